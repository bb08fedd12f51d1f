"""Multi-GPU tests of the tile-sharded batch mode: they need at least two MI355X in the node and are
skipped otherwise (a gpurun box has one).  The file sorts last on purpose: on a multi-GPU node these are the first runs of the
gather over xGMI anywhere, and `pytest -x` must not let a surprise there hide the parity results.  One process per GPU, the library's own RCCL communicator
(ocean_comm_init / ocean_gather_maps), every rank's tiles compared on the root bit for bit."""
import os
import subprocess
import sys

import pytest

import line_schema

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gpus() -> int:
    import torch
    return torch.cuda.device_count()


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "OCEAN_BENCH_BACKEND")}
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return env


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_rccl_gather_of_sharded_tiles(world):
    if _gpus() < world:
        pytest.skip(f"needs {world} GPUs, node has {_gpus()}")
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                        "--master-addr", "127.0.0.1", "--master-port", str(port),
                        os.path.join(ROOT, "tests", "workers", "gather_worker.py")], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "GATHER_OK" in r.stdout, r.stdout[-2000:]


def test_bench_two_gpus_over_rccl():
    if _gpus() < 2:
        pytest.skip("needs 2 GPUs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "200", "--warmup", "50", "--prewarm", "100",
                        "--full", "--no-extra", "--cpu-seconds", "1"], capture_output=True, text=True, env=_env(), timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]          # a gather that fails or hangs exits non-zero (bench.py: give_up / failed)
    out = line_schema.last_json_line(r.stdout)
    # (the keys checked here are the ones tests/test_bench_contract.py checks on a synthetic world-8 line: one schema, tests/line_schema.py)
    line_schema.check_multi_gpu_line(out, 2)


def _build_gather_demo(tmp_path):
    from watersurfacerendering_amd import _abi
    exe = tmp_path / "gather_demo"
    lib_dir = os.path.dirname(_abi.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                    "-D__HIP_PLATFORM_AMD__", os.path.join(ROOT, "tests", "cpp", "gather_demo.cpp"), "-o", str(exe),
                    "-L", lib_dir, "-locean_hip", "-Wl,-rpath," + lib_dir, "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_bench_config5_invocation_on_eight_gpus():
    """BASELINE config 5 as the timed workload: `bench.py --gpus 8 --size 1024 --tiles 8 --depth 2`."""
    if _gpus() < 8:
        pytest.skip("needs 8 GPUs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--size", "1024", "--tiles", "8", "--depth", "2",
                        "--steps", "200", "--warmup", "50", "--prewarm", "100", "--full", "--no-extra", "--cpu-seconds", "1"],
                       capture_output=True, text=True, env=_env(), timeout=1200)
    assert r.returncode == 0, r.stderr[-3000:]
    out = line_schema.last_json_line(r.stdout)
    line_schema.check_multi_gpu_line(out, 8)
    assert "BASELINE config 5" in out["config"]["workload"] and out["config"]["pipeline_depth"] == 2


@pytest.mark.parametrize("ranks", [1, 2, 8])
def test_cpp_host_shards_tiles_and_gathers_over_rccl(ranks, tmp_path):
    """tests/cpp/gather_demo.cpp: the batch mode from a plain C++ host through the C ABI -- one forked process per GPU,
    the RCCL id through pipes, the gather overlapped with the next batch; every rank's tiles verified on the root."""
    if _gpus() < ranks:
        pytest.skip(f"needs {ranks} GPUs, node has {_gpus()}")
    exe = _build_gather_demo(tmp_path)
    r = subprocess.run([str(exe), str(ranks), "256", "3", "6"], capture_output=True, text=True, env=_env(), timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    assert f"GATHER_OK ranks {ranks} tiles {3 * ranks}" in r.stdout
