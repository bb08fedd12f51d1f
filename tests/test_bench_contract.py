"""bench.py's CPU-checkable contract: flag defaults, byte accounting, the self-launcher and the CPU baseline leg on a tiny size."""
import importlib
import json
import os
import subprocess
import sys

import pytest

import line_schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    return importlib.import_module("bench")


def test_defaults_are_one_gpu_and_bounded(bench):
    a = bench.parse([])
    assert a.gpus == 1 and a.steps > 0 and a.warmup >= 0
    assert a.size == 2048 and a.tiles == 1            # BASELINE.json: the 2048x2048 single-tile configuration
    assert 1 <= a.depth <= 8


def test_byte_accounting(bench):
    # this pipeline's own bytes are what roofline.achieved uses ...
    assert sum(bench.KERNEL_BYTES_ACTUAL.values()) == bench.FRAME_BYTES_ACTUAL == 73
    # ... SURVEY.md 8d's model is kept beside it: 12 (h0 + omega) + 16 * 3.5 (intermediates out and in) + 32 (maps) + 8
    assert bench.FRAME_BYTES_SURVEY == 12 + 16 * 3.5 + 32 + 8 == 108
    assert sum(bench.KERNEL_BYTES_SURVEY.values()) == 108
    assert set(bench.KERNEL_BYTES_SURVEY) == set(bench.KERNEL_BYTES_ACTUAL) == {"k_zpass", "k_xpass_b", "k_xpass_disp"}
    assert bench.HBM_PEAK_GBPS == 8000.0


def test_roofline_object_uses_own_bytes_and_never_exceeds_peak_on_them(bench):
    names = ["k_zpass", "k_xpass_b", "k_xpass_disp"]
    n2 = 2048 * 2048
    r = bench.roofline_object(2048, 1, names, [0.027, 0.029, 0.0205], [0.06, 0.05, 0.04], 3, 0.054, 77.0, 73.0)
    assert r["kernel"] == "k_xpass_b" and r["algorithmic_bytes_per_launch"] == 28 * n2
    assert r["achieved"] == pytest.approx(28 * n2 / 29e-6 * 1e-9) and r["frac"] == pytest.approx(r["achieved"] / 8000.0)
    assert r["frame_frac"] == pytest.approx(73 * n2 / 54e-6 * 1e-9 / 8000.0) and r["frame_frac"] < 1.0
    assert "MODEL" in r["survey_model"]["what"] and "frac" not in r["survey_model"]       # the 108 figure is never a fraction of peak
    assert set(r["kernels"]) == set(names)


def _full_run(bench, argv=()):
    """A fully populated run (--full) as bench.py's main() assembles it: every object the stdout line and the sidecar are built from."""
    a = bench.parse(["--full", *argv])
    names = ["k_zpass", "k_xpass_b", "k_xpass_disp"]
    n, tiles = a.size, a.tiles
    w = tiles * n * n / 2048 ** 2                      # (durations scaled with the work of one launch: 8 x 1024^2 is twice a 2048^2 tile)
    roof = bench.roofline_object(n, tiles, names, [0.0221234567 * w, 0.0200345678 * w, 0.0166456789 * w], [0.0349 * w, 0.0492 * w, 0.0349 * w], a.depth,
                                 0.0498765432 * w, 58.123456789 * w, 73.0, dict(zip(names, (23, 28, 22))))
    cpu = {"value": 22.643211234, "unit": "frames/s", "cores": 16, "nproc": 256, "kind": "port", "fft": "own", "cores_note": "x" * 300,
           "sample": "20 frames of the same 2048x2048 7-field workload after 2 warm-up frames, median (44.2 ms/frame); FFTW not available on this host: " + "y" * 400,
           "stage_ms_of_the_median_frame": {"spectra": 1.0, "fft": 40.0, "pack": 2.0, "normalise": 1.2}, "gtexels_per_s": 0.0949, "host": {"cpu_model": "z" * 60, "nproc": 256},
           "config1_256x256_height_only_cpu_ms": 0.9}
    strong = dict(cpu, value=66.6123456789, cores=64, candidates_ms_per_frame={f"candidate {i} " + "c" * 80: 15.0 + i for i in range(10)})
    gather = bench.gather_report(1024, 8, 8, 8, 0, 0.118e-3, 3.9e-3, 3.6e-3, 1.9e-3, True)      # what measure_gather hands over on 8 ranks
    timing = {"regions": 9, "steps_per_region": a.steps, "statistic": "median over the regions", "ms_per_step_median": 0.0498765432, "ms_per_step_mean": 0.0501,
              "ms_per_step_p10": 0.0484, "ms_per_step_p90": 0.0504, "ms_per_step_min": 0.048, "ms_per_step_max": 0.052,
              "ms_per_step_of_each_region_in_order": [0.05] * 9, "what": "t" * 300}
    extra = {f"configuration_{i}": {"size": 512, "us_per_step": 16.5 + i, "what": "e" * 200, "kernel_us": {k: 5.0 for k in names}} for i in range(24)}
    return a, names, roof, cpu, strong, gather, timing, extra


def test_stdout_line_is_compact_strict_json_and_the_rest_goes_to_the_sidecar(bench):
    """the driver stopped parsing the line when it grew to 20.4 KB (16.4 KB still parsed).  The stdout line carries the
    contract's keys with compact roofline / cpu_baseline / gather / timing objects -- below 8 KB with every measurement populated, strict JSON --
    and everything else (extra, per-kernel tables, every note) goes to bench_extra.json + stderr."""
    for argv, world in (((), 1), (("--gpus", "8", "--size", "1024", "--tiles", "8", "--depth", "2"), 8)):
        a, names, roof, cpu, strong, gather, timing, extra = _full_run(bench, argv)
        line = bench.build_line(a, world, a.size, a.tiles, 20052.123456789, 0.0498765432, roof, gather, cpu, strong, timing, "a5cbb90d78459412")
        data = bench.encode_line(line)
        assert data.endswith(b"\n") and data.count(b"\n") == 1 and len(data) < bench.LINE_BYTES_MAX == 8192
        assert len(data) < 4096, len(data)                     # (in practice about 3 KB: room for the driver's 8 KB tail as well)
        back = json.loads(data, parse_constant=lambda c: pytest.fail(f"non-strict JSON constant {c}"))
        assert back == line
        for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                    "roofline", "cpu_baseline"):
            assert key in back, key
        assert "extra" not in back and set(back["config"]) >= {"workload", "tile_size", "tiles_per_rank", "pipeline_depth"}
        r = back["roofline"]
        assert set(r) >= {"bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "launch_us", "rocprof_launch_us", "frame_frac", "serial_frame_frac", "kernels"}
        assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-5)
        assert set(back["cpu_baseline"]) == {"value", "unit", "cores", "nproc", "kind", "fft", "sample"} and len(back["cpu_baseline"]["sample"]) <= 160
        assert back["cpu_baseline_strong"]["value"] == pytest.approx(66.6123, rel=1e-4)
        assert back["gather"]["rccl_ranks_seen"] == 8 and back["gather"]["compute_gather_overlapped_tiles_per_s"] == pytest.approx(64 / 3.6e-3, rel=1e-5)
        line_schema.check_contract_line(back, world)
        line_schema.check_gather(back["gather"], 8)
        assert back["timing"]["ms_per_step_p10"] <= back["ms_per_step"] <= back["timing"]["ms_per_step_p90"] and back["timing"]["regions"] == 9
        assert back["sidecar"] == bench.SIDECAR and back["build_id"] == "a5cbb90d78459412" and len(back["kernel_source_sha16"]) == 16
        side = bench.build_sidecar(line, a, roof, gather, extra, cpu, strong, timing)
        assert side["line"] == line and side["extra"] == extra and side["roofline"]["kernels"] and "bytes_model" in side["roofline"]
        assert side["cpu_baseline"]["host"] and side["speedup_vs_cpu_baseline_strong"] == pytest.approx(20052.1 / 66.6123, rel=1e-4)
        json.dumps(side)
    # non-finite numbers never reach the line as NaN / Infinity tokens
    a, names, roof, cpu, strong, gather, timing, extra = _full_run(bench)
    line = bench.build_line(a, 1, 2048, 1, float("nan"), float("inf"), roof, None, cpu, None, timing)
    assert line["value"] is None and line["ms_per_step"] is None and b"NaN" not in bench.encode_line(line)
    # an oversized line is a bug of the script, not something to emit
    with pytest.raises(RuntimeError):
        bench.encode_line(dict(line, junk="j" * 9000))


def test_plain_run_line_carries_the_headline_alone(bench):
    """A plain run (no --full) measures the headline only: its line keeps every contract key, null for what --full measures, and names
    no sidecar (none is written)."""
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs is None and bench.parse(["--full", "--dump-outputs", "d"]).full is True
    line = bench.build_line(a, 1, a.size, a.tiles, 2e4, 0.05, None, None, None, None, None, "a5cbb90d78459412")
    back = json.loads(bench.encode_line(line))
    for key in line_schema.CONTRACT_KEYS:
        assert key in back, key
    assert back["steps"] == 20 and back["warmup"] == 5 and back["ms_per_step"] == 0.05 and back["value"] == 2e4
    assert back["unit"] == "frames/s" and back["higher_is_better"] is True and back["dtype"] == "f32"
    assert back["roofline"] is None and back["cpu_baseline"] is None and back["gather"] is None and back["timing"] is None
    assert back["sidecar"] is None


class _FakeBatch:
    """What bench.dump_outputs reads of an OceanBatch: read_maps(), heights(i), tiles."""

    def __init__(self, n, tiles):
        import numpy as np
        rng = np.random.default_rng(n + tiles)
        self.tiles = tiles
        self.d = rng.standard_normal((tiles, n, n, 4), dtype=np.float32)
        self.q = rng.standard_normal((tiles, n, n, 4), dtype=np.float32)

    def read_maps(self):
        return self.d.copy(), self.q.copy()

    def heights(self, i):
        return 1.5 + i, -2.25 - i, 3.0 + i


@pytest.mark.parametrize("n,tiles", [(64, 2), (1024, 1), (2048, 1)])
def test_dump_outputs_writes_the_maps_or_a_fixed_sample_of_them(bench, tmp_path, n, tiles):
    """--dump-outputs: float32 / float64 .npy files, at most 64 MB in all; whole maps up to DUMP_TEXELS_MAX texels, above that the same
    seeded sample of texels in every run."""
    import numpy as np
    b = _FakeBatch(n, tiles)
    names = bench.dump_outputs(b, str(tmp_path / "a"))
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in names)
    assert all(v.dtype in (np.float32, np.float64) for v in got.values()) and sum(v.nbytes for v in got.values()) <= 64 << 20
    assert np.array_equal(got["heights"], np.array([b.heights(i) for i in range(tiles)], dtype=np.float32))
    texels = tiles * n * n
    if texels <= bench.DUMP_TEXELS_MAX:
        assert set(names) == {"displacement", "normal", "heights"}
        assert np.array_equal(got["displacement"], b.d) and np.array_equal(got["normal"], b.q)
        return
    assert set(names) == {"displacement", "normal", "heights", "sample_index"}
    idx = got["sample_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_TEXELS_MAX and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < texels
    assert np.array_equal(got["displacement"], b.d.reshape(-1, 4)[idx]) and np.array_equal(got["normal"], b.q.reshape(-1, 4)[idx])
    bench.dump_outputs(b, str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "sample_index.npy"), got["sample_index"])


def test_multi_gpu_line_carries_config5_workload_cpu_baseline_and_roofline(bench):
    """What rank 0 prints at N > 1: the documented config-5 invocation names the workload as BASELINE does,
    and the line keeps `cpu_baseline` and `roofline` (round 2 dropped both at N > 1)."""
    a = bench.parse(["--gpus", "8", "--size", "1024", "--tiles", "8", "--depth", "2", "--steps", "100", "--warmup", "20"])
    names = ["k_zpass", "k_xpass_b", "k_xpass_disp"]
    roof = bench.roofline_object(1024, 8, names, [0.045, 0.04, 0.03], [0.06, 0.05, 0.04], 2, 0.11, 120.0, 73.0,
                                 dict(zip(names, (23, 28, 22))))
    cpu = {"value": 20.0, "unit": "frames/s", "cores": 16, "kind": "port", "sample": "synthetic"}
    gather = bench.gather_report(1024, 8, 8, 8, 0, 64 / 5e5, 3.9e-3, 3.6e-3, 1.9e-3, True)
    line = bench.build_line(a, 8, 1024, 8, 5.6e5, 0.11, roof, gather, cpu, dict(cpu, value=80.0))
    # the SAME checks tests/test_zz_multi_gpu.py runs on the line of a real multi-GPU run (tests/line_schema.py): a key renamed in
    # bench.py fails here, on the CPU box, and not in the harness of the first 8-GPU run
    line_schema.check_multi_gpu_line(json.loads(bench.encode_line(line)), 8)
    for world in (2, 4):
        g = bench.gather_report(1024, 8, world, world, 0, 0.12e-3, 1.0e-3 * world, 0.9e-3 * world, 0.5e-3 * world, True)
        line_schema.check_multi_gpu_line(json.loads(bench.encode_line(bench.build_line(bench.parse(["--gpus", str(world)]), world, 2048, 1, 4e4, 0.05, roof, g, cpu, None))), world)
    with pytest.raises(AssertionError):
        line_schema.check_gather({"error": "the gather measurement did not finish within 240 s"}, 8)
    with pytest.raises(AssertionError):                 # the round-5 shape of the gather object (nested) is what the GPU test still read: refused now
        line_schema.check_gather(dict(line["gather"], compute_only={"tiles_per_s": 5e5}, compute_only_tiles_per_s=None), 8)
    assert line["n_gpus"] == 8 and line["scaling"] == "weak" and line["vs_baseline"] is None and line["dtype"] == "f32"
    assert line["config"]["workload"].startswith("64 x 1024x1024 tiles, 8 per GPU") and "BASELINE config 5" in line["config"]["workload"]
    assert line["config"]["tiles_per_rank"] == 8 and line["config"]["pipeline_depth"] == 2
    assert line["cpu_baseline"]["value"] == 20.0 and line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline_strong"]["value"] == 80.0
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and 0 < r["frac"] < 1 and r["kernel"] in names
    assert r["algorithmic_bytes_per_launch"] == r["kernels"][r["kernel"]]["bytes_per_texel"] * 1024 * 1024 * 8
    assert line["gather"]["rccl_ranks_seen"] == 8 and line["gather"]["compute_only_tiles_per_s"] == pytest.approx(5e5)
    assert line["warmup"] == 20 and line["prewarm_frames"] == a.prewarm
    bench.encode_line(line)
    # a single-GPU single-tile line still names the headline tile
    one = bench.build_line(bench.parse([]), 1, 2048, 1, 2e4, 0.05, roof, None, cpu, None)
    assert one["config"]["workload"].startswith("2048x2048 tile")


def test_stale_profile_summaries_are_not_quoted(bench, monkeypatch):
    """traffic / rocprof figures of profiles/*.json enter the line only while the kernel sources hash to what they were measured with."""
    names = ["k_zpass", "k_xpass_b", "k_xpass_disp"]
    r = bench.roofline_object(2048, 1, names, [0.025, 0.022, 0.0175], None, 1, 0.066, 66.0, 73.0)
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    current = t.get("_kernel_source_sha16") == bench.kernel_source_sha16()
    assert r["committed_profiles"]["current"] == current
    assert (r["traffic"] is not None) == current
    monkeypatch.setattr(bench, "kernel_source_sha16", lambda: "0" * 16)
    r = bench.roofline_object(2048, 1, names, [0.025, 0.022, 0.0175], None, 1, 0.066, 66.0, 73.0)
    assert r["traffic"] is None and r["rocprof_launch_us"] is None and r["rocprof_frac"] is None and all("traffic_bytes_per_launch" not in k for k in r["kernels"].values())
    assert bench.compact_roofline(r)["profiles_current"] is False


def test_cpu_baseline_leg_runs_and_reports_its_shape(bench):
    ref, strong = bench.cpu_baseline(64, 0.3)
    assert ref["kind"] == "port" and ref["unit"] == "frames/s" and ref["value"] > 0
    assert ref["cores"] >= 1 and "sample" in ref and ("FFTW not available" in ref["sample"] or ref["fft"] == "fftw3f")
    assert ref["host"]["nproc"] >= 1
    # (the strongest candidate of THIS run: the oracle's own FFT work-shared by a team, or scipy's pocketfft with stage D shared out -- which one
    #  wins depends on the host and on its load)
    assert strong["value"] > 0 and ("work-shared" in strong["sample"] or "shared out" in strong["sample"])
    # `cores` is the USABLE CPU count (min of the affinity mask and the cgroup quota) -- the team the sample really ran
    # with -- and the host's logical CPU count stands beside it (round 3 printed cores = 256 next to a quota of 16)
    usable, quota, aff, nproc = bench.usable_cpus()
    assert 1 <= usable <= aff <= nproc and (quota is None or usable <= int(quota + 0.999999))
    assert ref["cores"] == min(usable, ref["host"]["omp_max_threads"]) and ref["nproc"] == nproc == ref["host"]["nproc"]
    assert ref["host"]["usable_cpus"] == usable and f"{ref['cores']} threads" in ref["sample"]


def test_timed_regions_are_repeated_and_reported_as_median_with_spread(bench):
    """SURVEY.md 8d / VERDICT r03 #4: with --full the timed region of --steps frames is repeated K >= 7 more times inside one invocation;
    their median, p10 / p90 stand beside ms_per_step (the headline region).  (The GPU side is exercised by tests/test_parity_bench_regimes.py;
    here: the defaults and that the line keeps the contract's keys with the statistics added.)"""
    a = bench.parse([])
    assert a.regions >= 7
    assert bench.parse(["--regions", "11"]).regions == 11
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ("ms_per_step_p10", "ms_per_step_p90", "ms_per_step_median", "ms_per_step_mean", "steps_per_region"):
        assert key in src
    names = ["k_zpass", "k_xpass_b", "k_xpass_disp"]
    roof = bench.roofline_object(2048, 1, names, [0.025, 0.022, 0.0175], None, 1, 0.066, 66.0, 73.0)
    line = bench.build_line(a, 1, 2048, 1, 2e4, 0.05, roof, None, None, None)
    assert line["steps"] == a.steps and line["warmup"] == a.warmup and line["ms_per_step"] == 0.05
    # fewer than seven regions have no p10 / p90 worth the name: refused
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--regions", "3"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--regions must be >= 7" in r.stderr and "{" not in r.stdout


def test_config4_check_compares_saved_gpu_rows_with_the_float64_oracle(bench, tmp_path):
    """The CPU-baseline child's second job (VERDICT r03 #6a): frames the GPU side saved are compared with the float64 oracle per variant.
    Here the 'GPU frames' are the oracle's own float32-FFT frame (error at the fp32 floor) and a perturbed copy (error visible)."""
    import numpy as np
    from oracle import oracle as O
    n, t = 64, 1.0
    xi = O.gauss_xi_numpy(bench.SEED, n)
    o = O.Oracle(n)
    o.prepare(xi=xi)
    amp, d, q = o.compute_waves(t, fft=O.FFT_F32)
    rows = np.arange(0, n, 8)
    maps = np.concatenate([d[rows], q[rows]], axis=-1)
    bad = maps.copy(); bad[..., 0] += 1e-2 * np.abs(d[..., 0]).max()
    path = tmp_path / "check.npz"
    np.savez(path, n=n, t=t, rows=rows, names=np.array(["fp32", "broken"]), xi=xi, maps_fp32=maps, amp_fp32=amp, maps_broken=bad, amp_broken=amp)
    r = bench.check_frames_against_oracle(str(path))
    assert r["tile_size"] == n and r["rows_compared"] == len(rows)
    assert r["variants"]["fp32"]["max_err_over_max_channel"] < 1e-5 and r["variants"]["fp32"]["amplitude_rel_err"] < 1e-6
    assert 0.9e-2 < r["variants"]["broken"]["max_err_over_max_channel"] < 1.1e-2


def test_committed_profile_summaries_match_the_kernels(bench):
    """profiles/traffic.json (PMC-derived HBM bytes per launch) and profiles/kernel_stats.json (rocprofv3 durations)
    must name the kernels bench.py accounts for, and the measured traffic must stay near the algorithmic bytes."""
    t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    assert {k + "@2048" for k in bench.KERNEL_BYTES_ACTUAL} <= set(t)
    # the summaries say which kernel sources they were measured with; when those have moved on since, bench.py leaves the figures out
    # of its line (test_stale_profile_summaries_are_not_quoted) -- stale is allowed here, silently stale is not
    assert len(t["_kernel_source_sha16"]) == 16 and all(v.get("kernel_source_sha16") == t["_kernel_source_sha16"] for k, v in t.items() if not k.startswith("_"))
    if t["_kernel_source_sha16"] != bench.kernel_source_sha16():
        import warnings
        warnings.warn("profiles/traffic.json and kernel_stats.json were measured with other kernel sources: regenerate them "
                      "(tools/prof_round.sh, tools/pmc3.sh, tools/profile_summaries.py)")
    n2 = 2048 * 2048
    for k in bench.KERNEL_BYTES_ACTUAL:
        v = t[k + "@2048"]
        own = bench.KERNEL_BYTES_ACTUAL[k] * n2
        assert 0.85 * own <= v["hbm_bytes_per_launch"] <= 1.15 * own, (k, v["hbm_bytes_per_launch"], own)   # no wasted re-reads
        assert os.path.exists(os.path.join(ROOT, v["source"].split(" ")[0]))
    st = json.load(open(os.path.join(ROOT, "profiles", "kernel_stats.json")))
    for k in bench.KERNEL_BYTES_ACTUAL:
        assert st[k + "@2048"]["avg_us"] > 0 and os.path.exists(os.path.join(ROOT, st[k + "@2048"]["source"].split(" ")[0]))


def test_self_launcher_builds_a_torchrun_child_for_n_ranks(bench):
    a = bench.parse(["--gpus", "4", "--steps", "7"])
    cmd = bench.launch_command(a, ["--gpus", "4", "--steps", "7"])
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "7"] and cmd[-5].endswith("bench.py")


def test_bare_multi_gpu_run_refuses_instead_of_reporting_fewer_gpus():
    """`python bench.py --gpus 2` on a node with fewer GPUs must exit non-zero and print no JSON line
    (round 1 silently ran one rank and printed n_gpus = 1)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("node has >= 2 GPUs")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "n_gpus" not in r.stdout
    assert "refusing" in r.stderr


def test_world_size_mismatch_is_an_error():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode != 0 and "n_gpus" not in r.stdout and "refusing" in r.stderr


def test_committed_bench_line_is_reproducible_from_profiles(bench):
    """The committed default bench run (profiles/r06n_bench_default.json = the compact stdout line, profiles/r06n_bench_extra_default.json = its
    sidecar) against the committed rocprofv3 summary (profiles/kernel_stats.json <- r06n_kernel_stats_2048_bench_depth1.csv) and the byte
    accounting of this file: every kernel's fraction within 8 % of the one recomputed from the rocprofv3 average (two processes on two boxes: the
    hardware queue a context's stream lands on moves a kernel by up to +-1 us, profiles/r03_bimodal_probe.txt section 4a), nothing above 1, the
    line below the size limit, and the summaries regenerate from the CSV."""
    prof = os.path.join(ROOT, "profiles")
    raw = open(os.path.join(prof, "r06n_bench_default.json")).read()
    lines = [l for l in raw.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and len(lines[0]) < bench.LINE_BYTES_MAX
    d = json.loads(lines[0])
    side = json.load(open(os.path.join(prof, "r06n_bench_extra_default.json")))
    assert side["line"] == d
    st = json.load(open(os.path.join(prof, "kernel_stats.json")))
    r = d["roofline"]
    n2 = 2048 * 2048
    assert d["config"]["tile_size"] == 2048 and d["n_gpus"] == 1 and d["dtype"] == "f32" and d["vs_baseline"] is None
    assert r["profiles_current"] is True and r["traffic"] is not None and r["rocprof_launch_us"] is not None     # measured with the committed kernels
    for k, b in bench.KERNEL_BYTES_ACTUAL.items():
        frac_from_rocprof = b * n2 / (st[k + "@2048"]["avg_us"] * 1e-6) * 1e-9 / bench.HBM_PEAK_GBPS
        assert abs(r["kernels"][k]["frac"] - frac_from_rocprof) <= 0.08 * frac_from_rocprof, (k, r["kernels"][k]["frac"], frac_from_rocprof)
        assert r["kernels"][k]["frac"] < 1.0 and r["kernels"][k]["bytes_per_texel"] == b
    assert r["frac"] == r["kernels"][r["kernel"]]["frac"] and r["frame_frac"] < 1.0 and r["serial_frame_frac"] < 1.0
    assert r["rocprof_frac"] == pytest.approx(bench.KERNEL_BYTES_ACTUAL[r["kernel"]] * n2 / (r["rocprof_launch_us"] * 1e-6) * 1e-9 / bench.HBM_PEAK_GBPS, rel=1e-4)
    assert abs(r["frame_frac"] - bench.FRAME_BYTES_ACTUAL * n2 / (d["ms_per_step"] * 1e-3) * 1e-9 / bench.HBM_PEAK_GBPS) < 1e-5
    assert 0.85 * r["algorithmic_bytes_per_launch"] <= r["traffic"] <= 1.15 * r["algorithmic_bytes_per_launch"]           # no wasted re-reads
    # the timed region is repeated and reported as median with spread; the CPU baseline names the usable cores
    assert d["timing"]["regions"] >= 7 and d["timing"]["ms_per_step_p10"] <= d["ms_per_step"] <= d["timing"]["ms_per_step_p90"]
    assert d["cpu_baseline"]["cores"] <= d["cpu_baseline"]["nproc"] and d["cpu_baseline"]["cores"] == side["cpu_baseline"]["host"]["usable_cpus"]
    ex = side["extra"]
    assert {"4096x4096_fp32_depth3", "4096x4096_fp16_spectrum_depth3", "4096x4096_fp16_intermediates_depth3"} <= set(ex)
    assert ex["4096x4096_fp32_depth3"]["error_vs_float64_oracle"] <= 1e-5 < ex["4096x4096_fp16_spectrum_depth3"]["error_vs_float64_oracle"] <= 1e-3
    sc = ex["2048x2048_synchronous_calls"]
    assert sc["calls"] >= 1000 and sc["pinned_thread_gc_off"]["p95_over_median"] <= 1.25      # (host jitter of the box: 1.03-1.16 over this round's runs)
    # the driver's invocation, committed beside it: parsed line, the same keys
    short = json.loads([l for l in open(os.path.join(prof, "r06n_bench_steps20_warmup5.json")).read().splitlines() if l.startswith("{")][-1])
    assert short["steps"] == 20 and short["warmup"] == 5 and set(short) == set(d) and short["roofline"]["frac"] < 1.0
    # the summary itself regenerates from the committed CSV
    import csv
    import re
    acc = {}
    for row in csv.DictReader(open(os.path.join(prof, "r06n_kernel_stats_2048_bench_depth1.csv"))):
        m = re.search(r"(k_[a-z_0-9]+)<2048", row["Name"])
        name = m.group(1) if m else None
        if name and name.startswith("k_zpass"):          # the z pass's kernel forms (k_zpass, k_zpass_c1) are all the frame's first launch
            name = "k_zpass"
        if name in bench.KERNEL_BYTES_ACTUAL:
            a = acc.setdefault(name, [0, 0.0]); a[0] += int(row["Calls"]); a[1] += float(row["TotalDurationNs"])
    for k, (calls, total) in acc.items():
        assert abs(total / calls * 1e-3 - st[k + "@2048"]["avg_us"]) < 1e-6


def test_bench_py_refers_to_no_undefined_global(bench):
    """The GPU half of main() cannot run here; at least every name it (or any other function of the script) resolves at module level must
    exist -- a name that is neither assigned in its function nor defined at module level nor a builtin is a NameError waiting for the GPU
    box (round 5's first GPU run died of exactly that after the timed region)."""
    import builtins
    import symtable
    src = open(os.path.join(ROOT, "bench.py")).read()
    top = symtable.symtable(src, "bench.py", "exec")
    module_names = set(top.get_identifiers()) | set(dir(builtins)) | {"__file__", "__name__"}
    missing = []

    def walk(scope):
        for sym in scope.get_symbols():
            if sym.is_referenced() and sym.is_global() and sym.get_name() not in module_names:
                missing.append((scope.get_name(), sym.get_name()))
        for child in scope.get_children():
            walk(child)
    walk(top)
    assert not missing, missing


def test_cpu_baseline_child_does_not_inherit_the_launchers_single_thread(bench):
    """torch.distributed.run sets OMP_NUM_THREADS=1 for its ranks at nproc > 1: the CPU leg of an N > 1 run must not be timed on one thread."""
    env = bench.cpu_child_env({"OMP_NUM_THREADS": "1", "TORCHELASTIC_RUN_ID": "x", "RANK": "0", "WORLD_SIZE": "8", "LOCAL_WORLD_SIZE": "8", "PATH": "/usr/bin"})
    assert "OMP_NUM_THREADS" not in env and "RANK" not in env and "WORLD_SIZE" not in env and env["OMP_WAIT_POLICY"] == "PASSIVE" and env["PATH"] == "/usr/bin"
    # a user's own setting outside the launcher stands
    assert bench.cpu_child_env({"OMP_NUM_THREADS": "4"})["OMP_NUM_THREADS"] == "4"
