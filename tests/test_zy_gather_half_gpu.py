"""ocean_gather_maps_f16 and k_pack_half, read back for the first time: every half the gather delivers against the plain restatement
tests/half_maps.pack_half (numpy's float32 -> float16 cast, itself held to an integer-only restatement by tests/test_half_maps.py) of the
fp32 maps, bit for bit.  One GPU is enough: a one-rank RCCL communicator makes the gather a device-local copy, as in
test_zz_multi_gpu.py::test_rccl_gather_of_sharded_tiles[1].  The work runs in a child process (tests/workers/gather_half_worker.py), so
that RCCL stays out of the pytest process; the file sorts just before test_zz_multi_gpu.py for the reason given there.

What the child compares (np.array_equal on uint16 views throughout; for a NaN input only "is a NaN"):
  a. real maps: 64^2 x 3 tiles (tile-major order shows) and 256^2 x 1, FULL7 and JACOBIAN; the fp32 maps read afterwards are bit-equal to
     a context's that never gathered;
  b. every rounding boundary: tests/half_maps.boundary_table() written into a caller-bound displacement map and, reversed, into the
     normal map (each value meets both lanes of a half2 and both words of the uint2), a few NaNs; +-inf exactly from 65520 on;
  c. 4096^2 x 1, the smallest tile whose pack launch (grid capped at 65535 workgroups of 256) takes a second trip of its stride loop:
     the first trip, the last 256 texels and the whole arrays, named separately;
  d. order and buffer reuse: 2 depth + 1 frames in flight at depths 1, 2, 3, each gathered into its own sentinel-filled buffer, one
     synchronisation at the end, against a serial context; then an fp32 and an f16 gather of each frame back to back, in both orders;
  e. lifetime: a new tile size (the pack buffers are freed with the map sets and made again), then a new communicator;
  f. errors that must launch nothing: before ocean_comm_init and before any frame OCEAN_E_NOT_READY; a root out of range and a NULL
     receive pointer on the root OCEAN_E_INVALID; the receive arrays keep their sentinel.

A child that dies from a signal or runs into the time limit fails the test; it is never run again."""
import os
import re
import subprocess
import sys
import time

import pytest

from test_zz_multi_gpu import _env

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "workers", "gather_half_worker.py")

SMALL_CASES = (["errors"]
               + [f"real_maps_n{n}_tiles{t}_{m}" for n, t in ((64, 3), (256, 1)) for m in ("full7", "jacobian")]
               + ["rounding_boundaries"]
               + [f"order_depth{d}{s}" for d in (1, 2, 3) for s in ("", "_fp32_then_f16", "_f16_then_fp32")]
               + ["lifetime_new_tile_size", "lifetime_new_communicator"])
BIG_CASES = ["second_trip_first_trip", "second_trip_tail", "second_trip_whole"]


def run_worker(which, cases, timeout):
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-X", "faulthandler", WORKER, which], capture_output=True, text=True, env=_env(), timeout=timeout)
    except subprocess.TimeoutExpired as e:
        pytest.fail(f"gather_half_worker {which}: no end after {timeout} s (hung?)\n{(e.stdout or b'')[-2000:]}\n{(e.stderr or b'')[-2000:]}", pytrace=False)
    print(f"gather_half_worker {which}: {time.perf_counter() - t0:.1f} s")
    print(r.stdout)
    died = r.returncode < 0 or r.returncode in (134, 139)
    assert r.returncode == 0, (f"status {r.returncode}{' (died from a signal)' if died else ''}", r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    reported = [m.group(1) for m in (re.match(r"CASE (\S+) (OK|FAIL)", ln) for ln in lines) if m]
    assert sorted(reported) == sorted(cases), (reported, cases)            # every case ran, none twice, none unknown
    for c in cases:
        assert f"CASE {c} OK" in lines, [ln for ln in lines if ln.startswith(f"CASE {c}")]
    assert lines[-1] == "GATHER_HALF_OK", lines[-3:]


def test_f16_gather_delivers_the_restated_halves():
    """Cases a, b, d, e, f."""
    run_worker("small", SMALL_CASES, 300)


def test_f16_gather_second_trip_of_the_pack_loop_at_4096():
    """Case c."""
    run_worker("big", BIG_CASES, 300)
