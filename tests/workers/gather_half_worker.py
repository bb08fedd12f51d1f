"""Child process of tests/test_zy_gather_half_gpu.py: ocean_gather_maps_f16 over a one-rank RCCL communicator (a device-local copy), every
received half compared bit for bit with tests/half_maps.pack_half of the fp32 maps.  `small` runs cases a, b, d, e, f of that file's
docstring, `big` the 4096^2 tile whose pack launch takes a second trip of its stride loop.  Prints one `CASE <name> OK` or
`CASE <name> FAIL <detail>` line per case and GATHER_HALF_OK when every case passed; a HIP or RCCL error ends the run at once."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import half_maps as H  # noqa: E402
import watersurfacerendering_amd as W  # noqa: E402
from watersurfacerendering_amd import _abi as A  # noqa: E402

SEED = 0x5EED0000
SENTINEL = 0x5A5A               # a finite half (209.25): a texel the gather never wrote shows
FAILED = []


def report(name, detail=None):
    if detail is None:
        print(f"CASE {name} OK", flush=True)
    else:
        FAILED.append(name)
        print(f"CASE {name} FAIL {detail}", flush=True)


def recv_pair(tiles, n, dtype=torch.int16):
    """Two device receive arrays [1 rank][tiles][n][n][4], pre-filled: halves with SENTINEL, floats with -1."""
    fill = SENTINEL if dtype == torch.int16 else -1.0
    return torch.full((2, 1, tiles, n, n, 4), fill, dtype=dtype, device="cuda")


def ptrs(r):
    return r[0].data_ptr(), r[1].data_ptr()


def halves(r):
    """The received pair as uint16 arrays [2][tiles][n][n][4]."""
    return r.cpu().numpy().view(np.uint16)[:, 0]


def diff(got, want, ignore=None):
    """None when the uint16 arrays agree (outside `ignore`), else where they first part."""
    bad = got != want
    if ignore is not None:
        bad &= ~ignore
    if not bad.any():
        return None
    at = np.unravel_index(int(np.argmax(bad)), bad.shape)
    return f"{int(bad.sum())} of {bad.size} halves differ; first at {tuple(int(x) for x in at)}: got 0x{int(got[at]):04x} want 0x{int(want[at]):04x}"


def compare(name, r, d, q, where=""):
    """The received pair against pack_half of the fp32 maps d, q; reports the case as failed (and returns False) where they part."""
    got = halves(r)
    for m, (what, src) in enumerate((("displacement", d), ("normal", q))):
        msg = diff(got[m], H.pack_half(src))
        if msg:
            report(name, f"{where}{what}: {msg}")
            return False
    return True


def new_comm(b):
    b.comm_init(1, 0, W.comm_unique_id())
    assert b.comm_count() == (1, 0)


def reference_frames(n, tiles, seed, times, mode=A.OCEAN_MODE_FULL7):
    """(disp, nrm) of each time from a serial context that never gathers."""
    ref = W.OceanBatch(n, tiles, 0)
    ref.set_mode(mode)
    ref.prepare(seed)
    out = []
    for t in times:
        ref.compute_waves(t)
        out.append(ref.read_maps())
    ref.close()
    return out


# ---- a. real maps --------------------------------------------------------------------------------------------------------------
def case_real_maps():
    for n, tiles in ((64, 3), (256, 1)):
        b = W.OceanBatch(n, tiles, 0)
        b.prepare(SEED + n)
        new_comm(b)
        for mode, tag in ((A.OCEAN_MODE_FULL7, "full7"), (A.OCEAN_MODE_JACOBIAN, "jacobian")):
            name = f"real_maps_n{n}_tiles{tiles}_{tag}"
            b.set_mode(mode)
            r = recv_pair(tiles, n)
            b.compute_waves(2.25)
            b.gather_maps(0, *ptrs(r), half=True)
            b.synchronize()
            d, q = b.read_maps()
            (rd, rq), = reference_frames(n, tiles, SEED + n, [2.25], mode)
            ok = compare(name, r, d, q)
            if ok and not (np.array_equal(d.view(np.uint32), rd.view(np.uint32)) and np.array_equal(q.view(np.uint32), rq.view(np.uint32))):
                report(name, "the fp32 maps changed under the f16 gather"); ok = False
            if ok and tiles > 1 and np.array_equal(d[0], d[1]):
                report(name, "tiles do not differ: the order would not show"); ok = False
            if ok and mode == A.OCEAN_MODE_JACOBIAN and not float(np.abs(d[..., 3] - 1.0).max()) > 0.01:
                report(name, "displacement.w is the constant 1"); ok = False
            if ok:
                report(name)
        b.comm_destroy(); b.close()


# ---- b. every rounding boundary ---------------------------------------------------------------------------------------------------
NAN_TEXELS = ((0, 7, 0), (1, 7, 1), (0, 200, 2), (1, 200, 3), (0, 65535, 1), (1, 65535, 0))      # (map, texel, channel)


def case_rounding_boundaries():
    name = "rounding_boundaries"
    n = 256
    bound = torch.zeros((2, 1, n, n, 4), dtype=torch.float32, device="cuda")
    b = W.OceanBatch(n, 1, 0)
    b.bind_output(bound[0].data_ptr(), bound[1].data_ptr())
    b.prepare(SEED)
    new_comm(b)
    b.compute_waves(1.0)
    b.synchronize()
    table = H.padded_table(n * n * 4)
    maps = np.stack([table, table[::-1]]).reshape(2, n * n, 4).copy()
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff8fffff, 0x7fffffff, 0x7fa00000], np.uint32).view(np.float32)
    for (m, texel, ch), v in zip(NAN_TEXELS, nans):
        maps[m, texel, ch] = v
    assert np.isnan(maps).sum() == len(NAN_TEXELS)
    bound.copy_(torch.from_numpy(maps.reshape(2, 1, n, n, 4)))
    torch.cuda.synchronize()
    r = recv_pair(1, n)
    b.gather_maps(0, *ptrs(r), half=True)
    b.synchronize()
    got = halves(r).reshape(2, n * n, 4)
    isnan = np.isnan(maps)
    want = H.pack_half(maps)
    ok = True
    for m in range(2):
        msg = diff(got[m], want[m], isnan[m])
        if msg:
            report(name, f"map {m}: {msg}"); ok = False
            break
    if ok:
        g = got[isnan]
        if not np.all(((g & 0x7c00) == 0x7c00) & ((g & 0x03ff) != 0)):
            report(name, f"NaN texels arrived as {[hex(int(x)) for x in g]}"); ok = False
    if ok:
        # +-inf exactly where the restatement says: |x| >= 65520 (and nowhere else), with the sign of x
        inf = ((got & 0x7fff) == 0x7c00)
        with np.errstate(invalid="ignore"):
            big = np.abs(maps) >= 65520.0
        if not (np.array_equal(inf, big) and np.array_equal((got[inf] & 0x8000) != 0, np.signbit(maps[inf]))):
            report(name, "infinities are not exactly the values from 65520 on"); ok = False
    b.bind_output(None, None)
    b.comm_destroy(); b.close()
    if ok:
        report(name)


# ---- c. the second trip of the stride loop ------------------------------------------------------------------------------------------
def case_second_trip():
    n = 4096
    first = 65535 * 256                                                   # texels of the first trip of the capped grid
    assert n * n - first == 256                                           # the last 256 texels ARE the second trip (no smaller map set has one)
    b = W.OceanBatch(n, 1, 0)
    b.prepare(SEED)
    new_comm(b)
    r = recv_pair(1, n)
    b.compute_waves(0.75)
    b.gather_maps(0, *ptrs(r), half=True)
    b.synchronize()
    d, q = b.read_maps()
    got = halves(r).reshape(2, n * n, 4)
    b.comm_destroy(); b.close()
    del r
    want = np.stack([H.pack_half(d), H.pack_half(q)]).reshape(2, n * n, 4)
    for name, sl in (("second_trip_first_trip", slice(0, first)), ("second_trip_tail", slice(n * n - 256, n * n)),
                     ("second_trip_whole", slice(0, n * n))):
        msg = None
        for m in range(2):
            msg = msg or diff(got[m, sl], want[m, sl])
        if name == "second_trip_tail" and not msg and not float(np.abs(d[0, -1, -256:, :3]).max()) > 0.0:
            msg = "the last 256 texels are zero: a tail never written would not show"
        report(name, msg)


# ---- d. order and buffer reuse, e. lifetime ------------------------------------------------------------------------------------------
def case_order_and_lifetime():
    n, tiles = 64, 3
    b = W.OceanBatch(n, tiles, 0)
    b.prepare(SEED + 1)
    new_comm(b)
    for depth in (1, 2, 3):
        b.set_pipeline_depth(depth)
        frames = 2 * depth + 1
        times = [0.25 * j + 0.1 * depth for j in range(frames)]
        ref = reference_frames(n, tiles, SEED + 1, times)
        # one f16 gather per frame, frames in flight, one synchronisation at the end
        name = f"order_depth{depth}"
        bufs = [recv_pair(tiles, n) for _ in range(frames)]
        for t, r in zip(times, bufs):
            b.compute_waves_async(t)
            b.gather_maps(0, *ptrs(r), half=True)
        b.synchronize()
        if all(compare(name, r, *ref[j], where=f"frame {j}, ") for j, r in enumerate(bufs)):
            report(name)
        # an fp32 and an f16 gather of each frame, back to back, in both orders
        for half_first in (False, True):
            name = f"order_depth{depth}_{'f16_then_fp32' if half_first else 'fp32_then_f16'}"
            b16 = [recv_pair(tiles, n) for _ in range(frames)]
            b32 = [recv_pair(tiles, n, torch.float32) for _ in range(frames)]
            for t, r16, r32 in zip(times, b16, b32):
                b.compute_waves_async(t)
                for half in ((True, False) if half_first else (False, True)):
                    b.gather_maps(0, *ptrs(r16 if half else r32), half=half)
            b.synchronize()
            ok = all(compare(name, r, *ref[j], where=f"frame {j}, ") for j, r in enumerate(b16))
            for j, r in enumerate(b32):
                g = r.cpu().numpy()[:, 0]
                if ok and not (np.array_equal(g[0].view(np.uint32), ref[j][0].view(np.uint32)) and np.array_equal(g[1].view(np.uint32), ref[j][1].view(np.uint32))):
                    report(name, f"fp32 gather of frame {j} differs"); ok = False
            if ok:
                report(name)
    # e. the pack buffers are freed with the map sets and made again at the new size; a new communicator serves the same context
    b.set_pipeline_depth(2)
    b.set_tile_size(128)
    b.prepare(SEED + 2)
    (rd, rq), = reference_frames(128, tiles, SEED + 2, [1.5])
    for name, again in (("lifetime_new_tile_size", False), ("lifetime_new_communicator", True)):
        if again:
            b.comm_destroy()
            new_comm(b)
        r = recv_pair(tiles, 128)
        b.compute_waves_async(0.5)
        b.compute_waves_async(1.5)
        b.gather_maps(0, *ptrs(r), half=True)
        b.synchronize()
        if compare(name, r, rd, rq):
            report(name)
    b.comm_destroy(); b.close()


# ---- f. errors ---------------------------------------------------------------------------------------------------------------------
def case_errors():
    name = "errors"
    n = 64
    b = W.OceanBatch(n, 1, 0)
    r = recv_pair(1, n)
    seen = []

    def code(*args):
        try:
            b.gather_maps(*args, half=True)
        except W.OceanError as e:
            return e.code
        return 0

    b.prepare(SEED)
    b.compute_waves(0.5)
    seen.append(("before comm_init", code(0, *ptrs(r)), A.OCEAN_E_NOT_READY))
    new_comm(b)
    b.prepare(SEED)                                                       # (a prepared context that has no frame yet)
    seen.append(("before any frame", code(0, *ptrs(r)), A.OCEAN_E_NOT_READY))
    b.compute_waves(0.5)
    seen.append(("root 1 of 1", code(1, *ptrs(r)), A.OCEAN_E_INVALID))
    seen.append(("root -1", code(-1, *ptrs(r)), A.OCEAN_E_INVALID))
    seen.append(("NULL displacement", code(0, None, r[1].data_ptr()), A.OCEAN_E_INVALID))
    seen.append(("NULL normal", code(0, r[0].data_ptr(), None), A.OCEAN_E_INVALID))
    b.synchronize()
    wrong = [s for s in seen if s[1] != s[2]]
    untouched = bool((halves(r) == SENTINEL).all())                       # no launch, no copy
    seen.append(("then a valid call", code(0, *ptrs(r)), 0))
    b.synchronize()
    d, q = b.read_maps()
    b.comm_destroy(); b.close()
    if wrong or seen[-1][1] != 0:
        report(name, f"(what, code, expected): {wrong or seen[-1]}")
    elif not untouched:
        report(name, "a refused call wrote into the receive arrays")
    elif compare(name, r, d, q):
        report(name)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "small"
    torch.cuda.set_device(0)
    cases = {"small": (case_errors, case_real_maps, case_rounding_boundaries, case_order_and_lifetime), "big": (case_second_trip,)}[which]
    for case in cases:
        t0 = time.perf_counter()
        try:
            case()
            print(f"TIME {case.__name__} {time.perf_counter() - t0:.2f} s", flush=True)
        except W.OceanError as e:                                          # the device or the communicator is in an unknown state: stop here
            report(case.__name__, f"{e}")
            print("GATHER_HALF_ABORTED", flush=True)
            return 1
    if FAILED:
        print(f"GATHER_HALF_MISMATCH {FAILED}", flush=True)
        return 1
    print("GATHER_HALF_OK", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
