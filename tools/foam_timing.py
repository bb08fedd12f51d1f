"""Developer timing of the persistent foam: microseconds per k_foam_update and GB/s on its 24 B/texel (16 of the map texel, 4 of F in, 4 of F'
out) at 512^2, 2048^2, 4096^2 (one tile) and 8 x 1024^2, for both Jacobian sources (the normal map of a FULL7 frame, the Jacobian slot), beside
k_xpass_disp of the same context (22 B/texel, the yardstick of DESIGN.md section 6); and k_query_foam per point beside k_query_surface at 10^6
points, one and three cascades.  HIP events on the context's stream around `reps` back-to-back calls, behind at least 60 ms of the same work
(the shader clock needs load ahead of a timed window).  OCEAN_HIP_LIB names a variant library (tools/devlib.py), e.g. the
LDS form: make -C watersurfacerendering_amd/csrc variant NAME=foamlds DEFS=-DOCEAN_FOAM_LDS.

    python tools/foam_timing.py [--reps 200] [--only update|query] [--log profiles/foam_timing.txt] [--tag "row walk"]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import devlib  # noqa: E402,F401  (first: re-points the loader at OCEAN_HIP_LIB)


def timed(stream, call, reps, warm_ms=60.0):
    """us per call: events around `reps` calls, right behind warm_ms of the same calls."""
    import torch
    done = 0.0
    while done < warm_ms:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(100):
            call()
        e1.record(stream)
        e1.synchronize()
        done += max(e0.elapsed_time(e1), 0.05)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--only", choices=("update", "query"), default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import torch
    import watersurfacerendering_amd as W
    A = W._abi
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"foam timing{' [' + args.tag + ']' if args.tag else ''}: device {torch.cuda.get_device_name(0)}, library {os.path.basename(A.LIB_PATH)}, "
        f"{args.reps} calls per figure behind 60 ms of the same calls (HIP events on the context's stream)")
    if args.only in (None, "update"):
        out(f"{'tiles x N':>10} {'J source':>9} {'us/update':>10} {'GB/s @24':>9} {'k_xpass_disp us':>16} {'GB/s @22':>9} {'mean foam':>10}")
        for n, tiles in ((512, 1), (2048, 1), (4096, 1), (1024, 8)):
            for mode, name in ((A.OCEAN_MODE_FULL7, "normals"), (A.OCEAN_MODE_JACOBIAN, "jacobian")):
                b = W.OceanBatch(n, tiles, 0)
                b.set_mode(mode)
                b.prepare(0x5EED0000)
                b.compute_waves(3.7)
                _, per = b.time_frames(3.7, 0.016, 200, 200)            # serial frames: the yardstick kernel of this context
                xd = max(per[b.kernel_names().index("k_xpass_disp")] * 1e3, 1e-3)   # (ms per frame of that launch -> us)
                b.compute_waves(3.7)
                stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()
                us = timed(stream, lambda: b.update_foam(0.016), args.reps)
                texels = tiles * n * n
                mean = float(np.mean([b.read_foam(i).mean() for i in range(tiles)]))
                out(f"{str(tiles) + ' x ' + str(n):>10} {name:>9} {us:>10.2f} {texels * 24 / us * 1e-3:>9.0f} {xd:>16.2f} {texels * 22 / xd * 1e-3:>9.0f} {mean:>10.4f}")
                b.close()
    if args.only in (None, "query"):
        out(f"{'tile':>6} {'casc':>4} {'points':>8} {'k_query_foam us':>16} {'ns/point':>9} {'k_query_surface us':>19} {'ns/point':>9}")
        lengths3 = [1000.0, 370.0, 93.0]
        count = 1000000
        xz = torch.from_numpy(np.random.default_rng(1).uniform(-1000.0, 1000.0, (count, 2)).astype(np.float32)).cuda()
        res = torch.empty((count, 4), dtype=torch.float32, device="cuda")
        nrm = torch.empty_like(res)
        for n in (2048, 512):
            for cascades in (1, 3):
                lengths = lengths3[:cascades]
                b = W.OceanBatch(n, cascades, 0)
                for i, L in enumerate(lengths):
                    b.set_params(tile=i, tile_length=L)
                b.prepare(0x5EED0000)
                for j in range(10):
                    b.compute_waves(0.1 * j)
                    b.update_foam(0.1)
                b.synchronize()
                torch.cuda.synchronize()
                scales = [2.0 * lengths[0] / L for L in lengths]
                grid, vd = 512, 2.0 * lengths[0] / 512
                stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()
                reps = max(20, args.reps // 4)
                uf = timed(stream, lambda: b.query_foam_device(xz.data_ptr(), count, res.data_ptr(), 0, scales, grid, vd, -1.0, 8), reps)
                us = timed(stream, lambda: b.query_surface_device(xz.data_ptr(), count, res.data_ptr(), nrm.data_ptr(), 0, scales, grid, vd, -1.0, 8), reps)
                out(f"{n:>6} {cascades:>4} {count:>8} {uf:>16.1f} {uf * 1e3 / count:>9.3f} {us:>19.1f} {us * 1e3 / count:>9.3f}")
                b.close()
    if args.log:
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
