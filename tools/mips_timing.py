"""Developer timing of the mip set and the LOD vertex stage.

1. ocean_build_mips_tiles (at most two launches for the whole range) against ocean_build_mips called once per tile (log2 N launches
   each: what a caller had to do before), at 512^2 and 2048^2 with 1 and 4 tiles.  The floor of the new call is its traffic,
   N^2 * (32 + 32/3) bytes per tile, at the HBM peak of 8 TB/s.
2. ocean_displace_grid_lod against ocean_displace_grid_cascades on a 1024-quad grid over 4 cascades.

HIP events on the context's stream around `reps` back-to-back calls behind a warm-up; the two sides of a comparison alternate, `rounds`
times each, and every round is printed: the spread of the rounds is the margin a difference has to beat.

    python tools/mips_timing.py [--reps 200] [--rounds 5] [--log profiles/mips_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = [1000.0, 370.0, 93.0, 31.0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def timed(b, stream, call):
        """microseconds per call: `reps` calls between two events on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    def compare(b, stream, old, new):
        for _ in range(20):
            old(); new()
        b.synchronize()
        a, c = [], []
        for _ in range(args.rounds):
            a.append(timed(b, stream, old))
            c.append(timed(b, stream, new))
        return a, c

    def fmt(v):
        return f"median {np.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f}  rounds [" + " ".join(f"{x:.1f}" for x in v) + "]"

    out(f"mip set and LOD vertex stage timing: device {torch.cuda.get_device_name(0)}, {args.reps} calls per round, {args.rounds} rounds, "
        f"the two sides alternating (HIP events on the context's stream), microseconds per call")
    for n in (512, 2048):
        for tiles in (1, 4):
            b = W.OceanBatch(n, tiles, 0)
            for i in range(tiles):
                b.set_params(tile=i, tile_length=LENGTHS[i])
            b.prepare(0x5EED0000)
            b.compute_waves(3.7)
            b.synchronize()
            stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()

            def per_tile():
                for t in range(tiles):
                    _abi.check(b._L.ocean_build_mips(b._h, t), "ocean_build_mips")

            def whole_range():
                b.build_mips_tiles(0, tiles)
            old, new = compare(b, stream, per_tile, whole_range)
            mbytes = tiles * n * n * (32 + 32 / 3) / 1e6
            out(f"N {n:>5} tiles {tiles}  traffic {mbytes:7.1f} MB  floor at 8 TB/s {mbytes / 8.0:6.1f} us  launches {tiles * (n.bit_length() - 1)} -> {1 if n <= 64 else 2}")
            out(f"    ocean_build_mips x {tiles}      {fmt(old)}")
            out(f"    ocean_build_mips_tiles      {fmt(new)}   ({mbytes / np.median(new):.2f} TB/s)")
            if tiles == 4:
                grid, vd = 1024, LENGTHS[0] / 1024
                scales = [LENGTHS[0] / L for L in LENGTHS]
                sc = np.ascontiguousarray(scales, dtype=np.float32)
                lod = b._lod(1.0, 0)
                import ctypes as C
                p = sc.ctypes.data_as(C.POINTER(C.c_float))
                b.build_mips_tiles(0, tiles)

                def flat():
                    _abi.check(b._L.ocean_displace_grid_cascades(b._h, 0, tiles, grid, vd, p, -1.0), "ocean_displace_grid_cascades")

                def with_lod():
                    _abi.check(b._L.ocean_displace_grid_lod(b._h, 0, tiles, grid, vd, p, -1.0, C.byref(lod)), "ocean_displace_grid_lod")
                old, new = compare(b, stream, flat, with_lod)
                out(f"    1024-quad grid, 4 cascades, texels per vertex spacing " + " ".join(f"{s * n / grid:.2f}" for s in scales))
                out(f"    ocean_displace_grid_cascades {fmt(old)}")
                out(f"    ocean_displace_grid_lod      {fmt(new)}")
            b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
