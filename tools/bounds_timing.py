"""Developer timing of the surface bounds.

1. ocean_build_bounds_tiles at first_level 1 and 4 against ocean_build_mips_tiles on the same range, at 512^2 and 2048^2 with 1 and 4
   tiles.  The only expectation comes from bytes: the bounds build moves N^2 * (16 + 32/3) B per tile at first_level 1 and about N^2 * 16 B
   at first_level 4, the mip set N^2 * (32 + 32/3) B, so the build at first_level 1 should not take longer than ocean_build_mips_tiles.
   The sum of the two is printed as well: a caller who wants both reads the displacement map twice.
2. ocean_patch_bounds_device for 65536 rectangles over 4 cascades (2048^2, 4 tiles), without and with six planes.

HIP events on the context's stream around `reps` back-to-back calls behind a warm-up; the sides of a comparison alternate, `rounds` times
each, and every round is printed: the spread of the rounds is the margin a difference has to beat.

    python tools/bounds_timing.py [--reps 200] [--rounds 5] [--log profiles/bounds_timing.txt]
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
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    def timed(stream, call):
        """microseconds per call: `reps` calls between two events on the context's stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(args.reps):
            call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.reps

    def compare(b, stream, sides):
        for _ in range(20):
            for call in sides:
                call()
        b.synchronize()
        times = [[] for _ in sides]
        for _ in range(args.rounds):
            for t, call in zip(times, sides):
                t.append(timed(stream, call))
        return times

    def fmt(v):
        return f"median {np.median(v):8.1f}  min {min(v):8.1f}  max {max(v):8.1f}  rounds [" + " ".join(f"{x:.1f}" for x in v) + "]"

    out(f"surface bounds timing: device {torch.cuda.get_device_name(0)}, {args.reps} calls per round, {args.rounds} rounds, "
        f"the sides alternating (HIP events on the context's stream), microseconds per call")
    for n in (512, 2048):
        for tiles in (1, 4):
            b = W.OceanBatch(n, tiles, 0)
            for i in range(tiles):
                b.set_params(tile=i, tile_length=LENGTHS[i])
            b.prepare(0x5EED0000)
            b.compute_waves(3.7)
            b.synchronize()
            stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()
            mips, lvl1, lvl4 = compare(b, stream, [lambda: b.build_mips_tiles(0, tiles), lambda: b.build_bounds_tiles(0, tiles, 1),
                                                   lambda: b.build_bounds_tiles(0, tiles, 4)])
            texels = tiles * n * n
            mb = lambda per_texel: texels * per_texel / 1e6
            out(f"N {n:>5} tiles {tiles}  bytes moved: mips {mb(32 + 32 / 3):.1f} MB, bounds first_level 1 {mb(16 + 32 / 3):.1f} MB, first_level 4 {mb(16 + 32 / 3 / 64):.1f} MB")
            out(f"    ocean_build_mips_tiles                 {fmt(mips)}")
            out(f"    ocean_build_bounds_tiles first_level 1 {fmt(lvl1)}")
            out(f"    ocean_build_bounds_tiles first_level 4 {fmt(lvl4)}")
            verdict = "not longer than" if np.median(lvl1) <= np.median(mips) else "LONGER than"
            out(f"    first_level 1 takes {verdict} ocean_build_mips_tiles (medians {np.median(lvl1):.1f} vs {np.median(mips):.1f}); "
                f"both behind one frame, the map read twice: {np.median(mips) + np.median(lvl1):.1f}")
            if n == 2048 and tiles == 4:
                count = 65536
                rng = np.random.default_rng(1)
                width = LENGTHS[0]
                centre = rng.uniform(-0.5 * width, 0.5 * width, (count, 2))
                size = width / 64 * np.exp2(rng.uniform(-2.0, 3.0, (count, 2)))          # 4 .. 125 m: 8 .. 256 texels of tile 0
                rects = np.concatenate([centre - 0.5 * size, centre + 0.5 * size], axis=1).astype(np.float32)
                scales = [LENGTHS[0] / L for L in LENGTHS]
                planes = [[1, 0, 0, 300], [-1, 0, 0, 300], [0, 0, 1, 300], [0, 0, -1, 300], [0, 1, 0, 50], [0, -1, 0, 50]]
                d_in = torch.from_numpy(rects).cuda()
                d_out = torch.empty((2, count, 4), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                b.build_bounds_tiles(0, tiles, 4)
                plain, culled = compare(b, stream, [
                    lambda: b.patch_bounds_device(d_in.data_ptr(), count, d_out[0].data_ptr(), d_out[1].data_ptr(), 0, scales, 1024, width / 1024),
                    lambda: b.patch_bounds_device(d_in.data_ptr(), count, d_out[0].data_ptr(), d_out[1].data_ptr(), 0, scales, 1024, width / 1024, planes)])
                b.synchronize()
                cls = d_out[1, :, 3].cpu().numpy()
                out(f"    ocean_patch_bounds_device, {count} rectangles of 4 .. 125 m over 4 cascades (set at first_level 4)")
                out(f"      no planes                            {fmt(plain)}")
                out(f"      six planes                           {fmt(culled)}   classes 0/1/2: " + "/".join(str(int((cls == k).sum())) for k in (0, 1, 2)))
            b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
