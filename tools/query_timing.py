"""Developer timing of the surface query (ocean_query_surface_device): microseconds per call at 10^3 / 10^5 / 10^6 points, 1 and 3
cascades, on 2048^2 and 512^2 tiles, for coherent points (a jittered grid, row by row) and random points over the same square.
Device arrays (torch), HIP events on the context's stream around `reps` back-to-back calls behind a warm-up; K = 8.

    python tools/query_timing.py [--reps 50] [--log profiles/query_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def points(kind, count, half, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.uniform(-half, half, (count, 2)).astype(np.float32)
    side = int(np.ceil(np.sqrt(count)))
    g = (np.arange(side, dtype=np.float32) + 0.5) * np.float32(2 * half / side) - np.float32(half)
    xz = np.stack(np.meshgrid(g, g), axis=-1).reshape(-1, 2)[:count]
    return (xz + rng.uniform(-0.4, 0.4, xz.shape) * np.float32(2 * half / side)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import watersurfacerendering_amd as W
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"surface query timing: device {torch.cuda.get_device_name(0)}, K = 8, {args.reps} calls per figure (HIP events on the "
        f"context's stream), points over +-1000 m (the mesh spans 2000 m: grid 512, vertex distance 1000/256)")
    out(f"{'tile':>6} {'casc':>4} {'points':>8} {'kind':>8} {'us/call':>9} {'ns/point':>9} {'p99 residual m':>15}")
    lengths3 = [1000.0, 370.0, 93.0]
    for n in (2048, 512):
        for cascades in (1, 3):
            lengths = lengths3[:cascades]
            b = W.OceanBatch(n, cascades, 0)
            for i, L in enumerate(lengths):
                b.set_params(tile=i, tile_length=L)
            b.prepare(0x5EED0000)
            b.compute_waves(3.7)
            b.synchronize()
            scales = [2.0 * lengths[0] / L for L in lengths]
            grid, vd = 512, 2.0 * lengths[0] / 512
            stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()
            for count in (1000, 100000, 1000000):
                for kind in ("coherent", "random"):
                    xz = torch.from_numpy(points(kind, count, 1000.0, seed=count)).cuda()
                    pos = torch.empty((count, 4), dtype=torch.float32, device="cuda")
                    nrm = torch.empty_like(pos)
                    torch.cuda.synchronize()

                    def call():
                        b.query_surface_device(xz.data_ptr(), count, pos.data_ptr(), nrm.data_ptr(), 0, scales, grid, vd, -1.0, 8)
                    for _ in range(5):
                        call()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    for _ in range(args.reps):
                        call()
                    e1.record(stream)
                    e1.synchronize()
                    us = e0.elapsed_time(e1) * 1e3 / args.reps
                    res = float(torch.quantile(nrm[:, 3].float().cpu(), 0.99))
                    out(f"{n:>6} {cascades:>4} {count:>8} {kind:>8} {us:>9.1f} {us * 1e3 / count:>9.3f} {res:>15.3g}")
            b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
