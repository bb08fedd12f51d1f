"""Developer timing of the buoyancy call (ocean_buoyancy_bodies_device) against what it replaces on the device side: one
ocean_query_surface_device over the same number of points, on the same build and the same frame.  Microseconds per call at a few
(bodies x points per body) shapes, 1 and 3 cascades, on a 512^2 tile; bodies scattered over +-700 m, one shared hull (instancing).
Device arrays (torch), HIP events on the context's stream around `reps` back-to-back calls behind a warm-up; K = 8.  The query's figure
leaves out what its caller then still has to do -- read two float4 per point back and sum them on the host.

    python tools/buoyancy_timing.py [--reps 50] [--log profiles/buoyancy_timing.txt]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(16, 4), (1000, 4), (1000, 16), (1000, 64), (100, 640), (16384, 64), (100000, 16)]


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

    out(f"buoyancy timing: device {torch.cuda.get_device_name(0)}, 512^2 tiles, K = 8, {args.reps} calls per figure (HIP events on the "
        f"context's stream); the query runs over bodies x points world points")
    out(f"{'casc':>4} {'bodies':>7} {'points':>6} {'buoyancy us':>12} {'query us':>9} {'ratio':>6} {'ns/point':>9} {'bytes back':>22}")
    lengths3 = [1000.0, 370.0, 93.0]
    rng = np.random.default_rng(0)
    for cascades in (1, 3):
        lengths = lengths3[:cascades]
        b = W.OceanBatch(512, cascades, 0)
        for i, L in enumerate(lengths):
            b.set_params(tile=i, tile_length=L)
        b.prepare(0x5EED0000)
        b.compute_waves(3.7)
        b.synchronize()
        geo = dict(uv_scales=[lengths[0] / L for L in lengths], grid_size=512, vertex_distance=lengths[0] / 512, choppy=-1.0, iterations=8)
        stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()

        def timed(call):
            for _ in range(5):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.reps):
                call()
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.reps

        for bodies, points in SHAPES:
            hull = np.concatenate([rng.uniform(-1.0, 1.0, (points, 3)) * [3.0, 0.75, 1.5], np.full((points, 1), 0.4)], axis=1).astype(np.float32)
            b.set_hull(hull)
            rec = np.zeros(bodies, W.BODY_DTYPE)
            rec["pos"] = np.stack([rng.uniform(-700, 700, bodies), rng.uniform(-1, 1, bodies), rng.uniform(-700, 700, bodies)], axis=1)
            yaw = rng.uniform(0, 2 * np.pi, bodies)
            rec["quat"][:, 1], rec["quat"][:, 3] = np.sin(yaw / 2), np.cos(yaw / 2)
            rec["vel"] = rng.normal(0, 2, (bodies, 3))
            rec["points"] = points
            d_bodies = torch.from_numpy(rec.view(np.int32).reshape(-1, 16)).cuda()
            force = torch.empty((bodies, 4), dtype=torch.float32, device="cuda")
            torque = torch.empty_like(force)
            # the world points the caller of the query would have formed on the host: here only their number and spread matter
            xz = torch.from_numpy((np.repeat(rec["pos"][:, [0, 2]], points, axis=0) + np.tile(hull[:, [0, 2]], (bodies, 1))).astype(np.float32)).cuda()
            pos = torch.empty((bodies * points, 4), dtype=torch.float32, device="cuda")
            nrm = torch.empty_like(pos)
            torch.cuda.synchronize()
            us_b = timed(lambda: b.buoyancy_device(d_bodies.data_ptr(), bodies, force.data_ptr(), torque.data_ptr(), **geo))
            us_q = timed(lambda: b.query_surface_device(xz.data_ptr(), bodies * points, pos.data_ptr(), nrm.data_ptr(), **geo))
            out(f"{cascades:>4} {bodies:>7} {points:>6} {us_b:>12.1f} {us_q:>9.1f} {us_b / us_q:>6.2f} {us_b * 1e3 / (bodies * points):>9.3f} "
                f"{32 * bodies:>10} vs {32 * bodies * points:>8}")
        b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
