"""Developer timing of the water-velocity calls against the still-water calls they extend, modelled on tools/buoyancy_timing.py:
ocean_query_velocity_device against ocean_query_surface_device over the same points, and ocean_buoyancy_bodies_flow_device against
ocean_buoyancy_bodies_device over the same bodies.  A 2048^2 context of 2 tiles (a source and its derivative twin), one cascade, K = 8,
the (bodies x points per body) shapes of profiles/buoyancy_timing.txt; device arrays (torch), HIP events on the context's stream around
`reps` back-to-back calls behind a warm-up.  By count of gathers the velocity query does K + 2 map evaluations where the query does
K + 1, the extra one with half the bytes (the displacement map only).

    python tools/velocity_timing.py [--reps 50] [--log profiles/velocity_timing.txt]
    python tools/velocity_timing.py --baseline --tree <checkout of the parent commit, built>     # the two still-water calls on that library

--baseline times only the two still-water calls, on a 2-tile context without twins, and touches none of the new entry points, so it
runs on a checkout from before they existed (--tree: import the package from there)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(16, 4), (1000, 4), (1000, 16), (1000, 64), (100, 640), (16384, 64), (100000, 16)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--log", default=None)
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import watersurfacerendering_amd as W
    from watersurfacerendering_amd import _abi
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    n = args.size
    out(f"velocity timing{' (baseline: still-water calls only)' if args.baseline else ''}: device {torch.cuda.get_device_name(0)}, library build "
        f"{_abi.library_build_id()}, {n}^2, 2 tiles ({'no twins' if args.baseline else 'source + twin'}), 1 cascade, K = 8, {args.reps} calls "
        f"per figure (HIP events on the context's stream); the queries run over bodies x points world points")
    if args.baseline:
        out(f"{'bodies':>7} {'points':>6} {'query us':>9} {'buoyancy us':>12}")
    else:
        out(f"{'bodies':>7} {'points':>6} {'velocity us':>12} {'query us':>9} {'ratio':>6} {'flow us':>9} {'buoyancy us':>12} {'ratio':>6}")
    rng = np.random.default_rng(0)
    b = W.OceanBatch(n, 2, 0)
    if not args.baseline:
        b.set_velocity_twin(1, 0)
    b.prepare(0x5EED0000)
    b.compute_waves(3.7)
    b.synchronize()
    geo = dict(uv_scales=[1.0], grid_size=512, vertex_distance=1000.0 / 512, choppy=-1.0, iterations=8)
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
        xz = torch.from_numpy((np.repeat(rec["pos"][:, [0, 2]], points, axis=0) + np.tile(hull[:, [0, 2]], (bodies, 1))).astype(np.float32)).cuda()
        pos = torch.empty((bodies * points, 4), dtype=torch.float32, device="cuda")
        nrm = torch.empty_like(pos)
        torch.cuda.synchronize()
        us_q = timed(lambda: b.query_surface_device(xz.data_ptr(), bodies * points, pos.data_ptr(), nrm.data_ptr(), **geo))
        us_b = timed(lambda: b.buoyancy_device(d_bodies.data_ptr(), bodies, force.data_ptr(), torque.data_ptr(), **geo))
        if args.baseline:
            out(f"{bodies:>7} {points:>6} {us_q:>9.1f} {us_b:>12.1f}")
            continue
        us_v = timed(lambda: b.query_velocity_device(xz.data_ptr(), bodies * points, pos.data_ptr(), nrm.data_ptr(), **geo))
        us_f = timed(lambda: b.buoyancy_flow_device(d_bodies.data_ptr(), bodies, force.data_ptr(), torque.data_ptr(), **geo))
        out(f"{bodies:>7} {points:>6} {us_v:>12.1f} {us_q:>9.1f} {us_v / us_q:>6.2f} {us_f:>9.1f} {us_b:>12.1f} {us_f / us_b:>6.2f}")
    b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
