"""Developer timing of the ray cast (ocean_raycast_surface_device): microseconds per call and nanoseconds per ray at 10^3 / 10^5 / 10^6
rays, 1 and 3 cascades, on 2048^2 and 512^2 tiles, steps 64 and 256 (refine 3, K = 8), for two ray sets over the same 2000 m mesh:
camera (a frustum from one eye 20 m above the water, 5..60 degrees below the horizon: neighbouring rays read neighbouring texels) and
random (origins anywhere over +-1000 m from under the water to 40 m above it, directions mostly downwards).  Device arrays (torch), HIP
events on the context's stream around `reps` back-to-back calls behind a warm-up.  tools/devlib.py first: OCEAN_HIP_LIB may point the
run at a variant library (crc: CRC-32 of the results, equal for two libraries that compute the same bits).

    python tools/raycast_timing.py [--reps 20] [--log profiles/raycast_timing.txt]
"""
import argparse
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import devlib  # noqa: E402,F401


def rays(kind, count, hmax, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "camera":
        side = int(np.ceil(np.sqrt(count)))
        yaw, pitch = np.meshgrid(np.linspace(-0.8, 0.8, side), np.linspace(np.radians(5.0), np.radians(60.0), side))
        d = np.stack([np.cos(pitch) * np.sin(yaw), -np.sin(pitch), np.cos(pitch) * np.cos(yaw)], axis=-1).reshape(-1, 3)[:count]
        o = np.broadcast_to(np.array([0.0, 20.0, -900.0]), d.shape)
    else:
        o = np.stack([rng.uniform(-1000, 1000, count), rng.uniform(-hmax - 2.0, hmax + 40.0, count), rng.uniform(-1000, 1000, count)], 1)
        d = rng.normal(size=(count, 3))
        d[:, 1] -= 0.6
    return np.concatenate([o, d], axis=1).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import watersurfacerendering_amd as W
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"ray cast timing: device {torch.cuda.get_device_name(0)}, library {os.path.basename(W._abi.LIB_PATH)}, K = 8, refine 3, "
        f"max_distance 1500 m, {args.reps} calls per figure (HIP events on the context's stream); mesh grid 512, vertex distance 1000/256")
    out(f"{'tile':>6} {'casc':>4} {'steps':>5} {'rays':>8} {'kind':>7} {'us/call':>9} {'ns/ray':>8} {'hit':>7} {'miss':>7} {'under':>7} {'crc':>8}")
    lengths3 = [1000.0, 370.0, 93.0]
    for n in (2048, 512):
        for cascades in (1, 3):
            lengths = lengths3[:cascades]
            b = W.OceanBatch(n, cascades, 0)
            for i, L in enumerate(lengths):
                b.set_params(tile=i, tile_length=L)
            b.prepare(0x5EED0000)
            amps = b.compute_waves(3.7)
            b.synchronize()
            hmax = 1.001 * float(np.sum(amps))
            scales = [2.0 * lengths[0] / L for L in lengths]
            grid, vd = 512, 2.0 * lengths[0] / 512
            stream = torch.cuda.ExternalStream(b.stream) if b.stream else torch.cuda.current_stream()
            for steps in (64, 256):
                for count in (1000, 100000, 1000000):
                    for kind in ("camera", "random"):
                        d_rays = torch.from_numpy(rays(kind, count, hmax, seed=count)).cuda()
                        hit = torch.empty((count, 4), dtype=torch.float32, device="cuda")
                        nrm = torch.empty_like(hit)
                        torch.cuda.synchronize()

                        def call():
                            b.raycast_surface_device(d_rays.data_ptr(), count, hit.data_ptr(), nrm.data_ptr(), 1500.0, steps, 3, 0,
                                                     scales, grid, vd, -1.0, 8)
                        for _ in range(3):
                            call()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        for _ in range(args.reps):
                            call()
                        e1.record(stream)
                        e1.synchronize()
                        us = e0.elapsed_time(e1) * 1e3 / args.reps
                        w = hit[:, 3].cpu().numpy()
                        crc = zlib.crc32(nrm.cpu().numpy().tobytes(), zlib.crc32(hit.cpu().numpy().tobytes()))
                        out(f"{n:>6} {cascades:>4} {steps:>5} {count:>8} {kind:>7} {us:>9.1f} {us * 1e3 / count:>8.2f} "
                            f"{int((w >= 0).sum()):>7} {int((w == -1).sum()):>7} {int((w == -2).sum()):>7} {crc:08x}")
            b.close()
    if args.log:
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
