"""Writes tests/golden/foam_n64.npz: the foam restatement (tests/foam.py) pinned on oracle maps, so that restatement and kernel cannot
drift together.  N = 64, the default sea (seed 7, L = 1000, lambda = -1), 20 steps of dt = 0.1 behind frames t_j = 0.1 j, default
foam parameters, both Jacobian sources (the normal map of a FULL7 frame, the Jacobian slot); checkpoints at steps 5 and 20, kept as
float32 (4 x 16 KiB before compression).  Run from the repository root:
    python tests/golden/make_foam_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

N, SEED, STEPS, DT, CHECKPOINTS = 64, 7, 20, 0.1, (5, 20)


def run():
    import foam as FM
    from oracle import oracle as O
    prep = O.numpy_prepare(N, O.gauss_xi_numpy(SEED, N))
    p = FM.params()
    dec = FM.decay(DT, p["lifetime"])
    state = {False: np.zeros((N, N), np.float32), True: np.zeros((N, N), np.float32)}
    out = {}
    for j in range(STEPS):
        _, d, q, _, _ = O.numpy_compute_waves(prep, np.float32(0.1) * np.float32(j), lam=-1.0, jacobian=True)
        d, q = d.astype(np.float32), q.astype(np.float32)
        for slot in (False, True):
            state[slot] = FM.step(state[slot], FM.jacobian(d, q, -1.0, slot), p, dec)
            if j + 1 in CHECKPOINTS:
                out[f"{'jacobian' if slot else 'normals'}_step{j + 1}"] = state[slot].copy()
    return out


if __name__ == "__main__":
    arrays = run()
    path = os.path.join(HERE, "foam_n64.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), {k: float(v.mean()) for k, v in arrays.items()})
