"""Helper of tests/test_gpu_clear_grid.py (run as a subprocess: VAMP_AMD_CLEAR is read at context creation):
validates the seeded cage batch of clear_batch() and writes ok, n_e and whether the environment has a clearance
grid to the .npz path given."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mr-vamp_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def clear_batch(n=4096, seed=77):
    """set-B-like edges in the unit cube (scaled by the caller): a fifth of the way towards a second draw"""
    rng = np.random.default_rng(seed)
    s = rng.random((n, 7), dtype=np.float32)
    g = (s + (rng.random((n, 7), dtype=np.float32) - s) * np.float32(0.2)).astype(np.float32)
    return s, g


def main(out):
    import oracle_py as op
    import vamp_amd
    from test_c_abi import CAGE
    env = vamp_amd.Environment()
    for c in CAGE:
        env.add_sphere(vamp_amd.Sphere(c, 0.2))
    s, g = clear_batch()
    s, g = op.scale(s), op.scale(g)
    ok, n = vamp_amd.panda_0_0.validate_batch(s, g, env)
    hdr, _ = env.clear_grid()
    np.savez(out, ok=np.asarray(ok, bool), n=np.asarray(n, np.int32), grid=np.array(hdr is not None))


if __name__ == "__main__":
    main(sys.argv[1])
