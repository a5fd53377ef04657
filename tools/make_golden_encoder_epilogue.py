"""Writes tests/golden/encoder_epilogue_parent.npz: latent, adversarial cloud, gradient and perturbation after three attack steps
from seeded inputs under the f16x2 encoder arithmetic, on an MI355X (TEST INFRASTRUCTURE; run ONCE on the GPU, at the commit whose
bits the encoder forward must keep -- the parent of the change that forms the second fp16 piece with a mixed-precision FMA):

    python tools/make_golden_encoder_epilogue.py [--out tests/golden/encoder_epilogue_parent.npz]

tests/test_gpu_encoder_epilogue_bits.py imports CASES and compute() from here, rebuilds the same inputs and compares bit for bit.

Shapes: the smallest that reach each form of the forward (csrc/encoder_x3.hip) -- n = 2048 with B = 2 and B = 8 (the split form's
two instantiations: one / two workgroups per CU), B = 9 (a wave per 32 points), n = 160 and 161 with B = 3 (a cloud that is no
multiple of the 128-point tile; 161: a partly empty 32-point unit).  Backwards: the handle's default, the masked backward (reads
the forward's ReLU masks) and recompute_backward (re-runs the layers through xp_layer_lds, which shares the split).  A case whose
arrays total at most 64 KB is stored raw ("<case>/<array>"), any other as the SHA-256 of each array's bytes.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RAW_LIMIT = 64 * 1024
FILE_LIMIT = 300 * 1024
WEIGHT_SEED = 5
SHAPES = [(2048, 2), (2048, 8), (2048, 9), (160, 3), (161, 3)]
BACKWARDS = {"auto": {}, "masked": {"encoder_backward": "masked"}, "recompute": {"recompute_backward": True}}
CASES = ["n%d_b%d_%s" % (n, b, k) for n, b in SHAPES for k in BACKWARDS]
ARRAYS = ("latent", "adv", "grad", "pert")


def _clouds(seed, b, n):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)


_models = {}


def _model(n):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    if n not in _models:
        w = W.randomized_weights(n, seed=WEIGHT_SEED)
        _models[n] = (w, PointNetAE(w, n, encoder_arith="f16x2"))
    return _models[n]


def compute(case):
    """dict array name -> numpy array of one case (needs the GPU)."""
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    n, b, back = case.split("_")
    n, b = int(n[1:]), int(b[1:])
    w, ae = _model(n)
    assert ae.encoder_arith == "f16x2", case
    x, gt = _clouds(131 * n + b, b, n), _clouds(131 * n + b + 1, b, n)
    p0 = (1e-3 * np.random.default_rng(7 * n + b).standard_normal((b, n, 3))).astype(np.float32)
    at = AdvAE("golden", Configuration(batch_size=b, n_points=n, weights=w, learning_rate=1e-4, num_iterations=3,
                                       num_iterations_thresh=10 ** 6, **BACKWARDS[back]), ae=ae)
    at.set_inputs(x, gt, ae.transform(gt), 1.0)
    at.init_pert(p0, reset_optimizer=True)
    at.run(0, 3, 10 ** 6)
    at.status()
    out = {k: v.cpu().numpy() for k, v in at.peek().items() if k in ARRAYS}
    ae.status()
    assert set(out) == set(ARRAYS), case
    return out


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "encoder_epilogue_parent.npz"))
    a = ap.parse_args()
    out = {}
    for case in CASES:
        arrays = compute(case)
        raw = sum(v.nbytes for v in arrays.values()) <= RAW_LIMIT
        for k, v in arrays.items():
            assert np.isfinite(v).all(), (case, k)
            assert np.abs(v).max() > 0, (case, k)
            if raw:
                out["%s/%s" % (case, k)] = v
            else:
                out["%s/%s.sha256" % (case, k)] = np.array(sha256(v))
        print(case, "raw" if raw else "sha256", {k: v.shape for k, v in arrays.items()}, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    assert size < FILE_LIMIT, size
    print("wrote %s (%d bytes, %d keys)" % (a.out, size, len(out)))


if __name__ == "__main__":
    main()
