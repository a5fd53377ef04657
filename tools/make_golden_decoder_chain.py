"""Writes tests/golden/decoder_chain_parent.npz: what the decoder chain of the auto-encoder (latent_decode, FC2 forward, FC2
backward, the backward's tail) gives on an MI355X for seeded inputs (TEST INFRASTRUCTURE; run ONCE on the GPU, at the commit
whose bits the chain must keep -- the parent of the change that reschedules the chain's loads):

    python tools/make_golden_decoder_chain.py [--out tests/golden/decoder_chain_parent.npz]

tests/test_gpu_decoder_chain_bits.py imports CASES and compute() from here, rebuilds the same inputs and compares bit for bit.

Forward cases ("fwd_n<N>_b<B>"): PointNetAE.transform -> z, max_and_argmax -> crit, reconstruct -> recon, decode(z) -> dec.
Step cases ("step_<name>"): AdvAE, three iterations at learning_rate 1e-4 -> pert, adv, recon, latent, grad (the step's whole
gradient, g_enc included) and the loss rows; each asserts the code path it is there for (STEP).  A case whose arrays total at
most 64 KB is stored raw ("<case>/<array>"), any other as the SHA-256 of each array's bytes ("<case>/<array>.sha256").
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

FORWARD = ([(n, b) for n in (1, 65, 200, 256) for b in (1, 31, 32, 33)]      # 3n % 32 != 0, row-block clamp, second row block
           + [(64, b) for b in (64, 65, 129)]                                  # latent_decode with 4 / 2 / 1 workgroups per cloud
           + [(2048, 2), (8192, 2)])                                           # 16 and 64 encoder tiles
# name: (n, B, Configuration fields, tied cloud 1, what compute() asserts of the path).  At default settings a handle with
# B * n < 4096 runs the two-scan Chamfer kernel and the masked encoder backward: its tail has no Jacobian to apply (n1_b2, n65_b5,
# n200_b3, n2048_b1 -- their split-K shapes are what they are here for); from 4096 points on the symmetric scan carries the pool
# Jacobian and the tail applies it (n256_b33, n2048_b33, n8192_b2, tied_n256_b17).  "symmetric": _test_plan()["symmetric"];
# "search": the paired grid search is in use (with the two-scan kernel it rides in latent_decode_and_grid_kernel: 1024 threads
# while 9 B <= 256, 512 beyond).
STEP = {
    "n1_b2": (1, 2, {}, False, {"symmetric": False}),                 # one chunk, empty split-K groups
    "n65_b5": (65, 5, {}, False, {"symmetric": False}),               # 4 chunks
    "n200_b3": (200, 3, {}, False, {"symmetric": False}),             # 10 chunks, ragged last chunk, uneven groups
    "jac_n200_b3": (200, 3, {"encoder_backward": "jacobian"}, False, {"symmetric": False}),   # the same with the Jacobian's apply
    "n256_b33": (256, 33, {}, False, {"symmetric": True}),
    "n2048_b1": (2048, 1, {}, False, {"symmetric": False}),           # 24 split-K loads per thread
    "n2048_b33": (2048, 33, {}, False, {"symmetric": True}),
    "n8192_b2": (8192, 2, {}, False, {"symmetric": True}),            # 384 chunks; tail and dense backward as two plain launches
    "masked_n256_b4": (256, 4, {"encoder_backward": "masked"}, False, {}),   # the tail without the Jacobian
    # cloud 1 = two copies of 128 points, perturbation included: every pool maximum is tied in the first forward, so the first
    # step's tail block publishes dz for the dense blocks of its launch (decoder_tail_dense_kernel: 17 + 16 workgroups)
    "tied_n256_b17": (256, 17, {}, True, {"symmetric": True}),
    # latent_decode_and_grid_kernel, both shapes: the two-scan kernel with the search on
    "grid1024_n2048_b6": (2048, 6, {"chamfer_kernel": "two_scan", "chamfer_prune": "always"}, False, {"symmetric": False, "search": True}),
    "grid512_n256_b29": (256, 29, {"chamfer_kernel": "two_scan", "chamfer_prune": "always"}, False, {"symmetric": False, "search": True}),
}
CASES = ["fwd_n%d_b%d" % nb for nb in FORWARD] + ["step_" + k for k in STEP]


def _clouds(seed, b, n):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)


_models = {}


def _model(n):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    if n not in _models:
        w = W.randomized_weights(n, seed=WEIGHT_SEED)        # non-zero biases: the chain's bias loads matter
        _models[n] = (w, PointNetAE(w, n))
    return _models[n]


def compute(case):
    """dict array name -> numpy array of one case (needs the GPU)."""
    import torch
    kind, rest = case.split("_", 1)
    if kind == "fwd":
        n, b = (int(s[1:]) for s in rest.split("_"))
        _, ae = _model(n)
        x = _clouds(1000 * n + b, b, n)
        z = ae.transform(x)
        _, crit = ae.max_and_argmax(x)
        recon, _ = ae.reconstruct(x, compute_loss=False)
        return {"z": z, "crit": crit.cpu().numpy(), "recon": recon, "dec": ae.decode(z)}
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    from geometric_adv_amd.adversary import init_pert_value
    n, b, fields, tied, path = STEP[rest]
    w, ae = _model(n)
    x, gt = _clouds(77 * n + b, b, n), _clouds(77 * n + b + 1, b, n)
    pert0 = init_pert_value(b, n)
    if tied:
        x[1, n // 2:] = x[1, :n // 2]
        pert0[1, n // 2:] = pert0[1, :n // 2]
    at = AdvAE("golden", Configuration(batch_size=b, n_points=n, weights=w, learning_rate=1e-4, num_iterations=3,
                                       num_iterations_thresh=10 ** 6, **fields), ae=ae)
    at.set_inputs(x, gt, ae.transform(gt), 1.0)
    at.init_pert(pert0, reset_optimizer=True)
    if "symmetric" in path:
        assert at._test_plan()["symmetric"] is path["symmetric"], case
    if "search" in path:
        assert at.search_state()[0] is path["search"], case
    if tied:    # the first forward's cloud 1: duplicated points and a positive maximum, so its tie flag is set
        first = at.peek()
        adv1 = first["adv"][1].cpu().numpy().view(np.uint32)
        assert (adv1[n // 2:] == adv1[:n // 2]).all() and bool((first["latent"][1] > 0).any()), case
    at.run(0, 3, 10 ** 6)
    at.status()
    out = {k: v.cpu().numpy() for k, v in at.peek().items() if k in ("pert", "adv", "recon", "latent", "grad")}
    losses = torch.empty((8, b), dtype=torch.float32, device=at.device)
    from geometric_adv_amd import _lib
    with torch.cuda.device(at.device):
        _lib.check(_lib.lib().geoadv_attack_test_loss_state(at._h, None, None, _lib.ptr(losses), None, None, _lib.stream_handle()),
                   "attack_test_loss_state")
    out["losses"] = losses.cpu().numpy()
    ae.status()
    return out


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "decoder_chain_parent.npz"))
    a = ap.parse_args()
    out = {}
    for case in CASES:
        arrays = compute(case)
        raw = sum(v.nbytes for v in arrays.values()) <= RAW_LIMIT
        for k, v in arrays.items():
            assert np.isfinite(v).all() if v.dtype.kind == "f" else True, (case, k)
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
