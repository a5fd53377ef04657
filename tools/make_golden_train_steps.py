"""Writes tests/golden/train_steps_parent.npz: what three training steps of the three layer-by-layer trainers (FoldingNet,
AtlasNet, the PointNet classifier) leave on an MI355X from seeded weights and clouds (TEST INFRASTRUCTURE; run ONCE on the GPU,
with the library built at the commit whose bits the steps must keep -- the parent of the change that moves their batch-norm,
pool and Adam kernels into csrc/train_bn.h):

    python tools/make_golden_train_steps.py [--out tests/golden/train_steps_parent.npz]

tests/test_gpu_train_step_bits.py imports CASES and compute() from here, rebuilds the same inputs and compares bit for bit.

Every case records, after the third step: the loss(es) of each step, the flat parameter and gradient buffers, both optimizer
slots, the running (moving) mean and variance of every batch-norm layer, and the last step's gmax_row / pool_argmax.  A case
whose arrays total at most 64 KB is stored raw ("<case>/<array>"), any other as the SHA-256 of each array's bytes
("<case>/<array>.sha256").  Every shape of the list the change was specified with is accepted by the trainers as it stands.
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
STEPS = 3

# name: (B, n, weight_decay, explicit picks)
FOLD = {
    "b2_n17": (2, 17, 1e-6, False),          # the lower limits; bn_bwd_fc with two rows
    "b3_n70": (3, 70, 1e-6, False),          # 210 rows: one ragged 256-row chunk
    "b5_n100": (5, 100, 1e-6, False),        # 500 rows: two chunks, the second ragged
    "wd_b3_n33": (3, 33, 0.1, False),        # the weight-decay term of Adam
    "picks_b2_n40": (2, 40, 1e-6, True),     # the given-picks path
}
# name: (B, n, nb_primitives, number_points, num_layers, decoder BN, explicit template)
ATLAS = {
    "b2_n1_q1_p1_l0": (2, 1, 1, 1, 0, True, False),          # gmax with n < 4; one decoder row per cloud
    "b3_n33_q2_p7_l1": (3, 33, 2, 14, 1, True, False),       # G = 2; ragged chunks
    "nobn_b3_n33_q2_p7_l1": (3, 33, 2, 14, 1, False, False), # remove_all_batchNorms: the BN = false apply
    "b5_n130_q3_p100_l2": (5, 130, 3, 300, 2, True, False),  # 500 decoder rows per primitive: more than one chunk per group
    "tmpl_b2_n20_q2_p5_l1": (2, 20, 2, 10, 1, True, True),   # the given-template path
}
# name: (B, n, num_classes, optimizer)
CLS = {
    "b1_n1_c1": (1, 1, 1, "adam"),           # the lower limits
    "b3_n70_c5_adam": (3, 70, 5, "adam"),    # ragged chunks
    "b3_n70_c5_momentum": (3, 70, 5, "momentum"),
    "b33_n40_c13": (33, 40, 13, "adam"),     # fc layers with more than 32 rows; 1320 point rows
}
CASES = ["fold_" + k for k in FOLD] + ["atlas_" + k for k in ATLAS] + ["cls_" + k for k in CLS]


def _clouds(seed, b, n):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)


def _flat(tr):
    """(params, grads): host copies of the trainer's flat buffers."""
    import torch
    from geometric_adv_amd import _lib
    torch.cuda.synchronize(tr.device)
    return tuple(_lib.device_view(p, tr._count, "<f4", tr.device).cpu().numpy().copy() for p in (tr._params_ptr, tr._grads_ptr))


_fold_state = []


def _fold(name):
    from geometric_adv_amd import fold_weights as FW
    from geometric_adv_amd.fold_trainer import FoldingNetTrainer
    B, n, wd, given = FOLD[name]
    if not _fold_state:
        _fold_state.append(FW.synthetic_state(0))
    tr = FoldingNetTrainer(weights=_fold_state[0], num_points=n, batch_size=B, weight_decay=wd, seed=11)
    losses = []
    for s in range(STEPS):
        x = _clouds(1000 * n + 10 * B + s, B, n)
        picks = None
        if given:       # seeded positions in [0, degree) of each point's adjacency row
            deg = tr.degrees(x).cpu().numpy()
            draw = np.random.default_rng(77 + s).integers(0, 1 << 30, (2, B, n, 16))
            picks = (draw % deg[None, :, :, None]).astype(np.int32)
        losses.append(tr.train_step(x, picks=picks))
    out = {"losses": np.asarray(losses, np.float32)}
    out["params"], out["grads"] = _flat(tr)
    out["slot1"], out["slot2"] = tr.state("slot1"), tr.state("slot2")
    for l in range(6):
        out["running_mean%d" % l], out["running_var%d" % l] = tr.state("running_mean", l), tr.state("running_var", l)
    out["gmax_row"] = tr.state("gmax_row")
    return out


def _atlas(name):
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlas_trainer import AtlasNetTrainer
    B, n, nb, points, nl, dbn, given = ATLAS[name]
    p = points // nb
    opt, state = AW.synthetic_state(nb, nl, dbn, seed=3, number_points_eval=max(4, min(p, 100)) * nb)
    opt["number_points"] = points
    tr = AtlasNetTrainer(weights=state, options=opt, num_points=n, batch_size=B, seed=13)
    assert tr.points_per_primitive == p and tr.decoder_bn == dbn, name
    losses = []
    for s in range(STEPS):
        tmpl = np.random.default_rng(55 + s).random((nb, p, 2), dtype=np.float32) if given else None
        losses.append(tr.train_step(_clouds(2000 * n + 10 * B + s, B, n), template=tmpl))
    out = {"losses": np.asarray(losses, np.float32)}
    out["params"], out["grads"] = _flat(tr)
    out["slot1"], out["slot2"] = tr.state("slot1"), tr.state("slot2")
    for l, layer in enumerate(tr.layers):
        if layer[4]:
            out["running_mean%d" % l], out["running_var%d" % l] = tr.state("running_mean", l), tr.state("running_var", l)
    out["gmax_row"] = tr.state("gmax_row")
    return out


def _cls(name):
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer
    B, n, nc, optimizer = CLS[name]
    tr = PointNetClassifierTrainer(weights=CW.synthetic_weights(nc, 5), num_points=n, batch_size=B, num_classes=nc,
                                   optimizer=optimizer, seed=17)
    losses = []
    for s in range(STEPS):
        labels = np.random.default_rng(31 + s).integers(0, nc, B)
        loss, pred = tr.train_step(_clouds(3000 * n + 10 * B + s, B, n), labels)
        losses.append(loss)
    out = {"losses": np.asarray(losses, np.float32), "pred": pred.astype(np.int32)}
    out["params"], out["grads"] = _flat(tr)
    out["slot1"], out["slot2"] = tr.state("slot1"), tr.state("slot2")
    for l, layer in enumerate(tr._shapes()):
        if layer[3]:
            out["moving_mean%d" % l], out["moving_var%d" % l] = tr.state("moving_mean", l), tr.state("moving_var", l)
    for i in range(3):
        out["pool_argmax%d" % i] = tr.state("pool_argmax", i)
    return out


def compute(case):
    """dict array name -> numpy array of one case (needs the GPU)."""
    kind, name = case.split("_", 1)
    return {"fold": _fold, "atlas": _atlas, "cls": _cls}[kind](name)


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_steps_parent.npz"))
    a = ap.parse_args()
    out = {}
    for case in CASES:
        arrays = compute(case)
        raw = sum(v.nbytes for v in arrays.values()) <= RAW_LIMIT
        for k, v in arrays.items():
            assert v.dtype.itemsize == 4, (case, k, v.dtype)
            assert np.isfinite(v).all() if v.dtype.kind == "f" else True, (case, k)
            if raw:
                out["%s/%s" % (case, k)] = v
            else:
                out["%s/%s.sha256" % (case, k)] = np.array(sha256(v))
        print(case, "raw" if raw else "sha256", {k: v.shape for k, v in arrays.items() if not k.startswith(("running", "moving"))},
              arrays["losses"].tolist(), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **out)
    size = os.path.getsize(a.out)
    assert size < FILE_LIMIT, size
    print("wrote %s (%d bytes, %d keys)" % (a.out, size, len(out)))


if __name__ == "__main__":
    main()
