"""Writes tests/golden/trainer_offsets.json: where the auto-encoder trainer's arena (csrc/train.hip) places the buffers that the
Python handle can see, in bytes from the parameter buffer, which is the arena's first block (TEST INFRASTRUCTURE; run ONCE on
the GPU, at the commit whose arena must be kept -- the parent of the change that carves the arena with Carver):

    python tools/make_golden_trainer_offsets.py [--out tests/golden/trainer_offsets.json]

Per case: "grads" and every item of PointNetAETrainer._state_view as [offset, element count] ("act", "mean", "inv_std", "scale",
"shift": one pair per encoder layer).  All of these blocks precede the ones sized by the device's CU count, so the file does not
depend on how the machine is partitioned.  tests/test_gpu_train.py imports CASES and offsets() from here and compares.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = {"b2_n64_chamfer": (2, 64, "chamfer"), "b2_n64_emd": (2, 64, "emd"), "b3_n128_chamfer": (3, 128, "chamfer")}
PER_LAYER = ("act", "mean", "inv_std", "scale", "shift")
SINGLE = ("idx1", "idx2", "pool_max", "pool_ties", "d1", "d2")


def offsets(name):
    """dict of one case: the placements in a freshly created trainer (needs the GPU)."""
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.trainer import PointNetAETrainer
    b, n, loss = CASES[name]
    tr = PointNetAETrainer(W.synthetic_weights(n), n, batch_size=b, loss=loss)
    base = tr.parameter_buffer().data_ptr()

    def at(view):
        return [view.data_ptr() - base, view.numel()]
    out = {"grads": at(tr.gradient_buffer())}
    for k in PER_LAYER:
        out[k] = [at(tr._state_view(k, i)) for i in range(5)]
    for k in SINGLE:
        out[k] = at(tr._state_view(k))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "trainer_offsets.json"))
    a = ap.parse_args()
    doc = {name: offsets(name) for name in CASES}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s (%d bytes)" % (a.out, os.path.getsize(a.out)))
    print(json.dumps(doc["b2_n64_emd"], sort_keys=True))


if __name__ == "__main__":
    main()
