"""CPU: geometric_adv_amd.evaluate_attack against tests/golden/evaluate_attack.npz, which tools/make_golden_evaluate_attack.py
made by running the reference's own attacker/evaluate_attack.py on the same synthetic attack folder (three distance weights,
planted ties in source Chamfer + target reconstruction error); the single-weight case and the refusal of the plot flags."""
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_evaluate_attack as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "evaluate_attack.npz"))


def _inputs(golden):
    conf = json.loads(str(golden["conf_json"]))
    per_class = {c: (golden["adversarial_metrics__" + c], golden["adversarial_pc_input_dists__" + c]) for c in conf["class_names"]}
    return conf, per_class


def _run(top, *extra):
    from geometric_adv_amd import evaluate_attack
    evaluate_attack.main(["--top_dir", str(top), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy"] + list(extra))


def test_fixture_inputs_are_the_tools():
    """The fixture's inputs are what the tool draws (so a regenerated fixture covers the same ground), with ties planted."""
    from geometric_adv_amd import evaluate_attack  # noqa: F401  (numpy only: imports without a GPU)
    conf, per_class = G.synthetic_inputs()
    golden = np.load(os.path.join(GOLDEN, "evaluate_attack.npz"))
    assert json.loads(str(golden["conf_json"])) == conf
    ties = 0
    for c, (m, d) in per_class.items():
        assert np.array_equal(golden["adversarial_metrics__" + c], m)
        assert np.array_equal(golden["adversarial_pc_input_dists__" + c], d)
        norm = m[:, :, 2] + m[:, :, 4]
        ties += int(np.sum(np.sum(norm == norm.min(axis=0), axis=0) > 1))
    assert ties > 5


def test_matches_reference_run(tmp_path, golden):
    conf, per_class = _inputs(golden)
    att = G.write_attack_folder(str(tmp_path), conf, per_class)
    _run(tmp_path)
    for c in conf["class_names"]:
        for base in G.INDEX_FILES:
            got = np.load(os.path.join(att, c, "analysis_results", base + ".npy"))
            want = golden[base + "__" + c]
            assert got.dtype == want.dtype and got.shape == want.shape, (c, base, got.dtype, got.shape)
            assert np.array_equal(got, want), (c, base)
    for t in G.TEXTS:
        with open(os.path.join(att, "over_classes", t)) as f:
            assert f.read() == str(golden[t]), t
    assert not os.path.exists(os.path.join(att, "lamp"))


def test_single_weight_selects_weight_zero(tmp_path, golden):
    conf, per_class = _inputs(golden)
    conf = dict(conf, dist_weight_list=[1.0])
    per_class = {c: (m[:1], d[:1]) for c, (m, d) in per_class.items()}
    att = G.write_attack_folder(str(tmp_path), conf, per_class)
    _run(tmp_path)
    for c in conf["class_names"]:
        sel = np.load(os.path.join(att, c, "analysis_results", "source_target_norm_min_idx.npy"))
        assert sel.shape == (per_class[c][0].shape[1],) and not sel.any()
        m = per_class[c][0][0]
        norm = (m[:, 2] + m[:, 4]).reshape(conf["num_pc_for_attack"], -1)
        per_class_idx = np.load(os.path.join(att, c, "analysis_results", "source_target_norm_min_per_target_class_idx.npy"))
        t = conf["num_pc_for_target"]
        want = np.stack([np.argmin(norm[:, k * t:(k + 1) * t], axis=1) for k in range(per_class_idx.shape[1])], axis=1)
        assert per_class_idx.dtype == np.int16 and np.array_equal(per_class_idx, want)


@pytest.mark.parametrize("flag", ["--save_graphs", "--save_pc_plots"])
def test_plot_flags_are_refused(tmp_path, golden, flag):
    conf, per_class = _inputs(golden)
    att = G.write_attack_folder(str(tmp_path), conf, per_class)
    with pytest.raises(SystemExit, match="matplotlib"):
        _run(tmp_path, flag, "1")
    assert not os.path.exists(os.path.join(att, "over_classes"))
