"""CPU: geometric_adv_amd.evaluate_classifier against tests/golden/classifier_eval.npz, which tools/make_golden_classifier_eval.py
made by running the reference's own classifier/evaluate_classifier.py on the same tiny pipeline tree (every data type, both
classification types, without and with correct_pred_only); the refusal of --save_graphs; tst_classifier's argument parser
and the naming rule of --save_pred_labels."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_classifier_eval as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "classifier_eval.npz"))


def _tree(golden):
    return {k[len("tree__"):]: golden[k] for k in golden.files if k.startswith("tree__")}


def test_fixture_inputs_are_the_tools(golden):
    """The fixture's tree is what the tool draws, every combination is recorded, and correct_pred_only changes a report."""
    t, want = _tree(golden), G.synthetic_tree()
    assert sorted(t) == sorted(want)
    for k in want:
        assert t[k].dtype == want[k].dtype and np.array_equal(t[k], want[k]), k
    texts = [k for k in golden.files if k.startswith("text__")]
    assert len(texts) == 2 * len(G.COMBOS) * 3
    differ = sum(str(golden[k]) != str(golden[k.replace("text__0__", "text__1__")]) for k in texts if k.startswith("text__0__"))
    assert differ >= 3


@pytest.mark.parametrize("correct_pred_only", [0, 1])
@pytest.mark.parametrize("data_type,classification_type", G.COMBOS)
def test_matches_reference_run(tmp_path, golden, data_type, classification_type, correct_pred_only):
    from geometric_adv_amd import evaluate_classifier
    att = G.write_tree(str(tmp_path), _tree(golden), correct_pred_only)
    evaluate_classifier.main(["--top_dir", str(tmp_path)] + G.cli_args(data_type, classification_type))
    out = G.report_dir(att, data_type)
    names = G.report_names(data_type, classification_type)
    assert sorted(os.listdir(out)) == sorted(names)
    for name in names:
        with open(os.path.join(out, name)) as f:
            assert f.read() == str(golden["text__%d__%s__%s__%s" % (correct_pred_only, data_type, classification_type, name)]), name


def test_save_graphs_is_refused(tmp_path, golden):
    from geometric_adv_amd import evaluate_classifier
    att = G.write_tree(str(tmp_path), _tree(golden), 0)
    args = G.cli_args("adversarial", "hit_target")
    args[args.index("--save_graphs") + 1] = "1"
    with pytest.raises(SystemExit, match="matplotlib"):
        evaluate_classifier.main(["--top_dir", str(tmp_path)] + args)
    assert not os.path.exists(G.report_dir(att, "adversarial"))


@pytest.mark.parametrize("flag,value", [("--data_type", "defended"), ("--classification_type", "hit_source")])
def test_wrong_types_are_refused(tmp_path, golden, flag, value):
    from geometric_adv_amd import evaluate_classifier
    G.write_tree(str(tmp_path), _tree(golden), 0)
    with pytest.raises(AssertionError, match="wrong"):
        evaluate_classifier.main(["--top_dir", str(tmp_path), flag, value])


# ---- tst_classifier: what needs no GPU -----------------------------------------------------------------------------------
def test_tst_classifier_parser_has_the_reference_defaults():
    from geometric_adv_amd import tst_classifier
    f = tst_classifier.build_parser().parse_args([])
    assert (f.gpu, f.model, f.batch_size, f.num_point, f.num_classes) == (0, "pointnet_cls", 2, 2048, 13)
    assert (f.model_path, f.dump_dir) == ("log/pointnet/model-150.ckpt", "log/pointnet/log_test")
    assert f.test_data == "log/autoencoder_victim/eval/point_clouds_test_set_13l.npy"
    assert f.test_labels == "log/autoencoder_victim/eval/pc_label_test_set_13l.npy"
    assert f.pc_classes == "log/autoencoder_victim/eval/pc_classes_13l.npy"
    assert (f.num_votes, f.save_pred_labels, f.top_dir) == (1, 0, ".")
    f = tst_classifier.build_parser().parse_args(["--num_votes", "12", "--save_pred_labels", "1", "--gpu", "3"])
    assert (f.num_votes, f.save_pred_labels, f.gpu) == (12, 1, 3)


def test_tst_classifier_pred_labels_name():
    from geometric_adv_amd import tst_classifier
    from geometric_adv_amd.attack_data import load_data
    got = tst_classifier.pred_labels_path(os.path.join("a", "eval", "pc_label_test_set_13l.npy"))
    assert got == os.path.join("a", "eval", "pc_pred_labels_test_set_13l.npy")
    assert "pc_pred_labels_test_set" in os.path.basename(got) and "pc_label_test_set" not in os.path.basename(got)
    assert load_data  # (the name is what attack_data.load_data looks up by 'pc_pred_labels_test_set')
    with pytest.raises(SystemExit, match="pc_label_"):
        tst_classifier.pred_labels_path(os.path.join("pc_label_dir", "labels_test_set.npy"))


def test_tst_classifier_refuses_other_models_and_bad_label_names_before_writing(tmp_path):
    from geometric_adv_amd import tst_classifier
    with pytest.raises(SystemExit, match="pointnet_cls_basic"):
        tst_classifier.main(["--top_dir", str(tmp_path), "--model", "pointnet_cls_basic"])
    with pytest.raises(SystemExit, match="pc_label_"):
        tst_classifier.main(["--top_dir", str(tmp_path), "--test_labels", "labels.npy", "--save_pred_labels", "1"])
    assert os.listdir(str(tmp_path)) == []
