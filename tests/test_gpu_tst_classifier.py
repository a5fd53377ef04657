"""GPU: the tst_classifier command end to end on a tiny test set -- 3 classes, 9 clouds of 64 points, a saved checkpoint of
randomized weights and a batch size that does not divide the set: the four outputs in the reference's formats, the labels
against classify, and the pc_pred_labels file as attack_data.load_data finds it."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CLASSES = ["chair", "table", "car"]


@pytest.fixture(scope="module")
def weights():
    from geometric_adv_amd import cls_weights as CW
    return CW.synthetic_weights(3, seed=77)


def _tree(top, weights, labels_name="pc_label_test_set_3l.npy"):
    from geometric_adv_amd import tf_checkpoint
    ev = os.path.join(top, "log", "ae", "eval")
    os.makedirs(ev)
    os.makedirs(os.path.join(top, "log", "pointnet"))
    tf_checkpoint.write_checkpoint(os.path.join(top, "log", "pointnet", "model-150.ckpt"), weights)
    rng = np.random.default_rng(9)
    data = (rng.random((9, 80, 3)) - 0.5).astype(np.float32)             # 80 points stored, --num_point 64 read
    labels = np.array([0, 0, 0, 1, 1, 1, 1, 0, 1], np.int8)              # class 'car' is never seen
    np.save(os.path.join(ev, "point_clouds_test_set_3l.npy"), data)
    np.save(os.path.join(ev, labels_name), labels)
    np.save(os.path.join(ev, "pc_classes_3l.npy"), np.array(CLASSES))
    return ev, data, labels


def _args(top, labels_name="pc_label_test_set_3l.npy"):
    return ["--top_dir", top, "--batch_size", "4", "--num_point", "64", "--num_classes", "3", "--model_path",
            "log/pointnet/model-150.ckpt", "--dump_dir", "log/pointnet/log_test", "--test_data",
            "log/ae/eval/point_clouds_test_set_3l.npy", "--test_labels", "log/ae/eval/" + labels_name, "--pc_classes",
            "log/ae/eval/pc_classes_3l.npy"]


def test_cli_end_to_end(tmp_path, weights):
    from geometric_adv_amd import tst_classifier
    from geometric_adv_amd.attack_data import load_data
    from geometric_adv_amd.classifier import PointNetClassifier
    top = str(tmp_path)
    ev, data, labels = _tree(top, weights)
    res = tst_classifier.main(_args(top) + ["--save_pred_labels", "1"])
    want = PointNetClassifier(None, num_classes=3, weights=weights, batch_size=4).classify(data[:, :64])
    assert np.array_equal(res["pred"], want.astype(np.int64))

    dump = os.path.join(top, "log", "pointnet", "log_test")
    assert sorted(os.listdir(dump)) == ["log_test.txt", "pred_label.txt", "test_accuracy.npy"]
    with open(os.path.join(dump, "pred_label.txt")) as f:
        assert f.read() == "".join("%d, %d\n" % (p, l) for p, l in zip(want, labels))
    acc = np.load(os.path.join(dump, "test_accuracy.npy"))
    assert acc.shape == () and acc.dtype == np.float64 and float(acc) == np.sum(want == labels) / 9.0
    with open(os.path.join(dump, "log_test.txt")) as f:
        lines = f.read().split("\n")
    assert lines[0].startswith("Namespace(") and lines[1] == "Model restored."
    assert re.fullmatch(r"test mean loss: \d+\.\d{6}", lines[2])
    assert lines[3] == "test accuracy: %f" % float(acc)
    assert lines[4] == "test avg class acc: nan"                       # np.mean over the unseen class, as in the reference
    seen = [np.sum(labels == c) for c in range(3)]
    for c in range(2):
        assert lines[5 + c] == "%10s:\t%0.3f" % (CLASSES[c], np.sum((labels == c) & (want == c)) / float(seen[c]))
    assert lines[7] == "%10s:\t%0.3f" % ("car", float("nan"))
    assert float(lines[2].split(": ")[1]) == pytest.approx(res["mean_loss"], abs=1e-6)

    # the predicted labels, as every --correct_pred_only 1 consumer loads them
    files = [f for f in os.listdir(ev) if os.path.isfile(os.path.join(ev, f))]
    assert "pc_pred_labels_test_set_3l.npy" in files
    got = load_data(ev, files, ["pc_pred_labels_test_set"])
    assert got.dtype == np.int8 and got.shape == labels.shape and np.array_equal(got, want)
    assert np.array_equal(load_data(ev, files, ["pc_label_test_set"]), labels)


def test_votes_and_no_saved_labels_by_default(tmp_path, weights):
    from geometric_adv_amd import tst_classifier
    from geometric_adv_amd.classifier import PointNetClassifier
    top = str(tmp_path)
    ev, data, labels = _tree(top, weights)
    res = tst_classifier.main(_args(top) + ["--num_votes", "3"])
    want = PointNetClassifier(None, num_classes=3, weights=weights, batch_size=4).evaluate(data[:, :64], labels, num_votes=3)
    assert np.array_equal(res["pred"], want["pred"]) and res["mean_loss"] == want["mean_loss"]
    assert res["vote_loss"].shape == (3, 3)
    assert not any("pc_pred_labels" in f for f in os.listdir(ev))


def test_labels_file_name_without_pc_label_is_refused(tmp_path, weights):
    from geometric_adv_amd import tst_classifier
    top = str(tmp_path)
    _tree(top, weights, labels_name="labels_test_set_3l.npy")
    with pytest.raises(SystemExit, match="pc_label_"):
        tst_classifier.main(_args(top, "labels_test_set_3l.npy") + ["--save_pred_labels", "1"])
    assert not os.path.exists(os.path.join(top, "log", "pointnet", "log_test"))
