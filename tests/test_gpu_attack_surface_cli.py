"""GPU: run_attack with the kNN term under the surface rule on the tiny synthetic eval folder of
tests/test_gpu_attack_knn_cli.py: --knn_weight 2 --knn_rule surface --knn_k 2 --knn_thresh T writes adversarial_knn_loss.npy
[W, num, 2] float64 = (K, masked points) of the saved adversarial clouds under THAT rule and puts the two new values into
attack_configuration.json; --knn_rule sor writes the files of a run that does not name the rule."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import _knn_loss_model as M  # noqa: E402
import _surface_loss_model as SM  # noqa: E402


def test_run_attack_under_the_surface_rule(tmp_path):
    import torch
    from geometric_adv_amd import ops, run_attack
    from test_gpu_attack_knn_cli import N, _folder
    ev = _folder(tmp_path)
    # the threshold: the median model score of the folder's first cloud, a float32 (its repr is exact on the command line and in JSON)
    first = np.load(ev / "point_clouds_test_set_3l.npy")[:1].astype(np.float32)
    T = float(np.float32(np.median(SM.scores(SM.dists(first, M.brute_idx(first, 2)), 2))))
    assert T > 0 and float(np.float32(float(repr(T)))) == T
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy", "--batch_size", "2",
            "--num_iterations", "12", "--num_iterations_thresh", "8", "--num_pc_for_attack", "2", "--num_pc_for_target", "1",
            "--dist_weight_list", "0.5", "2.0", "--class_names", "chair", "car"]
    run_attack.main(base + ["--output_folder_name", "surface", "--knn_weight", "2", "--knn_rule", "surface", "--knn_k", "2",
                            "--knn_thresh", repr(T)])
    run_attack.main(base + ["--output_folder_name", "unnamed", "--knn_weight", "2", "--knn_k", "2"])
    run_attack.main(base + ["--output_folder_name", "sor", "--knn_weight", "2", "--knn_k", "2", "--knn_rule", "sor", "--knn_thresh", "9.5"])
    run_attack.main(base + ["--output_folder_name", "plain"])
    run_attack.main(base + ["--output_folder_name", "plain_sor", "--knn_rule", "sor"])

    masked = 0
    for cls in ("chair", "car"):
        a = np.load(ev / "surface" / cls / "adversarial_pc_input.npy")
        kl = np.load(ev / "surface" / cls / "adversarial_knn_loss.npy")
        assert a.shape == (2, 2, N, 3) and kl.shape == (2, 2, 2) and kl.dtype == np.float64
        for w in range(2):
            parts = ops.knn_outlier_loss(torch.as_tensor(a[w], device="cuda:0"), 2, rule="surface", thresh=T, return_parts=True)
            assert kl[w, :, 0].tobytes() == parts[0].cpu().numpy().tobytes()
            assert np.array_equal(kl[w, :, 1], parts[3].sum(dim=1).cpu().numpy().astype(np.float64))
        assert np.isfinite(kl).all() and (kl >= 0).all()
        masked += int(kl[:, :, 1].sum())
    assert masked > 0, "no saved cloud has a point over the threshold: the comparison above would hold for any rule"
    conf = json.load(open(ev / "surface" / "attack_configuration.json"))
    assert (conf["knn_weight"], conf["knn_k"], conf["knn_rule"], conf["knn_thresh"]) == (2.0, 2, "surface", T)
    for cls in ("chair", "car"):
        stats = open(ev / "surface" / cls / "attack_stats.txt").read()
        assert "knn_rule='surface'" in stats and "knn_thresh=%r" % T in stats

    # --knn_rule sor: the files of a run that does not name the rule, with the term on and off; neither names the two values
    for named, unnamed in (("sor", "unnamed"), ("plain_sor", "plain")):
        one = open(ev / named / "attack_configuration.json", "rb").read()
        assert one == open(ev / unnamed / "attack_configuration.json", "rb").read()
        assert b"knn_rule" not in one and b"knn_thresh" not in one
        for cls in ("chair", "car"):
            assert sorted(os.listdir(ev / named / cls)) == sorted(os.listdir(ev / unnamed / cls))
            for f in sorted(os.listdir(ev / named / cls)):
                if f.endswith(".npy"):
                    assert np.load(ev / named / cls / f).tobytes() == np.load(ev / unnamed / cls / f).tobytes(), (named, cls, f)
            text = open(ev / named / cls / "attack_stats.txt").read()
            assert "knn_rule" not in text and "knn_thresh" not in text
            flags = lambda t: [ln for ln in t.splitlines() if ln.startswith("Train flags")]      # noqa: E731
            strip = lambda ln: ln.replace("output_folder_name='%s'" % named, "").replace("output_folder_name='%s'" % unnamed, "")  # noqa: E731
            assert [strip(ln) for ln in flags(text)] == [strip(ln) for ln in flags(open(ev / unnamed / cls / "attack_stats.txt").read())]
    assert b"knn" not in open(ev / "plain" / "attack_configuration.json", "rb").read()
    assert "adversarial_knn_loss.npy" in os.listdir(ev / "sor" / "chair") and "adversarial_knn_loss.npy" not in os.listdir(ev / "plain" / "chair")
