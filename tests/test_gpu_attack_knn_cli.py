"""GPU: run_attack with the kNN outlier term on a tiny synthetic eval folder (built as tests/test_gpu_next_rows.py builds its
own): --knn_weight 5 writes adversarial_knn_loss.npy [W, num, 2] float64 = (K, masked points) of the saved adversarial clouds
and puts the three values into attack_configuration.json; a run without the flag writes no such file and the configuration
file of a run with the flag explicitly 0."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128


def _folder(top):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    from conftest import cloud
    sizes = [4, 5, 4]
    slice_idx = np.concatenate([[0], np.cumsum(sizes)])
    pcs = cloud(17, int(slice_idx[-1]), N)
    w = W.synthetic_weights(N)
    ev = top / "log" / "ae" / "eval"
    os.makedirs(ev)
    W.save_npz(str(top / "log" / "ae" / "weights.npz"), w)
    ae = PointNetAE(w, N)
    latent, loss = ae.transform(pcs), ae.get_loss_per_pc(pcs)
    rng = np.random.default_rng(0)
    nn_idx = np.zeros((len(pcs), len(pcs)), np.int16)
    for s in range(len(pcs)):
        for t in range(3):
            nn_idx[s, slice_idx[t]:slice_idx[t + 1]] = rng.permutation(sizes[t])
    attack_idx = np.stack([rng.permutation(4)[:2] for _ in sizes])
    np.save(ev / "point_clouds_test_set_3l.npy", pcs); np.save(ev / "latent_vectors_test_set_3l.npy", latent)
    np.save(ev / "pc_classes_3l.npy", np.array(["chair", "table", "car"])); np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    np.save(ev / "ae_loss_test_set_3l.npy", loss); np.save(ev / "chamfer_nn_idx_complete_test_set_3l.npy", nn_idx)
    np.save(ev / "sel_idx.npy", attack_idx)
    return ev


def test_run_attack_with_and_without_the_term(tmp_path):
    import torch
    from geometric_adv_amd import ops, run_attack
    ev = _folder(tmp_path)
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy", "--batch_size", "2",
            "--num_iterations", "12", "--num_iterations_thresh", "8", "--num_pc_for_attack", "2", "--num_pc_for_target", "1",
            "--dist_weight_list", "0.5", "2.0", "--class_names", "chair", "car"]
    run_attack.main(base + ["--output_folder_name", "plain"])
    run_attack.main(base + ["--output_folder_name", "zero", "--knn_weight", "0", "--knn_k", "7", "--knn_alpha", "2.5"])
    run_attack.main(base + ["--output_folder_name", "term", "--knn_weight", "5"])

    for cls in ("chair", "car"):
        a = np.load(ev / "term" / cls / "adversarial_pc_input.npy")
        kl = np.load(ev / "term" / cls / "adversarial_knn_loss.npy")
        assert a.shape == (2, 2, N, 3) and kl.shape == (2, 2, 2) and kl.dtype == np.float64
        for w in range(2):
            parts = ops.knn_outlier_loss(torch.as_tensor(a[w], device="cuda:0"), 5, 1.05, return_parts=True)
            assert kl[w, :, 0].tobytes() == parts[0].cpu().numpy().tobytes()
            assert np.array_equal(kl[w, :, 1], parts[3].sum(dim=1).cpu().numpy().astype(np.float64))
        assert np.isfinite(kl).all() and (kl >= 0).all()
    conf = json.load(open(ev / "term" / "attack_configuration.json"))
    assert (conf["knn_weight"], conf["knn_k"], conf["knn_alpha"]) == (5.0, 5, 1.05)

    # without the flag: no such file, and the bytes of a run with the flag explicitly 0 (which names none of the three values)
    for name in ("plain", "zero"):
        for cls in ("chair", "car"):
            assert "adversarial_knn_loss.npy" not in os.listdir(ev / name / cls)
    plain = open(ev / "plain" / "attack_configuration.json", "rb").read()
    assert plain == open(ev / "zero" / "attack_configuration.json", "rb").read()
    assert b"knn" not in plain
    assert sorted(json.loads(plain)) == sorted(k for k in conf if not k.startswith("knn_"))
    for cls in ("chair", "car"):
        assert "knn" not in open(ev / "plain" / cls / "attack_stats.txt").read()
        for f in ("adversarial_metrics.npy", "adversarial_pc_input.npy", "adversarial_pc_recon.npy"):
            assert np.load(ev / "plain" / cls / f).tobytes() == np.load(ev / "zero" / cls / f).tobytes()
