"""GPU: prepare_indices_for_attack's --get_rand_idx and --get_latent_nn_idx stages on the device against the files the
reference's own script wrote (tests/golden/prepare_indices.npz), and the pipeline they complete: a synthetic eval folder with
the latent codes of a random-init victim, prepare_indices_for_attack, then run_attack --target_pc_idx_type latent_nn with no
file supplied from outside, every attacked target being the source's nearest other-class neighbour in latent space."""
import os
import os.path as osp

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
N = 256
CLASSES, SIZES = ["chair", "table", "car"], [6, 6, 6]


def test_cli_on_the_gpu_writes_the_reference_files(tmp_path):
    from geometric_adv_amd import prepare_indices_for_attack
    g = np.load(osp.join(GOLDEN, "prepare_indices.npz"))
    ev = tmp_path / "log" / "ae" / "eval"
    os.makedirs(ev)
    np.save(ev / "pc_classes_4l.npy", g["pc_classes"])
    np.save(ev / "slice_idx_test_set_4l.npy", g["slice_idx"])
    np.save(ev / "latent_vectors_test_set_4l.npy", g["latent_vectors"])
    before = set(os.listdir(ev))
    prepare_indices_for_attack.main(["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--get_rand_idx", "1", "--get_latent_nn_idx", "1",
                                     "--num_instance_per_class", "6"])
    names = {"sel_idx_rand": "sel_idx_rand_6_test_set_4l.npy", "latent_dist_mat": "latent_dist_mat_test_set_4l.npy",
             "latent_nn_idx": "latent_nn_idx_test_set_4l.npy"}
    assert set(os.listdir(ev)) - before == set(names.values())
    for key, name in names.items():
        got = np.load(ev / name)
        assert got.dtype == g[key].dtype and got.shape == g[key].shape and np.array_equal(got, g[key]), key
    assert np.array_equal(np.load(ev / names["latent_dist_mat"]).view(np.uint32), g["latent_dist_mat"].view(np.uint32))


def _eval_folder(top):
    """<top>/log/ae: a random-init victim (weights.npz) and the eval folder tst_ae would write for 3 classes x 6 clouds."""
    from conftest import cloud
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    ev = top / "log" / "ae" / "eval"
    os.makedirs(ev)
    w = W.synthetic_weights(N)
    W.save_npz(str(top / "log" / "ae" / "weights.npz"), w)
    pcs = cloud(17, sum(SIZES), N)
    latent, recon, loss = PointNetAE(w, N).evaluate(pcs)
    slice_idx = np.concatenate([[0], np.cumsum(SIZES)])
    np.save(ev / "point_clouds_test_set_3l.npy", pcs)
    np.save(ev / "latent_vectors_test_set_3l.npy", latent)
    np.save(ev / "reconstructions_test_set_3l.npy", recon)
    np.save(ev / "ae_loss_test_set_3l.npy", loss)
    np.save(ev / "pc_classes_3l.npy", np.array(CLASSES))
    np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    return ev, pcs, latent, slice_idx


def test_pipeline_from_the_eval_folder_to_run_attack_with_latent_nn(tmp_path, monkeypatch):
    from geometric_adv_amd import adv_ae, prepare_indices_for_attack, run_attack
    from geometric_adv_amd.scorer import latent_dist_mat_host
    ev, pcs, latent, slice_idx = _eval_folder(tmp_path)
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae"]
    prepare_indices_for_attack.main(base + ["--get_rand_idx", "1", "--num_instance_per_class", "3", "--get_latent_nn_idx", "1"])
    sel = np.load(ev / "sel_idx_rand_3_test_set_3l.npy")
    assert sel.dtype == np.int16 and sel.shape == (3, 3) and all(sorted(r) == sorted(set(r)) and 0 <= min(r) and max(r) < 6 for r in sel.tolist())
    dist = latent_dist_mat_host(latent)
    assert np.array_equal(np.load(ev / "latent_dist_mat_test_set_3l.npy").view(np.uint32), dist.view(np.uint32))

    attacked = []                       # (source clouds, target clouds) of every AdvAE.attack call, one per source class
    attack = adv_ae.AdvAE.attack

    def recording_attack(self, source_pc, target_latent, target_pc, *args, **kwargs):
        attacked.append((np.array(source_pc), np.array(target_pc), np.array(target_latent)))
        return attack(self, source_pc, target_latent, target_pc, *args, **kwargs)

    monkeypatch.setattr(adv_ae.AdvAE, "attack", recording_attack)
    # 2 sources x 2 other classes x 1 target = 4 attacks per class: one batch of 4
    run_attack.main(base + ["--attack_pc_idx", "log/ae/eval/sel_idx_rand_3_test_set_3l.npy", "--target_pc_idx_type", "latent_nn",
                            "--num_pc_for_attack", "2", "--num_pc_for_target", "1", "--num_iterations", "3",
                            "--num_iterations_thresh", "2", "--batch_size", "4"])
    assert len(attacked) == len(CLASSES)
    index_of = lambda c: int(np.flatnonzero((pcs == c).all(axis=(1, 2)))[0])
    for i, name in enumerate(CLASSES):
        m = np.load(ev / "attack_res" / name / "adversarial_metrics.npy")
        assert m.shape == (1, 4, 5) and np.isfinite(m).all()
        assert np.load(ev / "attack_res" / name / "adversarial_pc_input.npy").shape == (1, 4, N, 3)
        src, tgt, tgt_latent = attacked[i]
        assert src.shape == tgt.shape == (4, N, 3)
        pairs = [(index_of(s), index_of(t)) for s, t in zip(src, tgt)]
        others = [j for j in range(len(CLASSES)) if j != i]
        want = []
        for k in sel[i, :2]:
            s = int(slice_idx[i] + k)
            for j in others:            # nearest neighbour of s inside class j: a plain argsort of the host matrix
                want.append((s, int(slice_idx[j] + np.argsort(dist[s, slice_idx[j]:slice_idx[j + 1]])[0])))
        assert pairs == want
        assert np.array_equal(tgt_latent, latent[[t for _, t in pairs]])
