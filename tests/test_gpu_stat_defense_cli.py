"""GPU: run_defense_sor and run_defense_srs end to end on a tiny eval folder -- run_attack (two distance weights),
get_dists_per_point (whose files evaluate_attack reads), evaluate_attack, the two defenses with the sanity checks,
evaluate_defense on both folders and run_classifier on the SOR folder -- every written file checked by name, dtype, shape
and value against the library calls on the same inputs, the planted points of the clean sources among the points SOR removes,
and a rerun of the SRS command writing the same bytes."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stat_defense_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

N = 128
CLASSES, SIZES = ["chair", "table", "car"], [4, 5, 4]
ATTACKED = ["chair", "car"]
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 2, 2
NUM_KNN, ALPHA, DROP, SEED = 2, 1.1, 40, 9


def _planted(k):
    """The far-off points planted in chair cloud k: k + 1 of them, 0.1 apart."""
    return [7 * j + 3 for j in range(k + 1)]


def _test_set():
    """Clouds 0.06 wide; chair cloud k gets k + 1 far-off points 0.1 apart, car clouds none."""
    slice_idx = np.concatenate([[0], np.cumsum(SIZES)])
    pcs = ((np.random.default_rng(5).random((int(slice_idx[-1]), N, 3)) - 0.5) * 0.06).astype(np.float32)
    for k in range(SIZES[0]):
        for j, p in enumerate(_planted(k)):
            pcs[k, p] = np.float32([0.3 + 0.1 * j, 0.3, -0.2])
    return pcs, slice_idx


def _brute_knn(cloud, k):
    x = cloud.astype(np.float64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    return np.sort(d, axis=1)[:, 1:k + 1].astype(np.float32)


def test_the_rule_removes_the_planted_points_of_every_chair_cloud():
    """On the CPU, with brute-force distances: what the choice of the clouds rests on."""
    pcs, _ = _test_set()
    for k in range(SIZES[0]):
        scores = M.sor_scores(_brute_knn(pcs[k], NUM_KNN)[None], NUM_KNN)
        inl, (mu, var, m) = M.sor_inliers(scores, ALPHA)
        assert not inl[0][_planted(k)].any()
        assert scores[0][_planted(k)].min() > 2 * (mu[0] + ALPHA * np.sqrt(var[0]))      # by a margin no kNN rounding closes


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    from geometric_adv_amd import (cls_weights as CW, evaluate_attack, evaluate_defense, get_dists_per_point, run_attack,
                                   run_classifier, run_defense_sor, run_defense_srs, weights as W)
    from geometric_adv_amd.autoencoder import PointNetAE
    top = tmp_path_factory.mktemp("stat_defense_cli")
    ev = top / "log" / "ae" / "eval"
    os.makedirs(ev)
    pcs, slice_idx = _test_set()
    w = W.synthetic_weights(N)
    W.save_npz(str(top / "log" / "ae" / "weights.npz"), w)
    ae = PointNetAE(w, N)
    rng = np.random.default_rng(0)
    nn_idx = np.zeros((len(pcs), len(pcs)), np.int16)
    for s in range(len(pcs)):
        for t in range(len(SIZES)):
            nn_idx[s, slice_idx[t]:slice_idx[t + 1]] = rng.permutation(SIZES[t])
    attack_idx = np.stack([rng.permutation(4)[:NUM_PC_FOR_ATTACK] for _ in SIZES])
    np.save(ev / "point_clouds_test_set_3l.npy", pcs)
    np.save(ev / "latent_vectors_test_set_3l.npy", ae.transform(pcs))
    np.save(ev / "reconstructions_test_set_3l.npy", ae.get_reconstructions(pcs))
    np.save(ev / "ae_loss_test_set_3l.npy", ae.get_loss_per_pc(pcs))
    np.save(ev / "pc_classes_3l.npy", np.array(CLASSES))
    np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    np.save(ev / "chamfer_nn_idx_complete_test_set_3l.npy", nn_idx)
    np.save(ev / "sel_idx.npy", attack_idx)
    cdir = top / "log" / "pointnet"
    os.makedirs(cdir)
    CW.save_npz(str(cdir / "weights.npz"), CW.synthetic_weights(13, seed=13))

    base = ["--top_dir", str(top), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy"]
    run_attack.main(base + ["--batch_size", "2", "--num_iterations", "12", "--num_iterations_thresh", "8", "--learning_rate",
                            "0.0002", "--num_pc_for_attack", str(NUM_PC_FOR_ATTACK), "--num_pc_for_target", str(NUM_PC_FOR_TARGET),
                            "--dist_weight_list", "0.5", "2.0", "--class_names"] + ATTACKED)
    get_dists_per_point.main(base)                             # (evaluate_attack reads its files)
    evaluate_attack.main(base)
    run_defense_sor.main(base + ["--do_sanity_checks", "1"])
    srs_argv = base + ["--do_sanity_checks", "1", "--drop_num", str(DROP), "--seed", str(SEED)]
    run_defense_srs.main(srs_argv)
    att = ev / "attack_res"
    first = _tree_bytes(att, "defense_srs_res")
    for folder in ("defense_sor_res", "defense_srs_res"):
        evaluate_defense.main(base + ["--output_folder_name", folder])
    run_classifier.main(base + ["--classifier_folder", "log/pointnet", "--num_points", str(N), "--data_type", "after_defense",
                                "--defense_folder", "defense_sor_res"])
    return dict(top=top, ev=ev, att=att, pcs=pcs, slice_idx=slice_idx, nn_idx=nn_idx, attack_idx=attack_idx, ae=ae, base=base,
                srs_argv=srs_argv, srs_first=first)


def _tree_bytes(att, folder):
    """{relative path: bytes} of the class folders of a defense's two output folders, and their configurations."""
    out = {}
    for root in (att / folder, att / (folder + "_orig")):
        for name in ATTACKED:
            for f in sorted(os.listdir(root / name)):
                out[(root.name, name, f)] = (root / name / f).read_bytes()
        out[(root.name, "defense_configuration.json")] = (root / "defense_configuration.json").read_bytes()
    return out


def _prep(r, name, data):
    from geometric_adv_amd.attack_data import prepare_data_for_attack
    return prepare_data_for_attack(np.array(CLASSES), [name], ATTACKED, data, r["slice_idx"], r["attack_idx"], NUM_PC_FOR_TARGET,
                                   r["nn_idx"], None)


def _selected(r, name, base):
    a = np.load(r["att"] / name / (base + ".npy"))
    sel = np.load(r["att"] / name / "analysis_results" / "source_target_norm_min_idx.npy")
    assert sel.shape == (a.shape[1],)
    return a[sel, np.arange(a.shape[1])]


def _load(folder, name, shape, dtype):
    a = np.load(folder / (name + ".npy"))
    assert a.shape == tuple(shape) and a.dtype == dtype, (folder, name, a.shape, a.dtype)
    return a


def _check_scores(r, name, out, out_orig, def_in, def_src_in):
    """defended reconstructions == ae.get_reconstructions(defended input) and the metric columns == get_loss_per_pc and its
    ratio to the source's reference loss, bit for bit."""
    ae = r["ae"]
    src, _ = _prep(r, name, r["pcs"])
    ref = _prep(r, name, np.load(r["ev"] / "ae_loss_test_set_3l.npy"))[0].reshape(-1)
    m = len(src)
    adv = _selected(r, name, "adversarial_pc_input")
    assert np.array_equal(_load(out, "defended_pc_recon", (1, m, N, 3), np.float32)[0], ae.get_reconstructions(def_in))
    assert np.array_equal(_load(out_orig, "defended_source_recon", (m, N, 3), np.float32), ae.get_reconstructions(def_src_in))
    dm = _load(out, "defense_metrics", (1, m, 4), np.float32)[0]
    err, adv_err = ae.get_loss_per_pc(def_in, src), ae.get_loss_per_pc(adv, src)
    assert np.array_equal(dm[:, 0], err) and np.array_equal(dm[:, 1], err / ref)
    assert np.array_equal(dm[:, 2], adv_err) and np.array_equal(dm[:, 3], adv_err / ref)
    sm = _load(out_orig, "defense_source_metrics", (m, 4), np.float32)
    s_err = ae.get_loss_per_pc(def_src_in, src)
    assert np.array_equal(sm[:, 0], s_err) and np.array_equal(sm[:, 1], s_err / ref)
    assert np.array_equal(sm[:, 2], ref) and np.all(sm[:, 3] == 1)


OUT_NAMES = ("adversarial_critical_points", "adversarial_critical_idx", "adversarial_critical_num", "defended_pc_input")
ORIG_NAMES = ("original_source_critical_points", "original_critical_idx", "original_critical_num", "defended_source_input")
OUT_FILES = sorted([n + ".npy" for n in OUT_NAMES] + ["defended_pc_recon.npy", "defense_metrics.npy"])
ORIG_FILES = sorted([n + ".npy" for n in ORIG_NAMES] + ["defended_source_recon.npy", "defense_source_metrics.npy"])


def _source_rows(r, name):
    """The test-set rows of the sources of class `name`, one per attack (source x target)."""
    first = int(r["slice_idx"][CLASSES.index(name)])
    src, _ = _prep(r, name, np.arange(len(r["pcs"]), dtype=np.int64).reshape(-1, 1))
    return src.reshape(-1) - first


def test_sor_defense_files(run):
    import torch
    from geometric_adv_amd import ops
    out_root, orig_root = run["att"] / "defense_sor_res", run["att"] / "defense_sor_res_orig"
    for name in ATTACKED:
        out, out_orig = out_root / name, orig_root / name
        assert sorted(os.listdir(out)) == OUT_FILES and sorted(os.listdir(out_orig)) == ORIG_FILES      # (no kNN files)
        adv = _selected(run, name, "adversarial_pc_input")
        src, _ = _prep(run, name, run["pcs"])
        m = len(src)
        for pc, folder, names in ((adv, out, OUT_NAMES), (src, out_orig, ORIG_NAMES)):
            o_pc, o_idx, o_num, i_pc = [t.cpu().numpy() for t in ops.sor_filter(torch.from_numpy(pc).cuda(), k=NUM_KNN, alpha=ALPHA)]
            w = int(o_num.max())
            lead = (1,) if folder == out else ()
            assert np.array_equal(_load(folder, names[0], lead + (m, w, 3), np.float32).reshape(m, w, 3), o_pc[:, :w])
            assert np.array_equal(_load(folder, names[1], lead + (m, w), np.int16).reshape(m, w), o_idx[:, :w])
            assert np.array_equal(_load(folder, names[2], lead + (m,), np.int16).reshape(m), o_num)
            assert np.array_equal(_load(folder, names[3], lead + (m, N, 3), np.float32).reshape(m, N, 3), i_pc)
        _check_scores(run, name, out, out_orig, np.load(out / "defended_pc_input.npy")[0], np.load(out_orig / "defended_source_input.npy"))
    # the planted points of the clean chair sources are among the removed points
    idx = np.load(orig_root / "chair" / "original_critical_idx.npy")
    num = np.load(orig_root / "chair" / "original_critical_num.npy")
    rows = _source_rows(run, "chair")
    assert len(rows) == len(idx)
    for row, i, c in zip(rows, idx, num):
        assert set(_planted(int(row))) <= set(i[:c].tolist()), (row, i[:c])
    for folder in (out_root, orig_root):
        with open(folder / "defense_configuration.json") as f:
            conf = json.load(f)
        assert conf["num_knn_for_defense"] == NUM_KNN and conf["sor_alpha"] == ALPHA and "knn_dist_thresh" not in conf
        assert conf["class_names"] == ATTACKED and conf["dist_weight_list"] == [0.5, 2.0]


def test_srs_defense_files(run):
    import torch
    from geometric_adv_amd import ops
    out_root, orig_root = run["att"] / "defense_srs_res", run["att"] / "defense_srs_res_orig"
    for name in ATTACKED:
        out, out_orig = out_root / name, orig_root / name
        assert sorted(os.listdir(out)) == OUT_FILES and sorted(os.listdir(out_orig)) == ORIG_FILES
        adv = _selected(run, name, "adversarial_pc_input")
        src, _ = _prep(run, name, run["pcs"])
        m = len(src)
        counter = CLASSES.index(name)                          # the position of the class in pc_classes
        for pc, folder, names, slot in ((adv, out, OUT_NAMES, 0), (src, out_orig, ORIG_NAMES, m)):
            kept, idx = [t.cpu().numpy() for t in ops.random_drop(torch.from_numpy(pc).cuda(), DROP, SEED, counter=counter,
                                                                  slot_offset=slot, return_idx=True)]
            assert np.array_equal(idx, M.srs_dropped(SEED, counter, np.arange(m) + slot, N, DROP))
            lead = (1,) if folder == out else ()
            got_idx = _load(folder, names[1], lead + (m, DROP), np.int16).reshape(m, DROP)
            assert np.array_equal(got_idx, idx)
            want_pts = np.stack([pc[c][idx[c]] for c in range(m)])
            assert np.array_equal(_load(folder, names[0], lead + (m, DROP, 3), np.float32).reshape(m, DROP, 3), want_pts)
            assert (_load(folder, names[2], lead + (m,), np.int16) == DROP).all()
            assert np.array_equal(_load(folder, names[3], lead + (m, N, 3), np.float32).reshape(m, N, 3), kept)
        _check_scores(run, name, out, out_orig, np.load(out / "defended_pc_input.npy")[0], np.load(out_orig / "defended_source_input.npy"))
    for folder in (out_root, orig_root):
        with open(folder / "defense_configuration.json") as f:
            conf = json.load(f)
        assert conf["drop_num"] == DROP and conf["seed"] == SEED and conf["class_names"] == ATTACKED


def test_srs_rerun_writes_the_same_bytes(run):
    import torch
    from geometric_adv_amd import run_defense_srs
    torch.manual_seed(77)                                      # torch's and numpy's generators play no part
    np.random.seed(77)
    run_defense_srs.main(run["srs_argv"])
    again = _tree_bytes(run["att"], "defense_srs_res")
    assert sorted(again) == sorted(run["srs_first"])
    assert all(again[k] == run["srs_first"][k] for k in again)
    with pytest.raises(ValueError, match="drop_num"):
        run_defense_srs.main(run["base"] + ["--drop_num", str(N), "--output_folder_name", "too_many_res"])
    assert not os.path.exists(run["att"] / "too_many_res")


def test_reports_and_classifier_read_the_folders_unchanged(run):
    from geometric_adv_amd import cls_weights as CW
    from geometric_adv_amd.classifier import PointNetClassifier
    att = run["att"]
    for folder in ("defense_sor_res", "defense_srs_res"):
        for t in ("targeted_attacks.txt", "untargeted_attacks.txt", "eval_stats.txt"):
            assert os.path.getsize(att / folder / "over_classes" / t) > 0
    clf = PointNetClassifier(None, num_classes=13, weights=CW.synthetic_weights(13, seed=13))
    for name in ATTACKED:
        recon = np.load(att / "defense_sor_res" / name / "defended_pc_recon.npy")[0]
        got = _load(att / "defense_sor_res" / "classifier_res" / name, "defended_pc_recon_pred", (1, len(recon)), np.int8)
        assert np.array_equal(got[0], clf.classify(recon))
