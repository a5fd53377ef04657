"""GPU: the defense stage's commands end to end on a tiny eval folder -- run_attack (two distance weights), get_dists_per_point,
evaluate_attack, get_knn_dists_per_point, run_defense_surface and run_defense_critical with the reference's sanity checks, and
run_classifier for source / before_defense / after_defense -- every written file checked by name, dtype, shape and value
against the library calls and the numpy restatement of the packing (oracle/host_defense.py), and the refusals."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
CLASSES, SIZES = ["chair", "table", "car"], [4, 5, 4]
ATTACKED = ["chair", "car"]
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 2, 2
THRESH, TOP_K, NUM_KNN = 0.04, 2, 8


def _test_set():
    """Clouds 0.06 wide (every point's mean distance to its 2 nearest neighbours stays far below 0.04); chair cloud k gets
    k + 1 far-off points 0.1 apart (outliers of the surface defense), car clouds none."""
    slice_idx = np.concatenate([[0], np.cumsum(SIZES)])
    pcs = ((np.random.default_rng(5).random((int(slice_idx[-1]), N, 3)) - 0.5) * 0.06).astype(np.float32)
    for k in range(SIZES[0]):
        for j in range(k + 1):
            pcs[k, 7 * j + 3] = np.float32([0.3 + 0.1 * j, 0.3, -0.2])
    return pcs, slice_idx


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The whole chain on one folder, with the refusals checked at the point where they apply."""
    from geometric_adv_amd import (cls_weights as CW, evaluate_attack, get_dists_per_point, get_knn_dists_per_point,
                                   run_attack, run_defense_critical, run_defense_surface, weights as W)
    from geometric_adv_amd.autoencoder import PointNetAE
    top = tmp_path_factory.mktemp("defense_cli")
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
    get_dists_per_point.main(base + ["--do_sanity_checks", "1"])
    with pytest.raises(FileNotFoundError, match="source_target_norm_min_idx"):         # two weights and no selection yet
        get_knn_dists_per_point.main(base)
    evaluate_attack.main(base)
    with pytest.raises(FileNotFoundError, match="get_knn_dists_per_point"):
        run_defense_surface.main(base + ["--output_folder_name", "no_knn_res"])
    get_knn_dists_per_point.main(base + ["--num_knn", str(NUM_KNN)])
    run_defense_surface.main(base + ["--do_sanity_checks", "1", "--num_knn_for_defense", str(TOP_K),
                                     "--knn_dist_thresh", str(THRESH)])
    run_defense_critical.main(base + ["--do_sanity_checks", "1"])
    return dict(top=top, ev=ev, att=ev / "attack_res", pcs=pcs, slice_idx=slice_idx, nn_idx=nn_idx, attack_idx=attack_idx, ae=ae,
                base=base)


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


def _source_loss(r, name):
    loss = np.load(r["ev"] / "ae_loss_test_set_3l.npy")
    return _prep(r, name, loss)[0].reshape(-1)


def _check_scores(r, name, out, out_orig, def_in, def_src_in):
    """defended reconstructions == ae.get_reconstructions(defended input) and the metric columns == get_loss_per_pc and its
    ratio to the source's reference loss, bit for bit."""
    ae = r["ae"]
    src, _ = _prep(r, name, r["pcs"])
    ref = _source_loss(r, name)
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


OUT_FILES = sorted(["adversarial_critical_points.npy", "adversarial_critical_idx.npy", "adversarial_critical_num.npy",
                    "defended_pc_input.npy", "defended_pc_recon.npy", "defense_metrics.npy"])
ORIG_FILES = sorted(["original_source_critical_points.npy", "original_critical_idx.npy", "original_critical_num.npy",
                     "defended_source_input.npy", "defended_source_recon.npy", "defense_source_metrics.npy"])


def test_evaluate_attack_selection(run):
    for name in ATTACKED:
        m = np.load(run["att"] / name / "adversarial_metrics.npy")
        sel = np.load(run["att"] / name / "analysis_results" / "source_target_norm_min_idx.npy")
        assert sel.dtype == np.int64 and np.array_equal(sel, np.argmin(m[:, :, 2] + m[:, :, 4], axis=0))
    for t in ("targeted_attacks.txt", "untargeted_attacks.txt", "eval_stats.txt"):
        assert os.path.getsize(run["att"] / "over_classes" / t) > 0


def test_knn_dists_files(run):
    import torch
    from geometric_adv_amd import ops
    for name in ATTACKED:
        adv = _selected(run, name, "adversarial_pc_input")
        src, _ = _prep(run, name, run["pcs"])
        m = len(src)
        got = _load(run["att"] / "defense_surface_res" / name, "knn_dists_adversarial_pc_input", (1, m, N, NUM_KNN), np.float32)
        assert np.array_equal(got[0], ops.knn_dists(torch.from_numpy(adv).cuda(), NUM_KNN).cpu().numpy())
        got = _load(run["att"] / "defense_surface_res_orig" / name, "knn_dists_source_pc", (m, N, NUM_KNN), np.float32)
        assert np.array_equal(got, ops.knn_dists(torch.from_numpy(src).cuda(), NUM_KNN).cpu().numpy())


def test_surface_defense_files(run):
    from oracle.host_defense import outlier_inlier
    out_root, orig_root = run["att"] / "defense_surface_res", run["att"] / "defense_surface_res_orig"
    widths = {}
    for name in ATTACKED:
        out, out_orig = out_root / name, orig_root / name
        assert sorted(os.listdir(out)) == sorted(OUT_FILES + ["knn_dists_adversarial_pc_input.npy"])
        assert sorted(os.listdir(out_orig)) == sorted(ORIG_FILES + ["knn_dists_source_pc.npy"])
        adv = _selected(run, name, "adversarial_pc_input")
        src, _ = _prep(run, name, run["pcs"])
        m = len(src)
        for pc, knn, folder, names in (
                (adv, np.load(out / "knn_dists_adversarial_pc_input.npy")[0], out,
                 ("adversarial_critical_points", "adversarial_critical_idx", "adversarial_critical_num", "defended_pc_input")),
                (src, np.load(out_orig / "knn_dists_source_pc.npy"), out_orig,
                 ("original_source_critical_points", "original_critical_idx", "original_critical_num", "defended_source_input"))):
            o_pc, o_idx, o_num, i_pc = outlier_inlier(pc, np.mean(knn[:, :, :TOP_K], axis=-1), np.float32(THRESH))
            w = int(o_num.max())
            lead = (1,) if folder == out else ()
            assert np.array_equal(_load(folder, names[0], lead + (m, w, 3), np.float32).reshape(m, w, 3), o_pc[:, :w])
            assert np.array_equal(_load(folder, names[1], lead + (m, w), np.int16).reshape(m, w), o_idx[:, :w])
            assert np.array_equal(_load(folder, names[2], lead + (m,), np.int16).reshape(m), o_num)
            assert np.array_equal(_load(folder, names[3], lead + (m, N, 3), np.float32).reshape(m, N, 3), i_pc)
            widths[(name, folder == out)] = w
        _check_scores(run, name, out, out_orig, np.load(out / "defended_pc_input.npy")[0],
                      np.load(out_orig / "defended_source_input.npy"))
    # the planted points: chair clouds lose up to 4 (both halves), car clouds none -- a width-0 trim
    assert widths[("chair", True)] >= 1 and widths[("chair", False)] >= 1
    assert widths[("car", True)] == 0 and widths[("car", False)] == 0
    for folder in (out_root, orig_root):
        with open(folder / "defense_configuration.json") as f:
            conf = json.load(f)
        assert conf["num_knn_for_defense"] == TOP_K and conf["knn_dist_thresh"] == THRESH
        assert conf["class_names"] == ATTACKED and conf["dist_weight_list"] == [0.5, 2.0]


def test_critical_defense_files(run):
    from oracle.host_defense import critical_and_rest, same_critical_sets
    ae = run["ae"]
    out_root, orig_root = run["att"] / "defense_critical_res", run["att"] / "defense_critical_res_orig"
    bneck = ae.bneck
    for name in ATTACKED:
        out, out_orig = out_root / name, orig_root / name
        assert sorted(os.listdir(out)) == OUT_FILES and sorted(os.listdir(out_orig)) == ORIG_FILES
        adv = _selected(run, name, "adversarial_pc_input")
        src, _ = _prep(run, name, run["pcs"])
        m = len(src)
        for pc, folder, names in (
                (adv, out, ("adversarial_critical_points", "adversarial_critical_idx", "adversarial_critical_num", "defended_pc_input")),
                (src, out_orig, ("original_source_critical_points", "original_critical_idx", "original_critical_num",
                                 "defended_source_input"))):
            mv, mi = [t.cpu().numpy() for t in ae.max_and_argmax(pc)]
            pts_w, idx_w, num_w, _, rest_w = critical_and_rest(pc, mv, mi)
            lead = (1,) if folder == out else ()
            pts = _load(folder, names[0], lead + (m, bneck, 3), np.float32).reshape(m, bneck, 3)
            idx = _load(folder, names[1], lead + (m, bneck), np.int16).reshape(m, bneck)
            num = _load(folder, names[2], lead + (m,), np.int16).reshape(m)
            assert same_critical_sets(idx, num, idx_w, num_w, mv, mi)
            for k in range(m):
                assert np.array_equal(pts[k, :num[k]], pc[k][idx[k, :num[k]].astype(np.int64)])
                assert not idx[k, num[k]:].any() and not pts[k, num[k]:].any()
            assert np.array_equal(_load(folder, names[3], lead + (m, N, 3), np.float32).reshape(m, N, 3), rest_w)
        _check_scores(run, name, out, out_orig, np.load(out / "defended_pc_input.npy")[0],
                      np.load(out_orig / "defended_source_input.npy"))
    for folder in (out_root, orig_root):
        with open(folder / "defense_configuration.json") as f:
            conf = json.load(f)
        assert conf["class_names"] == ATTACKED and "knn_dist_thresh" not in conf


def test_run_classifier_defense_types(run):
    from geometric_adv_amd import run_classifier
    from geometric_adv_amd.classifier import PointNetClassifier
    from geometric_adv_amd import cls_weights as CW
    clf = PointNetClassifier(None, num_classes=13, weights=CW.synthetic_weights(13, seed=13))
    att = run["att"]
    base = run["base"] + ["--classifier_folder", "log/pointnet", "--num_points", str(N)]
    rec = np.load(run["ev"] / "reconstructions_test_set_3l.npy")
    run_classifier.main(base + ["--data_type", "source", "--defense_folder", "defense_surface_res"])
    run_classifier.main(base + ["--data_type", "before_defense", "--defense_folder", "defense_critical_res"])
    for d in ("defense_surface_res", "defense_critical_res", "defense_surface_res_orig"):
        run_classifier.main(base + ["--data_type", "after_defense", "--defense_folder", d])
    for name in ATTACKED:
        src_rec, _ = _prep(run, name, rec)
        m = len(src_rec)
        got = _load(att / "defense_surface_res" / "classifier_res_orig" / name, "source_pc_recon_pred", (1, m), np.int8)
        assert np.array_equal(got[0], clf.classify(src_rec))
        got = _load(att / "defense_critical_res" / "classifier_res" / name, "adversarial_pc_recon_pred", (1, m), np.int8)
        assert np.array_equal(got[0], clf.classify(_selected(run, name, "adversarial_pc_recon")))
        for d in ("defense_surface_res", "defense_critical_res"):
            got = _load(att / d / "classifier_res" / name, "defended_pc_recon_pred", (1, m), np.int8)
            assert np.array_equal(got[0], clf.classify(np.load(att / d / name / "defended_pc_recon.npy")[0]))
        got = _load(att / "defense_surface_res_orig" / "classifier_res" / name, "defended_source_recon_pred", (m,), np.int8)
        assert np.array_equal(got, clf.classify(np.load(att / "defense_surface_res_orig" / name / "defended_source_recon.npy")))
    for folder in (att / "defense_surface_res" / "classifier_res_orig", att / "defense_critical_res" / "classifier_res"):
        assert os.path.exists(folder / "classifier_configuration.json")
    for data_type in ("source", "before_defense", "after_defense"):
        with pytest.raises(SystemExit, match="run_defense_surface"):
            run_classifier.main(base + ["--data_type", data_type, "--defense_folder", "no_such_defense_res"])
    assert not os.path.exists(att / "no_such_defense_res")
