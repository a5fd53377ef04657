"""GPU: the reporting commands at the end of the pipeline, on files the pipeline itself wrote on a tiny eval folder --
run_attack (two distance weights), get_dists_per_point, evaluate_attack, get_knn_dists_per_point, run_defense_surface,
run_defense_critical, then evaluate_defense for both defenses on adversarial and on source data; run_transfer to a PointNet
with other weights and to a FoldingNet checkpoint, then evaluate_transfer for both.  Every report is rebuilt here from the
.npy files by plain index arithmetic and the reference's format strings, and compared for equality."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
CLASSES, SIZES = ["chair", "table", "car"], [4, 5, 4]
ATTACKED = ["chair", "car"]
NUM_PC_FOR_ATTACK, NUM_PC_FOR_TARGET = 2, 2
RULE = "--------------------------------------\n"
INDEX_FILES = ("source_target_norm_min_idx", "source_target_norm_min_per_target_class_idx",
               "source_target_norm_min_target_all_idx")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """The whole chain, once."""
    from geometric_adv_amd import (evaluate_attack, evaluate_defense, evaluate_transfer, fold_weights as FW, get_dists_per_point,
                                   get_knn_dists_per_point, run_attack, run_defense_critical, run_defense_surface, run_transfer,
                                   weights as W)
    from geometric_adv_amd.autoencoder import PointNetAE
    top = tmp_path_factory.mktemp("report_cli")
    ev = top / "log" / "ae" / "eval"
    os.makedirs(ev)
    slice_idx = np.concatenate([[0], np.cumsum(SIZES)])
    pcs = ((np.random.default_rng(5).random((int(slice_idx[-1]), N, 3)) - 0.5) * 0.06).astype(np.float32)
    for k in range(SIZES[0]):                      # far-off points: outliers for the surface defense to remove
        pcs[k, 7 * k + 3] = np.float32([0.3, 0.3, -0.2])
    w = W.synthetic_weights(N)
    W.save_npz(str(top / "log" / "ae" / "weights.npz"), w)
    ae = PointNetAE(w, N)
    rng = np.random.default_rng(0)
    nn_idx = np.zeros((len(pcs), len(pcs)), np.int16)
    for s in range(len(pcs)):
        for t in range(len(SIZES)):
            nn_idx[s, slice_idx[t]:slice_idx[t + 1]] = rng.permutation(SIZES[t])
    np.save(ev / "point_clouds_test_set_3l.npy", pcs)
    np.save(ev / "latent_vectors_test_set_3l.npy", ae.transform(pcs))
    np.save(ev / "reconstructions_test_set_3l.npy", ae.get_reconstructions(pcs))
    np.save(ev / "ae_loss_test_set_3l.npy", ae.get_loss_per_pc(pcs))
    np.save(ev / "pc_classes_3l.npy", np.array(CLASSES))
    np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    np.save(ev / "chamfer_nn_idx_complete_test_set_3l.npy", nn_idx)
    np.save(ev / "sel_idx.npy", np.stack([rng.permutation(4)[:NUM_PC_FOR_ATTACK] for _ in SIZES]))
    os.makedirs(top / "log" / "ae2")
    W.save_npz(str(top / "log" / "ae2" / "weights.npz"), W.synthetic_weights(N, seed=23))
    FW.save(str(top / "log" / "fold"), 40, FW.initial_weights(3))

    base = ["--top_dir", str(top), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy"]
    run_attack.main(base + ["--batch_size", "2", "--num_iterations", "12", "--num_iterations_thresh", "8", "--learning_rate",
                            "0.0002", "--num_pc_for_attack", str(NUM_PC_FOR_ATTACK), "--num_pc_for_target", str(NUM_PC_FOR_TARGET),
                            "--dist_weight_list", "0.5", "2.0", "--class_names"] + ATTACKED)
    get_dists_per_point.main(base)
    evaluate_attack.main(base)
    get_knn_dists_per_point.main(base + ["--num_knn", "8"])
    run_defense_surface.main(base + ["--num_knn_for_defense", "2", "--knn_dist_thresh", "0.04"])
    run_defense_critical.main(base)
    for folder in ("defense_surface_res", "defense_critical_res"):
        for adv in ("1", "0"):
            evaluate_defense.main(base + ["--output_folder_name", folder, "--use_adversarial_data", adv])
    run_transfer.main(base + ["--transfer_ae_type", "PointNet", "--transfer_ae_folder", "log/ae2"])
    run_transfer.main(base + ["--transfer_ae_type", "FoldingNet", "--transfer_ae_folder", "log/fold",
                              "--transfer_ae_restore_epoch", "40", "--graph_seed", "7"])
    for folder in ("log/ae2", "log/fold"):
        evaluate_transfer.main(base + ["--transfer_ae_folder", folder])
    return dict(top=top, att=ev / "attack_res")


def _line(attack_name, labels, v):
    return "%s%s%s: %.5f   %s: %.2f   %s: %.5f   %s: %.2f\n" % (
        attack_name, " " * (40 - len(attack_name)), labels[0], v[0], labels[1], v[1], labels[2], v[2], labels[3], v[3])


def _expected(att, metrics_of_class, targeted, untargeted, heading):
    """(targeted text, untargeted text, statistics text).  metrics_of_class(name) -> [n_attacks, 4]: this project's metric
    files hold one entry per attack, already at its selected distance weight (leading dimension 1).  targeted / untargeted:
    (which text the lines go to, name prefix, labels)."""
    texts = ["", ""]
    means = {"targeted": [], "untargeted": []}
    per_instance = (len(ATTACKED) - 1) * NUM_PC_FOR_TARGET
    for name in [c for c in CLASSES if c in ATTACKED]:
        weight_idx, per_class_idx, all_idx = [np.load(att / name / "analysis_results" / (b + ".npy")) for b in INDEX_FILES]
        n_weights = len(np.load(att / name / "dist_weight.npy"))
        m = metrics_of_class(name)
        assert m.shape == (NUM_PC_FOR_ATTACK * per_instance, 4) and m.dtype == np.float32
        stacked = np.stack([m] * n_weights)                      # what the commands select from: the same for every weight
        targets = [c for c in ATTACKED if c != name]
        tar = np.zeros((NUM_PC_FOR_ATTACK, len(targets), 4), np.float32)
        untar = np.zeros((NUM_PC_FOR_ATTACK, 4), np.float32)
        texts[0] += "Shape class: %s\n" % name + RULE
        where, prefix, labels = targeted
        for j in range(NUM_PC_FOR_ATTACK):
            for k in range(len(targets)):
                flat = j * per_instance + k * NUM_PC_FOR_TARGET + per_class_idx[j, k]
                tar[j, k] = stacked[weight_idx[flat], flat]
                texts[where] += _line("%s_%s_%d_target_%s_%d" % (prefix, name, j, targets[k], per_class_idx[j, k]), labels, tar[j, k])
        texts[0] += "\n"
        texts[1] += "Shape class: %s\n" % name + RULE
        where, prefix, labels = untargeted
        for j in range(NUM_PC_FOR_ATTACK):
            k = all_idx[j]
            flat = j * per_instance + k * NUM_PC_FOR_TARGET + per_class_idx[j, k]
            untar[j] = stacked[weight_idx[flat], flat]
            texts[where] += _line("%s_%s_%d_target_%s_%d" % (prefix, name, j, targets[k], per_class_idx[j, k]), labels, untar[j])
        texts[1] += "\n"
        means["targeted"].append(tar)
        means["untargeted"].append(untar)
    stats = ""
    row = "%s%s%.5f\t\t%.2f\t\t%.5f\t\t%.2f\n"
    for kind in ("targeted", "untargeted"):
        stats += ("\n" if stats else "") + "Statistics for %s attack\n" % kind + RULE + heading[0] + heading[1] + "\n"
        for c, name in enumerate(ATTACKED):
            stats += row % ((name, " " * (16 - len(name))) + tuple(np.ascontiguousarray(means[kind][c][..., col]).mean() for col in range(4)))
        stats += "\n"
        stats += row % (("over classes", " " * 4) + tuple(np.vstack([a[..., col] for a in means[kind]]).mean() for col in range(4)))
    return texts[0], texts[1], stats


def _read(folder):
    assert sorted(os.listdir(folder)) == ["eval_stats.txt", "targeted_attacks.txt", "untargeted_attacks.txt"]
    out = []
    for t in ("targeted_attacks.txt", "untargeted_attacks.txt", "eval_stats.txt"):
        with open(folder / t) as f:
            out.append(f.read())
    return tuple(out)


DEF_HEADING = ("Shape\t\tDef\t\tDef\t\tAdv\t\tAdv\n", "Class\t\tS-RE\t\tS-NRE\t\tS-RE\t\tS-NRE\n")
TRA_HEADING = ("Shape\t\tTra\t\tTra\t\tAdv\t\tAdv\n", "Class\t\tT-RE\t\tT-NRE\t\tT-RE\t\tT-NRE\n")
T_LABELS = ("tra T-RE", "tra T-NRE", "adv T-RE", "adv T-NRE")


@pytest.mark.parametrize("folder", ["defense_surface_res", "defense_critical_res"])
@pytest.mark.parametrize("adv", [1, 0])
def test_evaluate_defense_reports(run, folder, adv):
    att = run["att"]
    out = att / (folder + ("" if adv else "_orig"))

    def metrics(name):
        if adv:
            m = np.load(out / name / "defense_metrics.npy")
            assert m.shape[0] == 1
            return m[0]
        return np.load(out / name / "defense_source_metrics.npy")

    want = _expected(att, metrics, (1, "def", T_LABELS), (1, "def", ("def S-RE", "def S-NRE", "adv S-RE", "adv S-NRE")), DEF_HEADING)
    got = _read(out / "over_classes")
    assert got == want
    assert got[0] == "".join("Shape class: %s\n%s\n" % (c, RULE) for c in ATTACKED)       # the reference's quirk: headers only
    if not adv:                                                                          # the clean source's S-NRE is 1
        assert all(l.endswith("adv S-NRE: 1.00") for l in got[1].splitlines() if "def S-RE" in l)


@pytest.mark.parametrize("folder", ["log/ae2", "log/fold"])
def test_evaluate_transfer_reports(run, folder):
    out = run["top"] / folder / "eval" / "attack_res_transfer"

    def metrics(name):
        m = np.load(out / name / "transfer_metrics.npy")
        assert m.shape[0] == 1
        return m[0]

    want = _expected(run["att"], metrics, (0, "def", ("tra T-RE", "def S-NRE", "adv S-RE", "adv S-NRE")), (1, "tra", T_LABELS),
                     TRA_HEADING)
    got = _read(out / "over_classes")
    assert got == want
    assert len([l for l in got[0].splitlines() if l.startswith("def_")]) == len(ATTACKED) * NUM_PC_FOR_ATTACK
    assert len([l for l in got[1].splitlines() if l.startswith("tra_")]) == len(ATTACKED) * NUM_PC_FOR_ATTACK


def test_reports_differ_between_the_auto_encoders(run):
    """The two transfer tables share the attack's columns and differ in the transferred ones."""
    a, b = [_read(run["top"] / f / "eval" / "attack_res_transfer" / "over_classes")[2] for f in ("log/ae2", "log/fold")]
    assert a != b
