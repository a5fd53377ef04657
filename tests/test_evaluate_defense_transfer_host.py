"""CPU: geometric_adv_amd.evaluate_defense and evaluate_transfer against tests/golden/evaluate_defense_transfer.npz, which
tools/make_golden_evaluate_defense_transfer.py made by running the reference's own defender/evaluate_defense.py and
transfer/evaluate_transfer.py on the same synthetic tree: every written text byte for byte (the reference's line-label quirks
included), the file names of every run, the minimal set of files read and the refusals."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_evaluate_defense_transfer as G  # noqa: E402

A = G.A
BASE = ["--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy"]


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "evaluate_defense_transfer.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tree(tmp_path_factory, golden):
    """The whole tree from the golden's arrays, with only the files listed under "Reads" (no clouds, neighbour indices,
    sel_idx, critical points, defended clouds or transferred_pc_recon), and this project's evaluate_attack run on it."""
    from geometric_adv_amd import evaluate_attack
    top = str(tmp_path_factory.mktemp("defense_transfer"))
    conf = json.loads(str(golden["conf_json"]))
    per_class = {c: (golden["adversarial_metrics__" + c], golden["adversarial_pc_input_dists__" + c]) for c in conf["class_names"]}
    att = A.write_attack_folder(top, conf, per_class)
    evaluate_attack.main(["--top_dir", top] + BASE)
    for folder in G.DEFENSE_FOLDERS:
        G.write_defense_folder(att, folder, json.loads(str(golden["defense_conf_json__" + folder])),
                               {c: (golden["defense_metrics__%s__%s" % (folder, c)],
                                    golden["defense_source_metrics__%s__%s" % (folder, c)]) for c in conf["class_names"]})
    for folder in G.TRANSFER_FOLDERS:
        G.write_transfer_folder(top, folder, {c: golden["transfer_metrics__%s__%s" % (folder, c)] for c in conf["class_names"]})
    return dict(top=top, att=att, conf=conf)


def _defense(top, folder, adv, params, *extra):
    from geometric_adv_amd import evaluate_defense
    evaluate_defense.main(["--top_dir", str(top)] + G.defense_argv(folder, adv, params) + list(extra))


def _transfer(top, folder, *extra):
    from geometric_adv_amd import evaluate_transfer
    evaluate_transfer.main(["--top_dir", str(top)] + G.transfer_argv(folder) + list(extra))


def _check_texts(over_classes, golden, run, want_names):
    assert sorted(os.listdir(over_classes)) == want_names, run
    assert sorted(k.split("__")[-1] for k in golden if k.startswith("text__%s__" % run)) == want_names, run
    for t in want_names:
        with open(os.path.join(over_classes, t)) as f:
            assert f.read() == str(golden["text__%s__%s" % (run, t)]), (run, t)


def test_fixture_inputs_are_the_tools(golden):
    """The fixture's inputs are what the tool draws, so a regenerated fixture covers the same ground: both leading
    dimensions, metrics that differ between distance weights, the surface defense's settings in one configuration only."""
    conf, per_class = A.synthetic_inputs()
    defense, transfer = G.synthetic_metrics()
    assert json.loads(str(golden["conf_json"])) == conf and list(golden["pc_classes"]) == A.PC_CLASSES
    assert len(A.PC_CLASSES) == 4 and len(conf["class_names"]) == 3 and len(conf["dist_weight_list"]) == 3
    for c, (m, d) in per_class.items():
        assert np.array_equal(golden["adversarial_metrics__" + c], m)
        assert np.array_equal(golden["adversarial_pc_input_dists__" + c], d)
    leads = set()
    for folder, (lead, surface) in G.DEFENSE_FOLDERS.items():
        def_conf = json.loads(str(golden["defense_conf_json__" + folder]))
        assert def_conf == G.defense_conf(conf, surface) and ("knn_dist_thresh" in def_conf) == surface
        for c, (m, s) in defense[folder].items():
            assert m.shape == (lead, G.n_attacks(), 4) and s.shape == (G.n_attacks(), 4) and m.dtype == s.dtype == np.float32
            assert np.array_equal(golden["defense_metrics__%s__%s" % (folder, c)], m)
            assert np.array_equal(golden["defense_source_metrics__%s__%s" % (folder, c)], s)
            assert lead == 1 or not np.any(m[0] == m[1])
        leads.add((lead, surface))
    assert leads == {(1, True), (3, True), (1, False)}
    for folder, lead in G.TRANSFER_FOLDERS.items():
        for c, m in transfer[folder].items():
            assert m.shape == (lead, G.n_attacks(), 4) and m.dtype == np.float32
            assert np.array_equal(golden["transfer_metrics__%s__%s" % (folder, c)], m)
    assert sorted(G.TRANSFER_FOLDERS.values()) == [1, 3]
    texts = [k for k in golden if k.startswith("text__")]
    assert len(texts) == 3 * (len(G.defense_runs()) + len(G.TRANSFER_FOLDERS))


@pytest.mark.parametrize("folder,adv,params", G.defense_runs())
def test_defense_matches_reference_run(tree, golden, folder, adv, params):
    out = os.path.join(tree["att"], folder + ("" if adv else "_orig"))
    shutil.rmtree(os.path.join(out, "over_classes"), ignore_errors=True)
    _defense(tree["top"], folder, adv, params, "--do_sanity_checks", "1")
    want = G.defense_text_names(folder, params)
    surface = G.DEFENSE_FOLDERS[folder][1]
    assert all(("_k_2_th_0.04" in t) == bool(params and surface) for t in want)
    _check_texts(os.path.join(out, "over_classes"), golden, G.defense_run_key(folder, adv, params), want)
    # the unattacked class leaves no trace, and nothing but over_classes/ is added
    assert sorted(os.listdir(out)) == sorted(tree["conf"]["class_names"] + ["defense_configuration.json", "over_classes"])
    assert not os.path.exists(os.path.join(tree["att"], "lamp"))


def test_defense_quirks_are_the_references(golden):
    """targeted_attacks.txt holds the class headers only; the per-target-class lines sit in the untargeted file, before
    the class's header, with the T- labels."""
    run = G.defense_run_key("defense_surface_res", 1, 0)
    tar = str(golden["text__%s__targeted_attacks.txt" % run]).splitlines()
    assert [l for l in tar if l and not l.startswith("-")] == ["Shape class: %s" % c for c in A.CLASS_NAMES]
    untar = str(golden["text__%s__untargeted_attacks.txt" % run]).splitlines()
    per_class = A.NUM_PC_FOR_ATTACK * (len(A.CLASS_NAMES) - 1)
    assert all("tra T-RE: " in l and "adv T-NRE: " in l for l in untar[:per_class])
    assert untar[per_class] == "Shape class: chair"
    assert all("def S-RE: " in l for l in untar[per_class + 2:per_class + 2 + A.NUM_PC_FOR_ATTACK])


@pytest.mark.parametrize("folder", list(G.TRANSFER_FOLDERS))
def test_transfer_matches_reference_run(tree, golden, folder):
    out = os.path.join(tree["top"], G.TRANSFER_AE_FOLDER, "eval", folder)
    shutil.rmtree(os.path.join(out, "over_classes"), ignore_errors=True)
    _transfer(tree["top"], folder)
    _check_texts(os.path.join(out, "over_classes"), golden, folder, G.transfer_text_names())
    assert sorted(os.listdir(out)) == sorted(tree["conf"]["class_names"] + ["over_classes"])
    tar = str(golden["text__%s__targeted_attacks.txt" % folder]).splitlines()
    assert tar[2].startswith("def_chair_0_target_table_") and "tra T-RE: " in tar[2] and "def S-NRE: " in tar[2]
    untar = str(golden["text__%s__untargeted_attacks.txt" % folder]).splitlines()
    assert untar[2].startswith("tra_chair_0_target_") and "tra T-NRE: " in untar[2]


def _copy(tree, tmp_path):
    top = str(tmp_path / "copy")
    shutil.copytree(tree["top"], top)
    for root, dirs, _ in os.walk(top):             # the reports earlier tests left in the shared tree
        if "over_classes" in dirs:
            shutil.rmtree(os.path.join(root, "over_classes"))
            dirs.remove("over_classes")
    return top, os.path.join(top, "log", "ae", "eval", "attack_res")


@pytest.mark.parametrize("flag", ["--save_graphs", "--save_pc_plots"])
def test_plot_flags_are_refused(tree, tmp_path, flag):
    top, att = _copy(tree, tmp_path)
    with pytest.raises(SystemExit, match="matplotlib"):
        _defense(top, "defense_surface_res", 1, 0, flag, "1")
    with pytest.raises(SystemExit, match="matplotlib"):
        _transfer(top, "attack_res_transfer", flag, "1")
    assert not os.path.exists(os.path.join(att, "defense_surface_res", "over_classes"))
    assert not os.path.exists(os.path.join(top, G.TRANSFER_AE_FOLDER, "eval", "attack_res_transfer", "over_classes"))


def test_missing_folders_are_refused(tree, tmp_path):
    top, att = _copy(tree, tmp_path)
    for adv in (1, 0):
        with pytest.raises(SystemExit, match="run_defense_surface.*run_defense_critical"):
            _defense(top, "no_such_defense_res", adv, 0)
    os.remove(os.path.join(att, "defense_critical_res", "defense_configuration.json"))
    with pytest.raises(SystemExit, match="run_defense_surface.*run_defense_critical"):
        _defense(top, "defense_critical_res", 1, 0)
    with pytest.raises(SystemExit, match="run_transfer"):
        _transfer(top, "no_such_transfer")
    assert not os.path.exists(os.path.join(att, "no_such_defense_res"))
    assert not os.path.exists(os.path.join(att, "no_such_defense_res_orig"))
    assert not os.path.exists(os.path.join(att, "defense_critical_res", "over_classes"))
    assert not os.path.exists(os.path.join(top, G.TRANSFER_AE_FOLDER, "eval", "no_such_transfer"))


def test_missing_analysis_results_is_refused(tree, tmp_path):
    top, att = _copy(tree, tmp_path)
    shutil.rmtree(os.path.join(att, "table", "analysis_results"))
    with pytest.raises(SystemExit, match="evaluate_attack"):
        _defense(top, "defense_surface_res", 1, 0)
    with pytest.raises(SystemExit, match="evaluate_attack"):
        _transfer(top, "attack_res_transfer")
    assert not os.path.exists(os.path.join(att, "defense_surface_res", "over_classes"))
    assert not os.path.exists(os.path.join(top, G.TRANSFER_AE_FOLDER, "eval", "attack_res_transfer", "over_classes"))
