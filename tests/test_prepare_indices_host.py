"""CPU: the host side of prepare_indices_for_attack's --get_rand_idx and --get_latent_nn_idx stages against what the reference's
own script wrote (tests/golden/prepare_indices.npz, tools/make_golden_prepare_indices.py): scorer.latent_dist_mat_host bit for
bit at several row blocks, and the command with --device cpu by file name, dtype and content."""
import os
import os.path as osp
import subprocess
import sys

import numpy as np
import pytest

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
GOLDEN = osp.join(ROOT, "tests", "golden")
OUT_NAMES = {"sel_idx_rand": "sel_idx_rand_6_test_set_4l.npy", "latent_dist_mat": "latent_dist_mat_test_set_4l.npy",
             "latent_nn_idx": "latent_nn_idx_test_set_4l.npy"}


@pytest.fixture(scope="module")
def golden():
    return np.load(osp.join(GOLDEN, "prepare_indices.npz"))


def _eval_folder(top, golden):
    ev = top / "log" / "ae" / "eval"
    os.makedirs(ev)
    np.save(ev / "pc_classes_4l.npy", golden["pc_classes"])
    np.save(ev / "slice_idx_test_set_4l.npy", golden["slice_idx"])
    np.save(ev / "latent_vectors_test_set_4l.npy", golden["latent_vectors"])
    return ev


def test_the_golden_is_what_the_issue_describes(golden):
    assert golden["latent_vectors"].shape == (40, 128) and golden["latent_vectors"].dtype == np.float32
    assert np.diff(golden["slice_idx"]).tolist() == [5, 17, 4, 14] and int(golden["num_instance_per_class"]) == 6
    assert golden["latent_dist_mat"].dtype == np.float32 and golden["latent_nn_idx"].dtype == np.int16


@pytest.mark.parametrize("row_block", [1, 7, 64])
def test_latent_dist_mat_host_is_bit_equal_to_the_reference(golden, row_block):
    from geometric_adv_amd.scorer import latent_dist_mat_host
    got = latent_dist_mat_host(golden["latent_vectors"], row_block=row_block)
    assert got.dtype == np.float32 and got.shape == (40, 40)
    assert np.array_equal(got, golden["latent_dist_mat"])
    assert np.array_equal(got.view(np.uint32), golden["latent_dist_mat"].view(np.uint32))


def test_cli_on_the_cpu_writes_the_reference_files(tmp_path, golden):
    from geometric_adv_amd import prepare_indices_for_attack
    ev = _eval_folder(tmp_path, golden)
    before = set(os.listdir(ev))
    prepare_indices_for_attack.main(["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--device", "cpu", "--get_rand_idx", "1",
                                     "--get_latent_nn_idx", "1", "--num_instance_per_class", "6"])
    assert set(os.listdir(ev)) - before == set(OUT_NAMES.values())
    got = {k: np.load(ev / name) for k, name in OUT_NAMES.items()}
    assert (got["sel_idx_rand"].dtype, got["latent_dist_mat"].dtype, got["latent_nn_idx"].dtype) == (np.int16, np.float32, np.int16)
    for k in OUT_NAMES:
        assert got[k].shape == golden[k].shape and np.array_equal(got[k], golden[k]), k
    sel = got["sel_idx_rand"]
    assert sel.shape == (4, 6)
    assert np.array_equal(sel[0, 5:], [-1]) and np.array_equal(sel[2, 4:], [-1, -1])      # the classes of 5 and 4 instances
    assert sorted(sel[0, :5]) == list(range(5)) and sorted(sel[2, :4]) == list(range(4))
    assert (sel[1] >= 0).all() and (sel[3] >= 0).all() and len(set(sel[1])) == 6 and sel[1].max() < 17 and sel[3].max() < 14


def test_a_call_without_a_stage_flag_writes_nothing(tmp_path, golden):
    from geometric_adv_amd import prepare_indices_for_attack
    ev = _eval_folder(tmp_path, golden)
    before = set(os.listdir(ev))
    prepare_indices_for_attack.main(["--top_dir", str(tmp_path), "--ae_folder", "log/ae"])
    assert set(os.listdir(ev)) == before


def test_rand_idx_alone_writes_one_file_and_does_not_import_torch(tmp_path, golden):
    ev = _eval_folder(tmp_path, golden)
    before = set(os.listdir(ev))
    code = ("import sys\n"
            "from geometric_adv_amd import prepare_indices_for_attack as p\n"
            "p.main(['--top_dir', sys.argv[1], '--ae_folder', 'log/ae', '--get_rand_idx', '1'])\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n")
    res = subprocess.run([sys.executable, "-c", code, str(tmp_path)], cwd=ROOT, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert set(os.listdir(ev)) - before == {"sel_idx_rand_100_test_set_4l.npy"}
    sel = np.load(ev / "sel_idx_rand_100_test_set_4l.npy")
    assert sel.dtype == np.int16 and sel.shape == (4, 100)
    assert (sel >= 0).sum(axis=1).tolist() == [5, 17, 4, 14]
    assert np.array_equal(sel[:, :4], golden["sel_idx_rand"][:, :4])        # the shuffle does not depend on the number asked for
