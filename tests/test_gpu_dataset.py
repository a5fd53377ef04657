"""GPU: the dataset stage on the device -- ops.sort_axes (csrc/dataset.hip) bit for bit against the reference's recorded outputs
(tests/golden/dataset.npz) and against a numpy restatement at the kernel's edge shapes, PointNetAE.evaluate against the three
calls it replaces, and the two commands end to end on the golden PLY tree: tst_ae writes the eval folder run_attack's loader
reads, train_ae --data_dir trains from the PLY folder and tst_ae evaluates what it wrote."""
import os
import os.path as osp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
TREE = osp.join(GOLDEN, "dataset")
CLASSES = ["table", "car"]
N = 64
DEV = "cuda:0"


@pytest.fixture(scope="module")
def golden():
    return np.load(osp.join(GOLDEN, "dataset.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("neg_rot", [False, True])
def test_sort_axes_is_bit_equal_to_the_golden(golden, neg_rot):
    from geometric_adv_amd import ops
    out, idx = ops.sort_axes(torch.from_numpy(golden["sa_in"]).to(DEV), neg_rot=neg_rot)
    assert out.dtype == torch.float32 and idx.dtype == torch.int32 and tuple(idx.shape) == (64, 3)
    assert np.array_equal(idx.cpu().numpy(), golden["sa_idx"])
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(golden["sa_out_neg%d" % int(neg_rot)]))
    assert list(golden["sa_idx"][2]) == [1, 0, 2]                  # equal x and y extents: the reference swaps
    assert golden["sa_ref_accepts"].sum() == 61                    # all but the three clouds with an x or y extent of exactly 0


def sort_axes_numpy(pc, neg_rot):
    """shift_rotate_util.py:22-62 over the whole batch at once.  Where the reference's argsort would move z (an x or y extent of
    exactly 0: its assertion fails there), z stays and the same x / y rule holds."""
    ext = pc.max(axis=1) - pc.min(axis=1)
    ext[:, 2] = 0.
    idx = np.argsort(ext, axis=1)[:, ::-1].copy()
    bad = idx[:, 2] != 2
    idx[bad] = np.where((ext[bad, 0] <= ext[bad, 1])[:, None], [1, 0, 2], [0, 1, 2])
    out = np.take_along_axis(pc, idx[:, None, :], axis=2)
    flip = ext[:, 0] < ext[:, 1]
    out[flip, :, int(neg_rot)] = -out[flip, :, int(neg_rot)]
    return out, idx


def _clouds(b, n, seed):
    """Cloud k is of kind (k + n) % 5: 0 x longer, 1 equal x and y extents, 2 z longest, 3 one repeated point, 4 y longer at
    negative coordinates; the boxes' corners are attained exactly where n >= 2."""
    rng = np.random.default_rng(seed)
    lo = rng.integers(-8, 0, (b, 3)) / np.float32(8)
    size = rng.integers(1, 9, (b, 3)) / np.float32(8)
    kind = (np.arange(b) + n) % 5
    size[kind == 0, 0] = size[kind == 0, 1] + 0.125
    size[kind == 1, 1] = size[kind == 1, 0]
    size[kind == 2, 2] = 2.0
    size[kind == 3] = 0.0
    size[kind == 4, 1] = size[kind == 4, 0] + 0.25
    lo[kind == 4] -= 2.0
    pc = (lo[:, None, :] + rng.random((b, n, 3), dtype=np.float32) * size[:, None, :]).astype(np.float32)
    if n >= 2:
        pc[:, 0], pc[:, n - 1] = lo, lo + size
    return pc


@pytest.mark.parametrize("b, n", [(b, n) for n in (1, 63, 64, 65, 257, 2048) for b in (1, 3)] + [(70000, 4)])
def test_sort_axes_is_bit_equal_to_numpy_at_edge_shapes(b, n):
    """One point, the wave's width and its neighbours, more than one pass of the 256 threads, the full-size cloud; and more
    clouds than the grid has workgroups (65 535).  The input lies in a NaN-filled buffer at an odd offset: a read outside the
    clouds would turn an extent into NaN and change the order."""
    from geometric_adv_amd import ops
    pc = _clouds(b, n, seed=b + n)
    pad = 5
    buf = torch.full((pad + pc.size + pad,), float("nan"), dtype=torch.float32, device=DEV)
    buf[pad:pad + pc.size] = torch.from_numpy(pc).reshape(-1).to(DEV)
    x = buf[pad:pad + pc.size].view(b, n, 3)
    for neg_rot in (True, False):
        want, want_idx = sort_axes_numpy(pc, neg_rot)
        out, idx = ops.sort_axes(x, neg_rot=neg_rot)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    if b == 70000:
        assert {tuple(r) for r in want_idx} == {(0, 1, 2), (1, 0, 2)}
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(pc))           # the input is left alone


def test_sort_axes_refuses_bad_shapes():
    from geometric_adv_amd import ops
    with pytest.raises(ValueError):
        ops.sort_axes(torch.zeros((1, 16385, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.sort_axes(torch.zeros((0, 8, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.sort_axes(torch.zeros((2, 0, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.sort_axes(torch.zeros((2, 8, 2), device=DEV))
    with pytest.raises(ValueError):
        ops.sort_axes(torch.zeros((2, 8, 3)))


@pytest.mark.parametrize("b, n, batch_size", [(7, 256, 3), (50, 2048, 50)])
def test_evaluate_equals_the_three_separate_calls(b, n, batch_size):
    from conftest import cloud
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    ae = PointNetAE(W.synthetic_weights(n), n)
    pcs = cloud(11, b, n)
    latent, recon, loss = ae.evaluate(pcs, batch_size=batch_size)
    chunks = [pcs[s:s + batch_size] for s in range(0, b, batch_size)]
    assert latent.shape == (b, 128) and recon.shape == (b, n, 3) and loss.shape == (b,)
    assert latent.dtype == recon.dtype == loss.dtype == np.float32
    assert np.array_equal(_bits(latent), _bits(np.vstack([ae.transform(c) for c in chunks])))
    assert np.array_equal(_bits(latent), _bits(np.vstack([ae.get_latent_vectors(c) for c in chunks])))
    assert np.array_equal(_bits(recon), _bits(ae.get_reconstructions(pcs, batch_size=batch_size)))
    assert np.array_equal(_bits(loss), _bits(np.concatenate([ae.get_loss_per_pc(c) for c in chunks])))
    assert np.all(loss > 0)


def _check_eval_folder(eval_dir, set_type, oc, sorted_clouds, labels, slice_idx, ae):
    from geometric_adv_amd import attack_data, tst_ae
    names = tst_ae.eval_file_names(set_type, [oc])
    assert sorted(os.listdir(eval_dir)) == sorted(names.values())
    k = len(sorted_clouds)
    got = {key: np.load(osp.join(eval_dir, names[key])) for key in names if key != "eval_stats"}
    assert list(got["pc_classes"]) == CLASSES
    assert got["pc_label"].dtype == np.int8 and list(got["pc_label"]) == list(labels)
    assert got["slice_idx"].dtype == np.int64 and list(got["slice_idx"]) == list(slice_idx)
    for key, shape in (("point_clouds", (k, N, 3)), ("latent_vectors", (k, 128)), ("reconstructions", (k, N, 3)), ("ae_loss", (k,))):
        assert got[key].dtype == np.float32 and got[key].shape == shape, key
    assert np.array_equal(_bits(got["point_clouds"]), _bits(sorted_clouds))
    assert np.array_equal(_bits(got["latent_vectors"]), _bits(ae.transform(sorted_clouds)))
    assert np.array_equal(_bits(got["reconstructions"]), _bits(ae.get_reconstructions(sorted_clouds)))
    assert np.array_equal(_bits(got["ae_loss"]), _bits(ae.get_loss_per_pc(sorted_clouds)))
    assert open(osp.join(eval_dir, names["eval_stats"])).read() == "Mean ae loss: %.9f\n" % got["ae_loss"].mean()
    return got, attack_data.load_data(eval_dir, os.listdir(eval_dir),
                                      ["point_clouds_" + set_type, "latent_vectors_" + set_type, "pc_classes", "slice_idx_" + set_type,
                                       "ae_loss_" + set_type])


@pytest.mark.parametrize("set_type", ["test_set", "train_set"])
def test_tst_ae_writes_the_eval_folder(tmp_path, golden, set_type):
    from geometric_adv_amd import tf_checkpoint, train_ae, tst_ae, weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    train_dir = tmp_path / "log" / "ae"
    flags = train_ae.parse_flags(["--data_dir", TREE, "--class_names"] + CLASSES)
    train_ae.save_configuration(str(train_dir), train_ae.make_configuration(flags, N))
    w = W.synthetic_weights(N)
    tf_checkpoint.write_checkpoint(str(train_dir / "models.ckpt-3"), w)
    eval_dir = tst_ae.main(["--top_dir", str(tmp_path), "--train_folder", "log/ae", "--restore_epoch", "3", "--data_dir", TREE,
                            "--set_type", set_type, "--output_folder_name", "eval_x"])
    assert eval_dir == str(train_dir / "eval_x")
    got, loaded = _check_eval_folder(eval_dir, set_type, "2l", golden[set_type + "_sorted"], golden[set_type + "_pc_label"],
                                     golden[set_type + "_slice_idx"], PointNetAE(w, N))
    # run_attack's loader reads the folder as it is
    point_clouds, latent_vectors, pc_classes, slice_idx, ae_loss = loaded
    assert np.array_equal(point_clouds, got["point_clouds"]) and np.array_equal(latent_vectors, got["latent_vectors"])
    assert list(pc_classes) == CLASSES and slice_idx[-1] == len(point_clouds) and np.all(ae_loss > 0)


def test_tst_ae_without_sort_axes_and_refusals(tmp_path, golden):
    from geometric_adv_amd import tf_checkpoint, train_ae, tst_ae, weights as W
    train_dir = tmp_path / "ae"
    flags = train_ae.parse_flags(["--data_dir", TREE, "--sort_axes", "0", "--class_names"] + CLASSES)
    train_ae.save_configuration(str(train_dir), train_ae.make_configuration(flags, N))
    tf_checkpoint.write_checkpoint(str(train_dir / "models.ckpt-500"), W.synthetic_weights(N))
    args = ["--top_dir", str(tmp_path), "--train_folder", "ae", "--data_dir", TREE]
    eval_dir = tst_ae.main(args)
    assert np.array_equal(_bits(np.load(osp.join(eval_dir, "point_clouds_test_set_2l.npy"))), _bits(golden["test_set_pc"]))
    with pytest.raises(ValueError, match="--set_type must be one of"):
        tst_ae.main(args + ["--set_type", "all"])
    with pytest.raises(FileNotFoundError):
        tst_ae.main(args + ["--restore_epoch", "7"])
    train_ae.save_configuration(str(train_dir), train_ae.make_configuration(flags, 128))
    with pytest.raises(ValueError, match="the model was trained on"):
        tst_ae.main(args)
    # a folder trained from a .npy names no classes: refused
    np.save(tmp_path / "clouds.npy", np.zeros((2, N, 3), np.float32))
    npy_flags = train_ae.parse_flags(["--train_data", str(tmp_path / "clouds.npy")])
    train_ae.save_configuration(str(train_dir), train_ae.make_configuration(npy_flags, N))
    with pytest.raises(ValueError, match="names no classes"):
        tst_ae.main(args)


def test_train_ae_from_the_ply_folder_then_tst_ae(tmp_path, golden):
    from geometric_adv_amd import train_ae, tst_ae, weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    train_dir = str(tmp_path / "log" / "victim")
    stats = train_ae.main(["--data_dir", TREE, "--class_names"] + CLASSES +
                          ["--train_folder", train_dir, "--training_epochs", "2", "--batch_size", "4", "--held_out_step", "1",
                           "--saver_step", "50"])
    assert [s[0] for s in stats] == [1, 2] and all(np.isfinite(s[1]) and s[1] > 0 for s in stats)
    conf = train_ae.load_configuration(train_dir)
    assert conf["n_input"] == [N, 3] and conf["class_names"] == CLASSES and conf["batch_size"] == 4 and conf["sort_axes"] == 1
    for epoch in (1, 2):
        assert osp.exists(osp.join(train_dir, "models.ckpt-%d.index" % epoch))
    lines = open(osp.join(train_dir, "train_stats.txt")).read().splitlines()
    assert len(lines) == 4
    for epoch in (1, 2):
        e, loss, minutes = lines[2 * epoch - 2].split("\t")
        assert e == "%04d" % epoch and float(loss) == pytest.approx(stats[epoch - 1][1], abs=1e-8)
        held = lines[2 * epoch - 1]
        assert held.startswith("On Held_Out: %04d\t" % epoch)
        held_loss = float(held.split("\t")[1])
        # the validation set is one cloud (fewer than a batch): its own reconstruction error under that epoch's checkpoint
        ae = PointNetAE(W.load(osp.join(train_dir, "models.ckpt-%d" % epoch)), N)
        assert held_loss == pytest.approx(float(ae.get_loss_per_pc(golden["val_set_sorted"]).mean()), abs=1e-8)
    eval_dir = tst_ae.main(["--top_dir", str(tmp_path), "--train_folder", "log/victim", "--restore_epoch", "2", "--data_dir", TREE])
    _check_eval_folder(eval_dir, "test_set", "2l", golden["test_set_sorted"], golden["test_set_pc_label"],
                       golden["test_set_slice_idx"], ae)
