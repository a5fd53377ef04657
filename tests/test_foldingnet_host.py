"""CPU: the FoldingNet auto-encoder's weights contract (key names, checkpoint loading), the grid, the float64 model and the
reference-mode host sampler against the reference modules' golden, the device sampler's numpy restatement, the ctypes
mirror of geoadv_fold_weights and run_transfer's refusal without a seed (no GPU)."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

import _fold_model64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "foldingnet.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _state():
    from geometric_adv_amd import fold_weights as FW
    return FW.synthetic_state(int(_golden()["weight_seed"]))


def test_key_names_equal_the_reference_modules():
    from geometric_adv_amd import fold_weights as FW
    assert FW.key_names() == [str(k) for k in _golden()["keys"]]
    assert FW.key_names("module.")[0] == "module.encoder.conv1.weight"


def test_grid_equals_the_reference():
    from geometric_adv_amd import fold_weights as FW
    g = _golden()["grid"]
    assert g.shape == (2025, 2) and np.array_equal(FW.grid(), g)


def test_synthetic_weights_are_the_goldens():
    from geometric_adv_amd import fold_weights as FW
    h = hashlib.sha256()
    for k in FW.key_names():
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(_state()[k], np.float32).tobytes())
    assert h.hexdigest() == str(_golden()["sha256"])


def test_float64_model_equals_the_reference_modules():
    """tests/_fold_model64.py with the golden positions against the reference's modules run in float64."""
    g = _golden()
    x = g["clouds"]
    cov, rows = M.graph_from_knn(x, M.knn(x))
    assert np.array_equal(M.degrees(rows), g["degree"])
    assert np.array_equal(cov[:, :g["cov"].shape[1]], g["cov"])
    cols = M.resolve(rows, g["positions"])
    code, p1, rec = M.model(_state(), x, cov, cols)
    for got, key in ((code, "code"), (p1, "p1"), (rec, "recon")):
        assert np.abs(got - g[key]).max() <= 1e-10 * max(1.0, np.abs(g[key]).max()), key


def test_fold_weights_forward64_agrees():
    from geometric_adv_amd import fold_weights as FW
    g = _golden()
    x = g["clouds"][:2]
    knn, cov, rows = FW.knn_graph(x)
    cols = FW.resolve(rows, g["positions"][:, :2])
    code, p1, rec = FW.forward64({k: v.astype(np.float64) for k, v in _state().items()}, x, cov, cols)
    assert np.abs(rec - g["recon"][:2]).max() <= 1e-9 * max(1.0, np.abs(rec).max())
    assert np.abs(code - g["code"][:2]).max() <= 1e-9 * max(1.0, np.abs(code).max())


def test_synthetic_model_is_calibrated():
    g = _golden()
    assert 0.1 < np.abs(g["code"]).mean() < 10 and 0.05 < np.abs(g["recon"]).std() < 10
    assert 0.05 < g["p1"].std() < 10


def test_reference_sampler_reproduces_every_golden_position():
    """FoldingNetAE's reference mode (one RandomState for the object's life, chunks of 4, pool 1 then pool 2 per chunk)
    against the positions the reference drew after np.random.seed, over both of its get_reconstructions calls."""
    from geometric_adv_amd.foldingnet import FoldingNetAE
    g = _golden()
    ae = FoldingNetAE.__new__(FoldingNetAE)                 # the host sampler alone: no device handle needed
    ae._rs = np.random.RandomState(int(g["graph_seed"]))
    start, got = 0, []
    for count in g["calls"]:
        got.append(ae.reference_picks(g["degree"][start:start + count].astype(np.int64)))
        start += count
    got = np.concatenate(got, axis=1)
    assert got.shape == g["positions"].shape
    assert np.array_equal(got, g["positions"].astype(np.int32))
    # one call of all six clouds is a different run of the reference (its chunks are 4 + 2): the draws differ
    ae._rs = np.random.RandomState(int(g["graph_seed"]))
    assert not np.array_equal(ae.reference_picks(g["degree"].astype(np.int64)), got)


def test_device_sampler_restatement_draws_distinct_positions_in_range():
    rng = np.random.default_rng(0)
    deg = rng.integers(16, 300, size=(3, 500))
    deg[0, :5] = 16
    p = M.device_picks(12345, [0, 1, 7], deg)
    assert p.shape == (2, 3, 500, 16)
    assert (p >= 0).all() and (p < deg[None, :, :, None]).all()
    s = np.sort(p, axis=3)
    assert (np.diff(s, axis=3) > 0).all()
    assert np.array_equal(np.sort(p[:, 0, :5], axis=2), np.broadcast_to(np.arange(16), (2, 5, 16)))
    # ordinal-keyed: a cloud's picks depend on its ordinal, not on its neighbours in the batch
    q = M.device_picks(12345, [7], deg[2:3])
    assert np.array_equal(q[:, 0], p[:, 2])
    assert not np.array_equal(M.device_picks(12346, [0, 1, 7], deg), p)


def _write_checkpoint(path, epoch=7, prefix="", drop=(), reshape=None, extra=None):
    import torch
    from geometric_adv_amd import fold_weights as FW
    state = _state()
    FW.save(str(path), epoch, state, prefix=prefix)
    if drop or reshape or extra:
        ck = torch.load(FW.checkpoint_path(str(path), epoch), weights_only=False)
        for k in drop:
            del ck["model"][k]
        for k, shape in (reshape or {}).items():
            ck["model"][k] = torch.zeros(shape)
        ck["model"].update(extra or {})
        torch.save(ck, FW.checkpoint_path(str(path), epoch))
    return state


@pytest.mark.parametrize("prefix", ["", "module."])
def test_loader_reads_a_checkpoint(tmp_path, prefix):
    import torch
    from geometric_adv_amd import fold_weights as FW
    state = _write_checkpoint(tmp_path, 250, prefix)
    ck = torch.load(str(tmp_path / "checkpoint_250.pth"), weights_only=False)
    assert set(ck) == {"epoch", "model", "optimizer"} and prefix + "encoder.bn6.num_batches_tracked" in ck["model"]
    got = FW.load(str(tmp_path), 250)
    assert set(got) == set(FW.key_shapes())
    for k, v in got.items():
        assert np.array_equal(v, state[k])
    c = FW.canonical(got)
    assert c["enc_w"][0].shape == (12, 64) and c["enc_w"][5].shape == (1024, 512) and c["enc_gamma"][6] is None
    assert c["dec_w"][0].shape == (514, 512) and c["dec_w"][3].shape == (515, 512) and c["dec_w"][5].shape == (512, 3)
    assert np.array_equal(c["dec_w"][3], state["decoder.fold2.conv1.weight"][:, :, 0].T)


def test_loader_reports_every_bad_key_at_once(tmp_path):
    import torch
    from geometric_adv_amd import fold_weights as FW
    _write_checkpoint(tmp_path, drop=["encoder.fc1.bias", "encoder.bn6.running_var"],
                      reshape={"decoder.fold2.conv1.weight": (512, 514, 1)},
                      extra={"encoder.conv6.weight": torch.zeros(3, 3, 1)})
    with pytest.raises(KeyError) as e:
        FW.load(str(tmp_path), 7)
    msg = str(e.value)
    for s in ("encoder.fc1.bias", "encoder.bn6.running_var", "decoder.fold2.conv1.weight", "encoder.conv6.weight",
              "2 missing", "1 unexpected", "1 of the wrong shape"):
        assert s in msg


def test_run_transfer_without_a_graph_seed_still_exits(tmp_path):
    from geometric_adv_amd import run_transfer
    missing = str(tmp_path / "does_not_exist")
    with pytest.raises(SystemExit, match="np.random.choice.*--graph_seed|--graph_seed.*np.random.choice"):
        run_transfer.main(["--transfer_ae_type", "FoldingNet", "--top_dir", missing, "--graph_sampling", "reference"])
    assert not os.path.exists(missing)
    with pytest.raises(SystemExit):
        run_transfer.main(["--transfer_ae_type", "FoldingNet", "--graph_sampling", "other", "--graph_seed", "1"])


def test_library_exports_the_fold_entry_points():
    from geometric_adv_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("geoadv_fold_create", "geoadv_fold_destroy", "geoadv_fold_workspace_bytes", "geoadv_fold_graph",
                 "geoadv_fold_forward"):
        assert hasattr(lib, name), name


def test_python_mirror_matches_the_header():
    from test_classifier_host import _header_struct
    from geometric_adv_amd.foldingnet import _FoldWeights
    got = [(f, "ptr", t._length_) for f, t in _FoldWeights._fields_]
    assert all(t._type_ is ctypes.c_void_p for _, t in _FoldWeights._fields_)
    assert got == _header_struct("geoadv_fold_weights")
    assert ctypes.sizeof(_FoldWeights) == (6 * 7 + 2 * 6) * ctypes.sizeof(ctypes.c_void_p)
