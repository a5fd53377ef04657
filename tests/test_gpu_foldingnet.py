"""GPU: the FoldingNet auto-encoder (csrc/foldingnet.hip through geoadv_fold_* and foldingnet.FoldingNetAE) against the
reference modules' golden and the float64 model of tests/_fold_model64.py: the graph, both sampling modes, the device
sampler's exact draws and distribution, isolation, refusals, streams, the Chamfer loss and the run_transfer CLI."""
import functools
import json
import os

import numpy as np
import pytest

import _fold_model64 as M

pytestmark = pytest.mark.gpu

# TOLERANCE, on max |got - ref| / max(1, max |ref|).  Every layer is an fp32 dot product (MFMA fp32 accumulation or an
# fmaf chain) whose rounding is about sqrt(K) * 2^-24 of the magnitudes summed; a coordinate sits at the end of 13 of them
# (conv1..conv5, fc1, fc2, the folds' code rows, two 512 x 512 layers, two 512 -> 3 layers), with K up to 1024, and bn6
# divides by statistics taken across clouds that differ little.  The graph pools are exact (a max of the same values), and
# the covariance is formed in float64 and rounded once.  AtlasNet's 11-layer chain holds 1e-4; measured here on the
# MI355X (the prints below): codes within 7.9e-7 of float64, p1 within 2.9e-6 and reconstructions within 3.6e-6 over the
# golden and n = 17 ... 4096.  The bound is 2e-5, over five times the largest; every "told apart" mistake moves the output
# by more than 50 x TOL (measured: 0.09 ... 0.85).
TOL = 2e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "foldingnet.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def _state(seed=None):
    from geometric_adv_amd import fold_weights as FW
    return FW.synthetic_state(int(_golden()["weight_seed"]) if seed is None else seed)


def _ae(sampling="device", seed=5, batch_size=32):
    from geometric_adv_amd.foldingnet import FoldingNetAE
    return FoldingNetAE(state=_state(), seed=seed, sampling=sampling, batch_size=batch_size)


def _clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max())


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def test_graph_against_the_golden():
    g = _golden()
    ae = _ae()
    x = g["clouds"]
    deg, knn, cov = (t.cpu().numpy() for t in ae.graph(x))
    assert np.array_equal(deg, g["degree"])
    want = M.knn(x)
    assert np.array_equal(np.sort(knn, axis=2), np.sort(want, axis=2))          # the 16-sets (no ties in these clouds)
    ref = g["cov"]
    got = cov[:, :ref.shape[1]]
    scale = np.abs(ref).max(axis=2, keepdims=True)
    assert (np.abs(got - ref) <= 1e-5 * scale).all()
    # the resolved columns at the golden positions equal a float64 numpy graph's
    _, rows = M.graph_from_knn(x, want)
    out = _np(ae.forward(x, picks=g["positions"].astype(np.int32)))
    assert np.array_equal(out["cols"], M.resolve(rows, g["positions"]))


def test_reference_mode_reproduces_the_golden():
    """Two successive get_reconstructions calls (5 clouds, then 1) of a reference-mode object reproduce the reference's
    own run after np.random.seed(seed); the code and p1 through forward with the same positions."""
    g = _golden()
    ae = _ae("reference", seed=int(g["graph_seed"]), batch_size=3)
    start, recs = 0, []
    for count in g["calls"]:
        recs.append(ae.get_reconstructions(g["clouds"][start:start + count]))
        start += count
    rec = np.concatenate(recs)
    out = _np(ae.forward(g["clouds"], picks=g["positions"].astype(np.int32), p1=True))
    ec, ep, er = _err(out["code"], g["code"]), _err(out["p1"], g["p1"]), _err(rec, g["recon"])
    print("golden: code %.2e p1 %.2e recon %.2e" % (ec, ep, er))
    assert rec.shape == (6, 2025, 3) and rec.dtype == np.float32
    assert ec <= TOL and ep <= TOL and er <= TOL
    assert np.array_equal(out["recon"], rec)


@pytest.mark.parametrize("b,n", [(1, 17), (3, 1000), (4, 2048), (2, 4096)])
def test_device_mode_against_float64(b, n):
    ae = _ae()
    x = _clouds(300 + n, b, n)
    deg, knn, _ = (t.cpu().numpy() for t in ae.graph(x))
    want = M.knn(x)
    same = (np.sort(knn, axis=2) == np.sort(want, axis=2)).all(axis=2)
    assert same.mean() > 0.999                  # fp32 against float64 distances: only near-ties may differ
    cov, rows = M.graph_from_knn(x, knn)        # the model on the GPU's own kNN
    assert np.array_equal(M.degrees(rows), deg)
    out = _np(ae.forward(x, cloud_offset=11, p1=True))
    assert np.array_equal(out["picks"], M.device_picks(ae.seed, np.arange(b) + 11, deg))
    cols = M.resolve(rows, out["picks"])
    assert np.array_equal(out["cols"], cols)
    code, p1, rec = M.model(_state(), x, cov, cols)
    e = (_err(out["code"], code), _err(out["p1"], p1), _err(out["recon"], rec))
    print("b %d n %d: code %.2e p1 %.2e recon %.2e" % ((b, n) + e))
    assert max(e) <= TOL


def test_high_degree_rows():
    """A point that is everybody's neighbour: six tight clusters of 15 points on the axes around it, each point's 16
    nearest being its 14 cluster mates, the centre and one point of another cluster -- the centre's row holds all 90
    (more than a wave's 64)."""
    rng = np.random.default_rng(4)
    axes = np.concatenate([np.eye(3), -np.eye(3)]) * 0.3
    pts = [np.zeros((1, 3))] + [a + 1e-3 * rng.standard_normal((15, 3)) for a in axes]
    x = np.concatenate(pts)[None].astype(np.float32)
    x = np.concatenate([x, _clouds(5, 1, 91)])
    ae = _ae()
    deg, knn, _ = (t.cpu().numpy() for t in ae.graph(x))
    _, rows = M.graph_from_knn(x, knn)
    assert np.array_equal(M.degrees(rows), deg)
    assert deg[0, 0] == 90
    out = _np(ae.forward(x))
    assert np.array_equal(out["cols"], M.resolve(rows, out["picks"]))
    assert (out["picks"] < deg[None, :, :, None]).all() and np.isfinite(out["recon"]).all()


def test_device_picks_are_keyed_by_ordinal():
    ae = _ae()
    x = _clouds(7, 6, 700)
    a = _np(ae.forward(x, cloud_offset=0))
    b = _np(ae.forward(x[2:5], cloud_offset=2))
    assert np.array_equal(b["picks"], a["picks"][:, 2:5]) and np.array_equal(b["recon"], a["recon"][2:5])
    c = _np(ae.forward(x, cloud_offset=0))
    assert np.array_equal(c["picks"], a["picks"]) and np.array_equal(c["recon"], a["recon"])
    d = _np(ae.forward(x, seed=6))
    assert not np.array_equal(d["picks"], a["picks"])
    # alone, at the front of a batch, a cloud draws by its ordinal
    e = _np(ae.forward(x[3:4], cloud_offset=3))
    assert np.array_equal(e["picks"][:, 0], a["picks"][:, 3]) and np.array_equal(e["recon"][0], a["recon"][3])
    f = _np(ae.forward(x[3:4], cloud_offset=0))
    assert np.array_equal(f["picks"], M.device_picks(ae.seed, [0], ae.graph(x[3:4])[0].cpu().numpy()))
    assert not np.array_equal(f["picks"][:, 0], a["picks"][:, 3])
    # get_reconstructions: the running ordinal makes results independent of batch_size and of the split between calls
    r1 = _ae(batch_size=32).get_reconstructions(x)
    ae2 = _ae(batch_size=4)
    r2 = np.concatenate([ae2.get_reconstructions(x[:1]), ae2.get_reconstructions(x[1:])])
    assert np.array_equal(r1, r2) and np.array_equal(r1, a["recon"])


def test_device_sampler_frequencies():
    """Fixed seed: every position of a row is drawn with frequency 16 / deg (chi-square over many rows of equal degree)."""
    ae = _ae(seed=99)
    x = _clouds(8, 16, 2048)
    out = _np(ae.forward(x))
    deg = ae.graph(x)[0].cpu().numpy()
    for d in (17, 18, 20):
        sel = out["picks"][:, deg == d]                           # (2, rows, 16)
        rows = sel.shape[1] * 2
        if rows < 500:
            continue
        counts = np.bincount(sel.reshape(-1), minlength=d)
        expect = rows * 16 / d
        chi2 = ((counts - expect) ** 2 / expect).sum()
        # with 16 of d drawn the counts are negatively correlated; the plain chi-square (d - 1 dof) is conservative
        assert chi2 < d - 1 + 6 * np.sqrt(2 * (d - 1)), (d, counts)


def test_non_default_stream_same_bits():
    """The delayed-call protocol of tests/_stream_order.py: behind a pending delay on a side stream, over scratch that holds
    another batch's values, the forward gives the default stream's bits and does not block the host."""
    import torch
    import _stream_order as SO
    ae = _ae()
    a, b = (torch.from_numpy(_clouds(s, 10, 1500)).to("cuda:0") for s in (30, 31))

    def forward(x):
        out = ae.forward(x, p1=True)
        return [out[k] for k in sorted(out)]
    SO.check_call("foldingnet.forward", forward, [a], [b], keep=ae)


def test_nonfinite_cloud_is_isolated():
    ae = _ae()
    x = _clouds(41, 5, 700)
    a = _np(ae.forward(x))
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[2, 17, 1] = bad
        y[2, 40] = bad
        b = _np(ae.forward(y))
        keep = [0, 1, 3, 4]
        for k in ("code", "recon", "picks", "cols"):
            assert np.array_equal(b[k][..., keep, :, :] if k in ("picks", "cols") else b[k][keep],
                                  a[k][..., keep, :, :] if k in ("picks", "cols") else a[k][keep]), k
        assert (b["cols"] >= 0).all() and (b["cols"] < 700).all()


def test_refusals():
    import ctypes
    import torch
    from geometric_adv_amd import _lib
    from geometric_adv_amd.foldingnet import FoldingNetAE
    ae = _ae()
    lib = _lib.lib()
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda:0")
    x = torch.zeros((2, 16385, 3), device="cuda:0")
    for b, n in ((1, 16), (1, 16385), (0, 100), (-1, 100)):
        assert lib.geoadv_fold_graph(ae.handle, b, n, _lib.ptr(x), None, None, None, _lib.ptr(ws), None) == 1
        assert lib.geoadv_fold_forward(ae.handle, b, n, _lib.ptr(x), 1, ctypes.c_ulonglong(1), ctypes.c_longlong(0), None,
                                       None, None, None, None, _lib.ptr(ws), None) == 1
    with pytest.raises(ValueError):
        ae.forward(torch.zeros((1, 16, 3), device="cuda:0"))
    with pytest.raises(ValueError):
        ae.forward(torch.zeros((1, 100, 2), device="cuda:0"))
    y = _clouds(3, 2, 300)
    deg = ae.graph(y)[0].cpu().numpy()
    picks = np.broadcast_to(np.arange(16, dtype=np.int32), (2, 2, 300, 16)).copy()
    picks[1, 1, 77, 5] = deg[1, 77]
    with pytest.raises(ValueError, match=r"picks\[1, 1, 77, 5\]"):
        ae.forward(y, picks=picks)
    picks[1, 1, 77, 5] = -1
    with pytest.raises(ValueError):
        ae.forward(y, picks=picks)
    with pytest.raises(ValueError):
        FoldingNetAE(state=_state(), seed=None)
    with pytest.raises(ValueError):
        FoldingNetAE(state=_state(), seed=1, sampling="host")


def test_mistakes_are_told_apart():
    """Each of these mistakes moves the output by more than 50 x TOL: the comparisons above would catch it."""
    g = _golden()
    x = g["clouds"][:3]
    knn = M.knn(x)
    cov, rows = M.graph_from_knn(x, knn)
    cols = M.resolve(rows, g["positions"][:, :3])
    out = _np(_ae().forward(x, picks=g["positions"][:, :3].astype(np.int32)))
    _, _, want = M.model(_state(), x, cov, cols)
    assert _err(out["recon"], want) <= TOL
    cov0, _ = M.graph_from_knn(x, knn, ddof=0)
    wrong = {"no max with self": M.model(_state(), x, cov, cols, no_self=True)[2],
             "ddof 0": M.model(_state(), x, cov0, cols)[2],
             "swapped grid axes": M.model(_state(), x, cov, cols, swap_grid=True)[2],
             "fold2 fed the grid": M.model(_state(), x, cov, cols, fold2_grid=True)[2]}
    for k, w in wrong.items():
        print("%s: %.2e" % (k, _err(w, want)))
        assert _err(w, want) > 50 * TOL, k


def test_loss_per_pc_equals_the_oracle_chamfer():
    from oracle.cpu_oracle import Oracle
    ae = _ae()
    recon = ae.get_reconstructions(_clouds(51, 5, 2048))
    target = _clouds(52, 5, 2048)
    got = ae.get_loss_per_pc(recon, target)
    d1, _, d2, _ = Oracle().nn_distance(recon, target)
    want = d1.astype(np.float64).mean(1) + d2.astype(np.float64).mean(1)
    assert got.shape == (5,) and np.allclose(got, want, rtol=1e-5, atol=0)


def test_run_transfer_end_to_end(tmp_path):
    from test_gpu_atlasnet import _eval_folder
    from geometric_adv_amd import fold_weights as FW, run_transfer
    from geometric_adv_amd.foldingnet import FoldingNetAE
    n = 256
    adv = _eval_folder(tmp_path, n)
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy",
            "--transfer_ae_type", "FoldingNet", "--transfer_ae_folder", "log/fold", "--transfer_ae_restore_epoch", "40"]
    FW.save(str(tmp_path / "log" / "fold"), 40, _state())
    out = tmp_path / "log" / "fold" / "eval" / "attack_res_transfer"
    results = {}
    for sampling in ("device", "reference", "reference"):
        run_transfer.main(base + ["--graph_seed", "17", "--graph_sampling", sampling])
        with open(out / "transfer_configuration.json") as f:
            conf = json.load(f)
        assert conf["graph_seed"] == 17 and conf["graph_sampling"] == sampling and conf["transfer_ae_type"] == "FoldingNet"
        files = {name: (np.load(out / name / "transferred_pc_recon.npy"), np.load(out / name / "transfer_metrics.npy"))
                 for name in adv}
        for name, (pc_in, metrics, tgt, tloss) in adv.items():
            rec, tm = files[name]
            assert rec.shape == (1, len(pc_in), 2025, 3) and tm.shape == (1, len(pc_in), 4)
            assert np.array_equal(tm[0, :, 2], metrics[:, 4]) and np.array_equal(tm[0, :, 1], tm[0, :, 0] / tloss)
        if sampling in results:                          # reference mode: the same files on a second run
            for name in adv:
                assert all(np.array_equal(a, b) for a, b in zip(files[name], results[sampling][name]))
        results[sampling] = files
    # device mode: one object over the classes in order, as run_transfer makes it
    ae = FoldingNetAE(str(tmp_path / "log" / "fold"), epoch=40, seed=17, sampling="device")
    for name in ("chair", "car"):
        if name in adv:
            assert np.array_equal(results["device"][name][0][0], ae.get_reconstructions(adv[name][0]))
