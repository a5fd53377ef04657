"""GPU: FoldingNetAE.evaluate and the tst_foldingnet command on a checkpoint of freshly initialised weights and five clouds
of 64 points: the per-cloud losses against get_loss_per_pc of get_reconstructions (bit for bit, both samplings), their
independence of the batch size, a float64 brute-force Chamfer distance, and the command's numbers, lines and refusals."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CLOUDS, SEED, EPOCH = 64, 5, 7, 3
# The losses against a float64 Chamfer distance of the same float32 clouds.  Every fp32 squared distance is a sum of three
# non-negative squares of fp32 differences: within about 6 * 2^-24 relative.  The nearest neighbour found in fp32 may be
# another point than in float64, but only one whose distance is within that error of the minimum.  The fp32 mean of up to
# 2048 (here 2025 and 64) non-negative values adds a few 2^-24 more.  Together below 2e-6; 1e-5 leaves a margin of five.
RTOL = 1e-5


@functools.lru_cache(maxsize=None)
def _state():
    from geometric_adv_amd import fold_weights as FW
    return FW.initial_weights(SEED)


@functools.lru_cache(maxsize=None)
def _clouds():
    return (np.random.default_rng(3).random((CLOUDS, N, 3)) - 0.5).astype(np.float32)


def _ae(sampling="device", batch_size=2, seed=11):
    from geometric_adv_amd.foldingnet import FoldingNetAE
    return FoldingNetAE(state=_state(), seed=seed, sampling=sampling, batch_size=batch_size)


def _chamfer64(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    d = ((a[:, :, None, :] - b[:, None, :, :]) ** 2).sum(-1)
    return d.min(2).mean(1) + d.min(1).mean(1)


@pytest.mark.parametrize("sampling", ["device", "reference"])
def test_evaluate_scores_get_reconstructions(sampling):
    x = _clouds()
    res = _ae(sampling).evaluate(x)
    assert sorted(res) == ["loss_per_pc", "mid_loss_per_pc"]
    for v in res.values():
        assert v.shape == (CLOUDS,) and v.dtype == np.float32 and np.all(v > 0)
    fresh = _ae(sampling)
    assert np.array_equal(res["loss_per_pc"], fresh.get_loss_per_pc(fresh.get_reconstructions(x), x))
    assert not np.array_equal(res["loss_per_pc"], res["mid_loss_per_pc"])


@pytest.mark.parametrize("sampling", ["device", "reference"])
def test_evaluate_does_not_depend_on_batch_size(sampling):
    x = _clouds()
    a, b = _ae(sampling, batch_size=2).evaluate(x), _ae(sampling, batch_size=5).evaluate(x)      # 2 + 2 + 1 clouds, and 5
    assert np.array_equal(a["loss_per_pc"], b["loss_per_pc"]) and np.array_equal(a["mid_loss_per_pc"], b["mid_loss_per_pc"])


def test_evaluate_advances_the_ordinals_like_get_reconstructions():
    """A second evaluate scores the clouds at the ordinals that follow, as a second get_reconstructions would."""
    x = _clouds()
    ae, fresh = _ae(), _ae()
    ae.evaluate(x)
    fresh.get_reconstructions(x)
    assert np.array_equal(ae.evaluate(x)["loss_per_pc"], fresh.get_loss_per_pc(fresh.get_reconstructions(x), x))


def test_evaluate_against_float64_chamfer():
    x = _clouds()
    ae = _ae()
    res = ae.evaluate(x)
    out = _ae().forward(x, cloud_offset=0, p1=True)
    for key, which in (("loss_per_pc", "recon"), ("mid_loss_per_pc", "p1")):
        want = _chamfer64(x, out[which].cpu().numpy())
        err = np.abs(res[key] - want) / want
        print("%s: max relative error %.2e" % (key, err.max()))
        assert np.allclose(res[key], want, rtol=RTOL, atol=0), (key, err)


def _checkpoint(tmp_path):
    from geometric_adv_amd import fold_weights as FW
    FW.save(str(tmp_path / "log" / "fold"), EPOCH, _state())
    np.save(tmp_path / "clouds.npy", _clouds())
    return ["--top_dir", str(tmp_path), "--test_set", "clouds.npy", "--outf", "log/fold", "--checkpoint_num", str(EPOCH)]


def test_cli_returns_and_prints_the_float64_means(tmp_path, capsys):
    from geometric_adv_amd import tst_foldingnet
    base = _checkpoint(tmp_path)
    before = sorted(p.name for p in tmp_path.rglob("*"))
    got = tst_foldingnet.main(base + ["--num_points", str(N), "--batchSize", "2", "--graph_seed", "11"])
    res = _ae(batch_size=2).evaluate(_clouds())
    want = (float(np.mean(res["loss_per_pc"].astype(np.float64))), float(np.mean(res["mid_loss_per_pc"].astype(np.float64))))
    assert got == want
    lines = capsys.readouterr().out.splitlines()
    assert lines[-1] == "Testing test loss: %f middle test loss: %f" % want
    batches = [l for l in lines if l.startswith("Batch ")]
    assert [l.split("\t")[0] for l in batches] == ["Batch 0/2", "Batch 1/2", "Batch 2/2"]          # %d of 5 / 2, as the reference
    assert all(l.split("\t")[1].startswith(" Duration (minutes): ") for l in batches)
    assert sorted(p.name for p in tmp_path.rglob("*")) == before                                   # the command writes nothing
    assert tst_foldingnet.main(base + ["--num_points", str(N), "--batchSize", "5", "--graph_seed", "11"]) == want


def test_cli_refusals(tmp_path):
    from geometric_adv_amd import tst_foldingnet
    with pytest.raises(SystemExit, match="--graph_seed"):                 # before any file is read: none of these exists
        tst_foldingnet.main(["--top_dir", str(tmp_path), "--test_set", "missing.npy", "--outf", "missing"])
    base = _checkpoint(tmp_path)
    with pytest.raises(AssertionError, match="--num_points"):
        tst_foldingnet.main(base + ["--num_points", "2048", "--graph_seed", "11"])
