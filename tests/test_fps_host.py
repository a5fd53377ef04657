"""CPU: the farthest-point-sampling model itself (tests/_fps_model.py) against a float64 brute force and at its degenerate
inputs, and everything ops.farthest_point_sample and resample_clouds decide before a device is touched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _fps_model import fps, fps_batch  # noqa: E402


def _brute_force64(x, m, start):
    """'maximise the minimum distance to the chosen set' in float64 -> (idx, the smallest gap between the winning distance and
    the runner-up over all picks, the largest winning distance)."""
    x = x.astype(np.float64)
    chosen = [start]
    gap, top = np.inf, 0.0
    for _ in range(m - 1):
        d = ((x[:, None, :] - x[None, chosen, :]) ** 2).sum(2).min(1)
        order = np.argsort(-d, kind="stable")
        gap = min(gap, d[order[0]] - d[order[1]])
        top = max(top, d[order[0]])
        chosen.append(int(order[0]))
    return np.array(chosen, np.int32), gap, top


@pytest.mark.parametrize("seed,n,m,start", [(0, 200, 60, 0), (1, 333, 100, 17), (2, 64, 40, 63)])
def test_model_equals_the_float64_brute_force_on_tie_free_clouds(seed, n, m, start):
    x = np.random.default_rng(seed).random((n, 3), dtype=np.float32)
    want, gap, top = _brute_force64(x, m, start)
    # an fp32 squared distance of coordinates in [0, 1) is within 6 roundings of 2^-24 relative of the exact one (three
    # differences, three squares, two sums: each operand error doubles in the square): the order of two candidates is safe
    # when the float64 gap exceeds twice that bound at the largest distance
    assert gap > 2 * 8 * 2.0 ** -24 * top, "the cloud is not tie-free in fp32: choose another seed"
    got, t = fps(x, m, start)
    assert np.array_equal(got, want)
    d64 = ((x.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, want, :]) ** 2).sum(2).min(1)
    assert np.allclose(t, d64, rtol=1e-6, atol=0)
    assert t.dtype == np.float32 and not np.isnan(t).any()


def test_model_degenerate_cases():
    rng = np.random.default_rng(5)
    x = rng.random((50, 3), dtype=np.float32)
    # a non-finite point carries t = -1 and is never chosen ...
    bad = x.copy()
    bad[7, 1] = np.nan
    bad[20, 0] = np.inf
    idx, t = fps(bad, 48, 0)
    assert 7 not in idx and 20 not in idx and t[7] == -1 and t[20] == -1 and not np.isnan(t).any()
    assert len(set(idx.tolist())) == 48                                    # the 48 finite points, each once
    # ... except as the given start, which is emitted as given; the next pick is the lowest finite index
    idx, t = fps(bad, 5, 7)
    assert idx[0] == 7 and idx[1] == 0 and 7 not in idx[1:]
    # once every finite point has t = 0 the lowest such index repeats: duplicates ...
    dup = np.concatenate([x[:10], x[:10]])
    idx, t = fps(dup, 16, 3)
    assert len(set(idx[:10].tolist())) == 10 and (idx[:10] < 10).all() and (idx[10:] == 0).all() and (t == 0).all()
    # ... and all-coincident clouds
    idx, t = fps(np.ones((9, 3), np.float32), 5, 4)
    assert idx.tolist() == [4, 0, 0, 0, 0]
    # no finite point: every pick after the first is 0
    idx, t = fps(np.full((6, 3), np.nan, np.float32), 4, 2)
    assert idx.tolist() == [2, 0, 0, 0] and (t == -1).all()
    # a start outside [0, n) is read as 0
    assert np.array_equal(fps(x, 10, -1)[0], fps(x, 10, 0)[0]) and np.array_equal(fps(x, 10, 50)[0], fps(x, 10, 0)[0])
    # m == n on distinct finite points is a permutation
    assert len(np.unique(x, axis=0)) == 50
    assert sorted(fps(x, 50, 11)[0].tolist()) == list(range(50))
    # a point whose distances overflow to +inf is finite, is chosen first, and leaves t = +inf nowhere afterwards
    far = x.copy()
    far[30] = 1e30
    idx, t = fps(far, 3, 0)
    assert idx[1] == 30 and np.isfinite(t[:30]).all()
    # the 8^3 lattice: ties at every pick, lowest index wins
    g = np.arange(8, dtype=np.float32)
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    assert fps(lattice, 5, 0)[0].tolist() == [0, 511, 31, 248, 451]
    # the batched form of the model is the model, cloud by cloud, bit for bit
    batch, starts = np.stack([x, far, bad, np.full_like(x, np.nan), np.concatenate([x[:25], x[:25]])]), [0, 2, 99, 3, -4]
    i5, p5, t5 = fps_batch(batch, 20, starts)
    for c in range(len(batch)):
        i1, t1 = fps(batch[c], 20, starts[c])
        assert np.array_equal(i5[c], i1) and np.array_equal(t5[c].view(np.int32), t1.view(np.int32))
        assert np.array_equal(p5[c].view(np.int32), batch[c][i1].view(np.int32))


def test_op_refuses_bad_inputs_before_any_launch():
    from geometric_adv_amd import ops
    x = torch.zeros((2, 16, 3), dtype=torch.float32)
    with pytest.raises(ValueError, match="GPU"):
        ops.farthest_point_sample(x, 4)                                                        # a CPU tensor
    with pytest.raises(ValueError):
        ops.farthest_point_sample(x.double(), 4)                                               # float64
    # the shape and range checks come after the device check, so they need a tensor that claims to live on the GPU; they
    # raise before anything asks for its device
    class _OnGpu(torch.Tensor):
        is_cuda = True
    for bad, npoint, msg in ((torch.zeros((2, 16, 2)), 4, "3d point sets"), (torch.zeros((2, 16, 3)), 17, "npoint"),
                             (torch.zeros((2, 16, 3)), 0, "npoint"), (torch.zeros((1, 16385, 3)), 4, "16384"),
                             (torch.zeros((16, 3)), 4, "rank")):
        with pytest.raises(ValueError, match=msg):
            ops.farthest_point_sample(bad.as_subclass(_OnGpu), npoint)
    with pytest.raises(ValueError, match="form"):
        ops.farthest_point_sample(x, 4, form="block")


def test_dispatch_plan_of_the_library():
    """The plan query answers without a device: forms, limits and the refusals of the C entry."""
    from geometric_adv_amd import ops
    assert ops.farthest_point_sample_plan(64) == ("wave", 1, 1)
    assert ops.farthest_point_sample_plan(256) == ("wave", 1, 4)
    assert ops.farthest_point_sample_plan(257) == ("workgroup", 4, 4)
    assert ops.farthest_point_sample_plan(1024, "wave") == ("wave", 1, 16)
    assert ops.farthest_point_sample_plan(16384) == ("workgroup", 16, 16)
    for n, form in ((0, "auto"), (16385, "auto"), (1025, "wave")):
        with pytest.raises(ValueError):
            ops.farthest_point_sample_plan(n, form)
    for waves_form in ("auto", "workgroup", "wave"):
        for n in (1, 63, 64, 65, 255, 256, 257, 1023, 1024):
            form, waves, ppt = ops.farthest_point_sample_plan(n, waves_form)
            assert waves * 64 * ppt >= n                                   # the registers of the instance hold the cloud


def test_c_entry_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    from geometric_adv_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()
    out = (C.c_int * 64)()
    p, o = C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)

    def status(b=1, n=4, xyz=p, m=2, form=0, idx=o, sampled=None, mindist=None):
        return L.geoadv_farthest_point_sample(b, n, xyz, m, None, form, idx, sampled, mindist, None)
    for kw in (dict(b=0), dict(n=0), dict(n=16385, m=1), dict(m=0), dict(m=5), dict(xyz=None), dict(idx=None), dict(form=3), dict(form=-1),
               dict(sampled=p), dict(mindist=C.c_void_p(p.value + 8)), dict(n=1025, form=2)):
        assert status(**kw) == 1, kw
        assert b"farthest_point_sample" in L.geoadv_last_error()


def test_resample_clouds_parser():
    from geometric_adv_amd import resample_clouds
    p = resample_clouds.build_parser()
    f = p.parse_args(["--input", "a.npy", "--output", "b.npy", "--n_points", "2048"])
    assert (f.input, f.output, f.n_points) == ("a.npy", "b.npy", 2048)
    assert (f.batch_size, f.start, f.seed, f.save_idx, f.device) == (64, "first", 0, None, "cuda:0")
    f = p.parse_args(["--input", "a", "--output", "b", "--n_points", "8", "--batch_size", "3", "--start", "random", "--seed", "3",
                      "--save_idx", "i.npy", "--device", "cuda:1"])
    assert (f.batch_size, f.start, f.seed, f.save_idx, f.device) == (3, "random", 3, "i.npy", "cuda:1")
    for argv in (["--output", "b", "--n_points", "8"], ["--input", "a", "--n_points", "8"], ["--input", "a", "--output", "b"],
                 ["--input", "a", "--output", "b", "--n_points", "8", "--start", "last"]):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_resample_clouds_refuses_large_clouds_before_a_device_is_touched(tmp_path, monkeypatch):
    from geometric_adv_amd import resample_clouds
    src = str(tmp_path / "big.npy")
    np.save(src, np.zeros((1, 16385, 3), np.float32))

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(torch, "device", no_device)
    monkeypatch.setattr(torch.Tensor, "to", no_device)
    with pytest.raises(ValueError, match="16384"):
        resample_clouds.main(["--input", src, "--output", str(tmp_path / "out.npy"), "--n_points", "1024"])
    assert not (tmp_path / "out.npy").exists()
    np.save(src, np.zeros((2, 100, 3), np.float32))
    with pytest.raises(ValueError, match="n_points"):
        resample_clouds.main(["--input", src, "--output", str(tmp_path / "out.npy"), "--n_points", "101"])
    np.save(src, np.zeros((2, 100, 2), np.float32))
    with pytest.raises(ValueError, match="shape"):
        resample_clouds.main(["--input", src, "--output", str(tmp_path / "out.npy"), "--n_points", "10"])
