"""GPU: plain Python values reach the C functions with the header's types.  Every case calls the function through _lib.lib() with
bare ints and floats -- no ctypes wrapper on any scalar -- and compares bit for bit with the ops wrapper on the same inputs: one
case per scalar type the header has beyond int (unsigned long long, double, float, long long and size_t)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stat_defense_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG = (1 << 40) + 3            # does not fit 32 bits: passed as a C int it would arrive as 3


def _cloud(seed, b, n):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5))).to(DEV)


def test_model_pins_for_the_wide_seed():
    """The numbers the unsigned long long case stands on (CPU model): the wide seed and the wide counter draw other points than 3."""
    assert M.srs_dropped(BIG, 0, np.arange(2, dtype=np.uint64), 16, 5)[0].tolist() == [2, 3, 6, 11, 14]
    assert M.srs_dropped(3, 0, np.arange(2, dtype=np.uint64), 16, 5)[0].tolist() == [0, 1, 6, 7, 11]
    wide, narrow = (M.srs_dropped(0, c, np.arange(2, dtype=np.uint64), 16, 5) for c in (BIG, 3))
    assert (wide[0] != narrow[0]).any() and (wide[1] != narrow[1]).any()


@pytest.mark.parametrize("seed,counter", [(BIG, 0), (0, BIG)])
def test_unsigned_long_long_random_drop(seed, counter):
    from geometric_adv_amd import _lib, ops
    b, n, drop = 2, 16, 5
    pc = _cloud(1, b, n)
    kept = torch.empty_like(pc)
    idx = torch.full((b, drop), -1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        st = _lib.lib().geoadv_random_drop(b, n, pc.data_ptr(), drop, seed, counter, 0, kept.data_ptr(), idx.data_ptr(),
                                           _lib.stream_handle())
    _lib.check(st, "random_drop")
    want = M.srs_dropped(seed, counter, np.arange(b, dtype=np.uint64), n, drop)
    narrow = M.srs_dropped(seed & 0xffffffff, counter & 0xffffffff, np.arange(b, dtype=np.uint64), n, drop)
    got = idx.cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[0] != narrow[0]).any() and (got[1] != narrow[1]).any()
    op_kept, op_idx = ops.random_drop(pc, drop, seed, counter, return_idx=True)
    assert np.array_equal(op_idx.cpu().numpy(), got)
    assert np.array_equal(op_kept.cpu().numpy().view(np.int32), kept.cpu().numpy().view(np.int32))


def test_double_rotate_y():
    from geometric_adv_amd import _lib, ops
    pc = _cloud(2, 1, 4)
    angle = 0.7
    out = torch.empty_like(pc)
    with torch.cuda.device(DEV):
        st = _lib.lib().geoadv_rotate_y(1, 4, pc.data_ptr(), float(np.cos(angle)), float(np.sin(angle)), out.data_ptr(),
                                        _lib.stream_handle())
    _lib.check(st, "rotate_y")
    got = out.cpu().numpy()
    assert not np.array_equal(got, pc.cpu().numpy())
    assert np.array_equal(got.view(np.int32), ops.rotate_point_cloud_by_angle(pc, angle).cpu().numpy().view(np.int32))


def test_float_query_ball_point():
    from geometric_adv_amd import _lib, ops
    xyz = _cloud(3, 1, 8)
    d = torch.cdist(xyz[0].double(), xyz[0].double()).cpu().numpy()
    radius = float(np.median(d[d > 0]))                   # splits the points: some pairs inside, some outside
    idx = torch.zeros((1, 8, 8), dtype=torch.int32, device=DEV)
    cnt = torch.zeros((1, 8), dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        st = _lib.lib().geoadv_query_ball_point(1, 8, 8, radius, 8, xyz.data_ptr(), xyz.data_ptr(), idx.data_ptr(), cnt.data_ptr(),
                                                _lib.stream_handle())
    _lib.check(st, "query_ball_point")
    got_cnt = cnt.cpu().numpy()
    assert got_cnt.min() >= 1 and got_cnt.max() <= 8 and 8 < got_cnt.sum() < 64
    op_idx, op_cnt = ops.query_ball_point(radius, 8, xyz, xyz)
    assert np.array_equal(op_cnt.cpu().numpy(), got_cnt) and np.array_equal(op_idx.cpu().numpy(), idx.cpu().numpy())


def test_long_long_and_size_t_train_gemm():
    from geometric_adv_amd import _lib, ops
    rng = np.random.default_rng(4)
    M_, N, K, batch = 8, 8, 8, 2
    sA, sB, ldc, sC = 80, 72, 9, 96                       # batch strides larger than the matrices, rows of C padded
    a = torch.from_numpy(rng.standard_normal(batch * sA).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rng.standard_normal(batch * sB).astype(np.float32)).to(DEV)
    got, want = (torch.full((batch * sC,), 7.0, dtype=torch.float32, device=DEV) for _ in range(2))
    L = _lib.lib()
    with torch.cuda.device(DEV):
        nf = L.geoadv_train_gemm_partial_floats()
        part = torch.empty(nf, dtype=torch.float32, device=DEV)
        st = L.geoadv_train_gemm(ops.TRAIN_GEMM_SPLITK, a.data_ptr(), K, 1, sA, b.data_ptr(), N, 1, sB, got.data_ptr(), ldc, sC, None, 0,
                                 M_, N, K, batch, part.data_ptr(), nf, None, _lib.stream_handle())
    _lib.check(st, "train_gemm")
    ops.train_gemm(ops.TRAIN_GEMM_SPLITK, a, (K, 1, sA), b, (N, 1, sB), want, (ldc, sC), None, 0, M_, N, K, batch=batch)
    g = got.cpu().numpy()
    assert np.array_equal(g.view(np.int32), want.cpu().numpy().view(np.int32))
    ref = np.stack([a.cpu().numpy()[z * sA:z * sA + M_ * K].reshape(M_, K).astype(np.float64) @
                    b.cpu().numpy()[z * sB:z * sB + K * N].reshape(K, N) for z in range(batch)])
    for z in range(batch):
        rows = g[z * sC:z * sC + M_ * ldc].reshape(M_, ldc)
        # the strides arrived whole, so these are the right elements: K fp32 products and sums, each rounded to 2^-24 relative
        bound = K * 2.0 ** -23 * (np.abs(a.cpu().numpy()[z * sA:z * sA + M_ * K].reshape(M_, K).astype(np.float64)) @
                                  np.abs(b.cpu().numpy()[z * sB:z * sB + K * N].reshape(K, N)))
        assert (np.abs(rows[:, :N] - ref[z]) <= bound).all()
        assert (rows[:, N:] == 7.0).all()


def test_an_argument_too_few_raises_before_c():
    import ctypes
    from geometric_adv_amd import _lib
    pc = _cloud(5, 1, 4)
    out = torch.full_like(pc, 9.0)
    with torch.cuda.device(DEV):
        with pytest.raises(TypeError):
            _lib.lib().geoadv_rotate_y(1, 4, pc.data_ptr(), 0.5, 0.5, out.data_ptr())              # no stream
        with pytest.raises(ctypes.ArgumentError):
            _lib.lib().geoadv_rotate_y(1, 4, pc.data_ptr(), ctypes.c_float(0.5), 0.5, out.data_ptr(), _lib.stream_handle())
        torch.cuda.synchronize()
    assert (out.cpu().numpy() == 9.0).all()                                   # nothing was launched
