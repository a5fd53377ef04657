"""GPU: ops.latent_dist_matrix (csrc/latent_dist.hip), the latent distance matrix of prepare_indices_for_attack, bit for bit
against scorer.latent_dist_mat_host -- the reference's numpy expression on row blocks -- at every d where numpy's summation
takes another path (below eight, whole groups of eight, a tail), at the tile edges (the tile is 64 x 64, the k chunk 64), on
subnormal, overflowing and non-finite rows, and against the matrix the reference's own script recorded
(tests/golden/prepare_indices.npz); its exact symmetry and zeros; its refusals."""
import functools
import os.path as osp

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = osp.join(osp.dirname(osp.abspath(__file__)), "golden")
DEV = "cuda:0"
DS = [1, 7, 8, 9, 100, 127, 128]
NS = [1, 2, 33, 65, 130]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rows(seed, n, d):
    """Rows at the scales 0.01, 1 and 30: pairs whose squares differ by up to seven orders of magnitude."""
    rng = np.random.default_rng(seed)
    scale = np.array([0.01, 1.0, 30.0], np.float32)[np.arange(n) % 3]
    return (rng.standard_normal((n, d)).astype(np.float32) * scale[:, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(n, d):
    from geometric_adv_amd.scorer import latent_dist_mat_host
    x = _rows(1000 * d + n, n, d)
    want = latent_dist_mat_host(x)
    want.setflags(write=False)
    return x, want


def _gpu(a, b=None):
    from geometric_adv_amd import ops
    out = ops.latent_dist_matrix(torch.from_numpy(a).to(DEV), None if b is None else torch.from_numpy(b).to(DEV))
    assert out.dtype == torch.float32 and out.is_cuda
    return out.cpu().numpy()


@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_bit_equal_to_the_host_form(n, d):
    x, want = _case(n, d)
    got = _gpu(x)
    assert got.shape == (n, n)
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("d", [5, 64, 65, 72, 128])
def test_rectangular_is_bit_equal_to_numpy(d):
    a, b = _rows(3, 37, d), _rows(4, 70, d)
    want = np.linalg.norm(b[None, :, :] - a[:, None, :], axis=-1)
    got = _gpu(a, b)
    assert got.shape == (37, 70)
    assert np.array_equal(_bits(got), _bits(want))
    # passing b = a explicitly is b = None
    assert np.array_equal(_bits(_gpu(a, a)), _bits(_gpu(a)))


@pytest.mark.parametrize("d", [7, 100, 128])
def test_symmetry_and_exact_zeros(d):
    x = _rows(9, 130, d).copy()
    x[77] = x[5]                                    # two deliberately equal rows
    got = _gpu(x)
    assert np.array_equal(_bits(got), _bits(got.T))
    diag = np.diagonal(got)
    assert np.array_equal(_bits(diag), np.zeros(130, np.uint32)) and not np.signbit(diag).any()
    assert _bits(got[5, 77]) == 0 and _bits(got[77, 5]) == 0
    off = got.copy()
    np.fill_diagonal(off, 1.0)
    off[5, 77] = off[77, 5] = 1.0
    assert (off > 0).all()


@pytest.mark.parametrize("d", [7, 9, 128])
@pytest.mark.parametrize("kind", ["subnormal", "overflow", "nonfinite"])
def test_numeric_edges_equal_numpy(kind, d):
    from geometric_adv_amd.scorer import latent_dist_mat_host
    x = _rows(21, 67, d)
    if kind == "subnormal":
        x = (x * np.float32(1e-21)).astype(np.float32)          # squares around 1e-42 .. 1e-38: subnormal or flushed to 0 by a wrong mode
    elif kind == "overflow":
        x = (x * np.float32(1e20)).astype(np.float32)           # squares overflow to inf
    else:
        x[3, 0] = np.inf
        x[66, d - 1] = np.nan
    with np.errstate(all="ignore"):
        want = latent_dist_mat_host(x)
    got = _gpu(x)
    if kind == "subnormal":
        assert ((want > 0) & (want < 1e-19)).any()              # sums below 2^-126: subnormal accumulators
    if kind == "overflow":
        assert np.isinf(want).any()
    if kind == "nonfinite":
        assert np.isnan(want[66]).all() and np.isnan(want[3, 3]) and np.isinf(want[3, 4])
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(_bits(got)[~np.isnan(want)], _bits(want)[~np.isnan(want)])


def test_the_golden_matrix_is_reproduced():
    g = np.load(osp.join(GOLDEN, "prepare_indices.npz"))
    got = _gpu(g["latent_vectors"])
    assert np.array_equal(_bits(got), _bits(g["latent_dist_mat"]))
    from geometric_adv_amd.scorer import get_latent_dist_mat, sort_dist_mat
    mat = get_latent_dist_mat(g["latent_vectors"], DEV)
    assert isinstance(mat, np.ndarray) and mat.dtype == np.float32 and np.array_equal(_bits(mat), _bits(g["latent_dist_mat"]))
    assert np.array_equal(sort_dist_mat(mat, g["slice_idx"]), g["latent_nn_idx"])


def test_argument_errors_and_empty_inputs():
    from geometric_adv_amd import _lib, ops
    z = lambda *shape, **kw: torch.zeros(shape, device=kw.pop("device", DEV), **kw)
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 129))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16), z(4, 17))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16), z(4, 16, dtype=torch.float16))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16, device="cpu"))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16), z(4, 16, device="cpu"))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 16, 1))
    with pytest.raises(ValueError):
        ops.latent_dist_matrix(z(4, 0))
    assert tuple(ops.latent_dist_matrix(z(0, 16)).shape) == (0, 0)
    assert tuple(ops.latent_dist_matrix(z(0, 16), z(5, 16)).shape) == (0, 5)
    assert tuple(ops.latent_dist_matrix(z(5, 16), z(0, 16)).shape) == (5, 0)
    # the C entry point refuses the same shapes by itself (GA_REQUIRE -> GEOADV_EINVAL = 1) and treats an empty side as a no-op
    a, out = z(4, 16), z(4, 4)
    call = lambda na, nb, d: _lib.lib().geoadv_latent_dist_matrix(na, nb, d, _lib.ptr(a), _lib.ptr(a), _lib.ptr(out), _lib.stream_handle())
    assert call(4, 4, 129) == 1 and call(4, 4, 0) == 1 and call(-1, 4, 16) == 1 and call(4, -1, 16) == 1
    assert call(0, 4, 16) == 0 and call(4, 0, 16) == 0
    torch.cuda.synchronize()
