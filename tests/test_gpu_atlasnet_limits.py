"""GPU: the AtlasNet forward (csrc/atlasnet.hip) across its chunk boundaries (64 clouds per chunk at 128 primitives, 327
at 25), at the ends of its accepted sizes (n 1 ... 16384, primitive counts whose points per primitive are 1225, 484, 324
and 16) and on the padded and degenerate clouds the defenses hand on, against the float64 model of
tests/_atlas_model64.py.  Tolerance, error metric, models and helpers are those of test_gpu_atlasnet.py.

Every call here goes through the C ABI with caller-made outputs: one guard cloud before and one after the range the call
may write, filled with a sentinel bit pattern (a NaN).  After the call the guards still hold the sentinel and no element
in range does.

Worst errors measured on the MI355X against float64 (the tests print each): across the chunk boundaries latent 3.6e-7,
recon 1.3e-6; n 1 ... 16384 latent 7.9e-6, recon 1.4e-5; 2 ... 128 primitives latent 7.2e-6, recon 1.8e-5 (5 primitives,
num_layers 0, batch norm), 1.7e-5 without decoder batch norm; coincident points 1.6e-6.
"""
import numpy as np
import pytest

import _atlas_model64 as M
from test_gpu_atlasnet import TOL, _ae, _clouds, _err, _model

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5A5A5               # int32; as a float a NaN
PIECE = 7                           # split-invariance: pieces of 7 clouds (64 and 327 are no multiples of 7)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _chunk(nb):
    return min(1024, 8192 // nb)    # atlasnet.hip: atlas_chunk, for a batch above it


def _forward(ae, x, latent=True):
    """geoadv_atlas_forward on the device tensor x (b, n, 3) into guarded outputs; {name: float32 device tensor} of the
    in-range parts, after the guard checks."""
    import torch
    from geometric_adv_amd import _lib
    lib = _lib.lib()
    b, n = int(x.shape[0]), int(x.shape[1])
    bufs = {"recon": torch.full((b + 2, ae.num_points, 3), SENTINEL, dtype=torch.int32, device="cuda:0")}
    if latent:
        bufs["latent"] = torch.full((b + 2, 1024), SENTINEL, dtype=torch.int32, device="cuda:0")
    ws = torch.empty(int(lib.geoadv_atlas_workspace_bytes(ae.handle, b, n)), dtype=torch.uint8, device="cuda:0")
    st = lib.geoadv_atlas_forward(ae.handle, b, n, _lib.ptr(x), _lib.ptr(bufs["latent"][1:]) if latent else None,
                                  _lib.ptr(bufs["recon"][1:]), _lib.ptr(ws), _lib.stream_handle())
    _lib.check(st, "atlas_forward")
    torch.cuda.synchronize()
    out = {}
    for k, buf in bufs.items():
        assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), "%s: a guard cloud was written" % k
        assert not bool((buf[1:-1] == SENTINEL).any()), "%s: an element in range was never written" % k
        out[k] = buf[1:-1].view(torch.float32)
    return out


def _sample(b, chunk, seed):
    """Clouds to compare with float64: the first, those around every chunk boundary, the first and last of the last chunk,
    a dozen random ones -- and, for each of these, the clouds a whole number of chunks before it, which a launcher that
    dropped or misapplied a chunk offset would have read or written instead."""
    s = {0, b - 1, (b - 1) // chunk * chunk}
    for k in range(chunk, b + chunk, chunk):
        s.update((k - 1, k, k + 1))
    s.update(int(v) for v in np.random.default_rng(seed).integers(0, b, 12))
    s = {c for c in s if 0 <= c < b}
    for c in list(s):
        s.update(range(c % chunk, c, chunk))
    return np.array(sorted(s))


def _separation(ref):
    """Smallest distance, in the tests' error metric, between the float64 outputs of two distinct sampled clouds."""
    flat = ref.reshape(len(ref), -1)
    d = np.array([[np.abs(p - q).max() for q in flat] for p in flat])
    d[np.diag_indices(len(d))] = np.inf
    return d.min() / max(1.0, np.abs(ref).max())


def _boxed_clouds(seed, b, n):
    """b clouds of n points, each uniform in a box of its own (centre within 0.3 of the origin, half side 0.05 ... 0.2)
    inside the unit cube: clouds that differ far more than two draws from the same cube do."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-0.3, 0.3, (b, 1, 3))
    half = rng.uniform(0.05, 0.2, (b, 1, 1))
    return (centre + half * (2 * rng.random((b, n, 3)) - 1)).astype(np.float32)


BOUNDARY = [(nb, n, f(_chunk(nb))) for nb, n in ((128, 40), (25, 70))
            for f in (lambda c: c - 1, lambda c: c, lambda c: c + 1, lambda c: 2 * c + 3)]


@pytest.mark.parametrize("nb,n,b", BOUNDARY)
def test_chunk_boundary(nb, n, b):
    """One call over b clouds (no second chunk, a full chunk, a second chunk of one cloud, three chunks with a short last
    one) at 128 primitives (chunk 64) and 25 (chunk 327), num_layers 0, decoder batch norm.

    1. latent and recon equal, bit for bit, the same clouds run 7 at a time (whose column slices and decoder tiles differ
       from the call's: the launch shape must not show);
    2. the sampled clouds (_sample) equal the float64 model within TOL;
    3. in float64 any two sampled clouds -- each boundary cloud and its counterparts one and two chunks earlier among
       them -- differ by more than 100 x TOL in the latent and in the reconstruction (_boxed_clouds; on the CPU the
       smallest distances over the eight cases are 5.0e-2 and 3.0e-2), so a neighbour's or another chunk's result cannot pass 2;
    4. the guards (_forward).  Without the latent output (the launcher then keeps it in scratch) the reconstruction is the
       same."""
    import torch
    chunk = _chunk(nb)
    ae = _ae(nb, 0, True)
    x = _boxed_clouds(10 * nb + b, b, n)
    xd = _dev(x)
    out = _forward(ae, xd)
    assert out["recon"].shape == (b, ae.num_points, 3)
    for s in range(0, b, PIECE):
        piece = _forward(ae, xd[s:s + PIECE])
        for k, v in piece.items():
            assert torch.equal(v, out[k][s:s + PIECE]), "%s differs from the run in pieces at clouds %d..." % (k, s)
    assert torch.equal(_forward(ae, xd, latent=False)["recon"], out["recon"])
    idx = _sample(b, chunk, b)
    _, state, tmpl = _model(nb, 0, True)
    z64, r64 = M.model(state, x[idx], tmpl, 0)
    sep = (_separation(z64), _separation(r64))
    print("nb %d b %d: %d sampled clouds, separation latent %.2e recon %.2e" % ((nb, b, len(idx)) + sep))
    assert min(sep) > 100 * TOL
    sel = torch.from_numpy(idx).to("cuda:0")
    e = (_err(out["latent"][sel].cpu().numpy(), z64), _err(out["recon"][sel].cpu().numpy(), r64))
    print("nb %d b %d: relative errors latent %.2e recon %.2e" % ((nb, b) + e))
    assert max(e) <= TOL


# ------------------------------------------------------------------------------------------------ size limits
@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 16383, 16384])
def test_point_count_limits_vs_float64(n, b):
    ae = _ae(25, 2, True)
    _, state, tmpl = _model(25, 2, True)
    x = _clouds(5000 + n, b, n)
    out = {k: v.cpu().numpy() for k, v in _forward(ae, _dev(x)).items()}
    z64, r64 = M.model(state, x, tmpl, 2)
    e = (_err(out["latent"], z64), _err(out["recon"], r64))
    print("n %d b %d: relative errors latent %.2e recon %.2e" % ((n, b) + e))
    assert out["recon"].shape == (b, 2500, 3)
    assert max(e) <= TOL


@pytest.mark.parametrize("dbn", [True, False])
@pytest.mark.parametrize("nl", [0, 4])
@pytest.mark.parametrize("nb", [2, 5, 7, 128])
def test_primitive_count_limits_vs_float64(nb, nl, dbn):
    """Points per primitive 35 x 35, 22 x 22, 18 x 18 and 4 x 4: decoder tiles that straddle clouds and primitives whose
    rows fill no tile (16 < 64)."""
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlasnet import AtlasNetAE
    g = AW.grain(2500, nb)
    assert g == {2: 35, 5: 22, 7: 18, 128: 4}[nb]
    opt, state = AW.synthetic_state(nb, nl, dbn, seed=nb)
    tmpl = AW.template(nb, g)
    ae = AtlasNetAE(options=opt, state=state)
    x = _clouds(6000 + nb, 3, 500)
    out = {k: v.cpu().numpy() for k, v in _forward(ae, _dev(x)).items()}
    assert out["recon"].shape == (3, nb * g * g, 3) and ae.num_points == nb * g * g
    z64, r64 = M.model(state, x, tmpl, nl)
    e = (_err(out["latent"], z64), _err(out["recon"], r64))
    print("nb %d nl %d bn %d: relative errors latent %.2e recon %.2e" % ((nb, nl, dbn) + e))
    assert max(e) <= TOL


# ------------------------------------------------------------------------------------------------ padded, degenerate
@pytest.mark.parametrize("n0,n", [(2011, 2048), (64, 2048), (1, 2048), (63, 64)])
def test_padding_with_the_last_point_changes_no_bit(n0, n):
    """What defend_surface / defend_critical hand on: n0 distinct points padded to n by repeating the last one (inside a
    tile, across a tile edge, across many tiles) give the bits of the n0-point cloud alone."""
    import torch
    ae = _ae(25, 2, True)
    x = _clouds(7000 + n0, 3, n0)
    padded = np.concatenate([x, np.repeat(x[:, -1:], n - n0, axis=1)], axis=1)
    assert padded.shape == (3, n, 3)
    a = _forward(ae, _dev(x))
    b = _forward(ae, _dev(padded))
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n", [1, 100, 2048])
def test_coincident_points_vs_float64(n):
    ae = _ae(25, 2, True)
    _, state, tmpl = _model(25, 2, True)
    x = np.repeat(_clouds(8000, 4, 1), n, axis=1)
    out = {k: v.cpu().numpy() for k, v in _forward(ae, _dev(x)).items()}
    assert np.isfinite(out["latent"]).all() and np.isfinite(out["recon"]).all()
    z64, r64 = M.model(state, x, tmpl, 2)
    e = (_err(out["latent"], z64), _err(out["recon"], r64))
    print("coincident n %d: relative errors latent %.2e recon %.2e" % ((n,) + e))
    assert max(e) <= TOL
