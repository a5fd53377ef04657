"""GPU: the f16x2 encoder arithmetic on models whose channels sit far from their layer's typical magnitude.

f16x2 scales a layer's activations and its weights by ONE power of two each (csrc/ae.hip); a channel far below that scale gets
fp16 pieces that are subnormal and loses bits that fp32 keeps.  Two families of models move one channel, eight, or half a layer by
f = 2^k, k = +-4 ... +-24:
  activations  layer j's gamma and beta times f, the matching input rows of layer j + 1's weights divided by f: the same function
               in exact arithmetic and, bit for bit, in f32 and bf16x3 (powers of two commute with the batch-norm fold);
  weights      layer L's output column, bias and moving mean times f, its moving variance times f^2: the same function up to the
               batch norm's eps, so the float64 model is rebuilt from the modified weights.
Every arithmetic a model is served in is held, per latent element, to the bound csrc/encoder_x3.h states, in units of 2^-24 of the
last layer's chain (tests/_chain64.py); f16x2 also to 1.25 x the fp32 chain's error + 4 units on the same inputs; the critical
points equal float64's wherever the float64 maximum leads every other point by more than both errors can close.  A model outside
f16x2's window must get bf16x3 by default and a refusal for an explicit f16x2; inside it (|k| <= 8 here, the benchmark's model)
f16x2 stays the default."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, B = 1024, 6
KS = (-24, -20, -16, -12, -8, -4, 4, 8, 12, 16, 20, 24)
COUNTS = ("1", "8", "half")
WIDTH = (64, 128, 128, 256, 128)                # output channels of encoder layers 0..4
BOUND_UNITS = 16.0                              # csrc/encoder_x3.h: the latent's error bound in units of 2^-24 of the last chain


def _name(layer, var):
    return "autoencoder/encoder_conv_layer_%d%s" % (layer, var)


def _channels(width, count):
    if count == "1":
        return np.array([width // 3])
    if count == "8":
        return np.arange(8) * (width // 8) + 1
    return np.arange(0, width, 2)


def _scaled(w, key, idx, factor, axis=-1):
    """w[key] with the entries `idx` along `axis` times `factor` (a power of two: exact in float32)."""
    a = np.array(w[key], dtype=np.float64)
    sl = [slice(None)] * a.ndim
    sl[axis] = idx
    a[tuple(sl)] *= factor
    out = a.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), a), key
    return out


def _cloud():
    from conftest import cloud
    return cloud(97, B, N)


def served_models(w, k=0):
    """{arithmetic: PointNetAE} for every arithmetic the library serves this model in.  The default is f16x2 or bf16x3; when it is
    bf16x3 an explicit f16x2 must be refused with a message."""
    from geometric_adv_amd.autoencoder import PointNetAE
    default = PointNetAE(w, N)
    out = {a: PointNetAE(w, N, encoder_arith=a) for a in ("f32", "bf16x3")}
    if default.encoder_arith == "f16x2":
        out["f16x2"] = default
    else:
        assert default.encoder_arith == "bf16x3"
        with pytest.raises(ValueError, match="f16x2"):
            PointNetAE(w, N, encoder_arith="f16x2")
    if abs(k) <= 8:
        assert "f16x2" in out, "k = %d: f16x2 must stay the default inside its window" % k
    return out


def measure(w, pc, aes):
    """{arithmetic: (max error in units of 2^-24 of the pooled chain, latents, critical points)} and the float64 reference."""
    from geometric_adv_amd import weights as W
    from oracle.attack_model import AEModel
    from _chain64 import last_layer_chain, pooled, error_units
    canon = W.canonical(w, N)
    model = AEModel(canon, N, np.float64)
    z64, hs = model.encode(pc.astype(np.float64), keep=True)
    chain = last_layer_chain(canon, model, hs[3])
    got = {}
    for a, ae in aes.items():
        z, idx = (t.cpu().numpy() for t in ae.max_and_argmax(pc))
        got[a] = (float(error_units(z, z64, pooled(chain, hs[4])).max()), z, idx)
    return got, z64, hs[4], chain


def check_served(w, pc, aes):
    """The assertions every served arithmetic must meet; returns the max errors in units."""
    from geometric_adv_amd import _lib
    from _chain64 import U24, certain_argmax
    got, z64, h4, chain = measure(w, pc, aes)
    sc = np.abs(z64).max()
    sure, arg64 = certain_argmax(h4, BOUND_UNITS * U24 * chain)
    units = {a: g[0] for a, g in got.items()}
    for a, (u, z, idx) in got.items():
        assert u <= BOUND_UNITS, (a, units)
        np.testing.assert_allclose(z / sc, z64 / sc, atol=2e-6, err_msg=a)
        assert np.array_equal(idx[sure], arg64[sure]), a
        assert _lib.lib().geoadv_ae_status(aes[a].handle, _lib.stream_handle()) == 0
    if "f16x2" in units:
        assert units["f16x2"] <= 1.25 * units["f32"] + 4.0, units
    return units


def activation_family(w, layer, count, k):
    w = dict(w)
    f, ch = 2.0 ** k, _channels(WIDTH[layer], count)
    for var in ("_bnorm/gamma", "_bnorm/beta"):
        w[_name(layer, var)] = _scaled(w, _name(layer, var), ch, f)
    w[_name(layer + 1, "/W")] = _scaled(w, _name(layer + 1, "/W"), ch, 1.0 / f, axis=-2)
    return w


def weight_family(w, layer, count, k):
    w = dict(w)
    f, ch = 2.0 ** k, _channels(WIDTH[layer], count)
    for var, g in (("/W", f), ("/b", f), ("_bnorm/moving_mean", f), ("_bnorm/moving_variance", f * f)):
        w[_name(layer, var)] = _scaled(w, _name(layer, var), ch, g)
    return w


@pytest.fixture(scope="module")
def base():
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    from oracle.attack_model import AEModel
    w = W.randomized_weights(N, seed=3)
    pc = _cloud()
    exact = {}
    for a in ("f32", "bf16x3"):
        z, idx = PointNetAE(w, N, encoder_arith=a).max_and_argmax(pc)
        exact[a] = (z.cpu().numpy(), idx.cpu().numpy())
    z64 = AEModel(W.canonical(w, N), N, np.float64).encode(pc.astype(np.float64))
    return w, pc, exact, z64


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_activation_side_reparametrization(base, layer, count, k):
    from geometric_adv_amd import weights as W
    from oracle.attack_model import AEModel
    w0, pc, exact, z64_0 = base
    w = activation_family(w0, layer, count, k)
    z64 = AEModel(W.canonical(w, N), N, np.float64).encode(pc.astype(np.float64))
    assert np.abs(z64 - z64_0).max() <= 1e-12 * np.abs(z64_0).max()
    aes = served_models(w, k)
    for a in ("f32", "bf16x3"):                 # the construction itself: exact where the arithmetic scales exactly
        z, idx = (t.cpu().numpy() for t in aes[a].max_and_argmax(pc))
        assert np.array_equal(z, exact[a][0]) and np.array_equal(idx, exact[a][1]), a
    check_served(w, pc, aes)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("layer", [1, 2, 3, 4])
def test_weight_side_reparametrization(base, layer, count, k):
    w = weight_family(base[0], layer, count, k)
    check_served(w, base[1], served_models(w, k))


def _with_mantissa(shape, pattern, rng):
    """Weights of one magnitude in [2^-4, 2^-3) with the given 23-bit mantissa and random signs."""
    bits = np.full(shape, ((127 - 4) << 23) | pattern, dtype=np.uint32)
    bits |= (rng.random(shape) < 0.5).astype(np.uint32) << 31
    return bits.view(np.float32)


@pytest.mark.parametrize("pattern", [0x7FFFFF, 0x555555, 0xAAAAAA])
def test_weights_whose_mantissas_maximise_the_dropped_remainder(base, pattern):
    """All-ones and alternating mantissas leave the largest remainders below each fp16 piece; one magnitude per layer keeps every
    column at the layer's scale, so f16x2 is served and only the written bound speaks for it."""
    w = dict(base[0])
    rng = np.random.default_rng(pattern)
    for layer in (1, 2, 3, 4):
        w[_name(layer, "/W")] = _with_mantissa(np.shape(w[_name(layer, "/W")]), pattern, rng)
    aes = served_models(w)
    assert "f16x2" in aes
    check_served(w, base[1], aes)


def _calibrate_batch_norm(w, layer, pc):
    """Moving mean / variance of `layer` set to its pre-activations' own statistics on `pc` (float64 model): what training on such
    data would leave, so that the layers behind it see activations of the usual size."""
    from geometric_adv_amd import weights as W
    from oracle.attack_model import AEModel
    model = AEModel(W.canonical(w, N), N, np.float64)
    h = model.encode(pc.astype(np.float64), keep=True)[1][layer - 1] if layer else pc.astype(np.float64)
    a = (h @ model.W[layer] + model.b[layer]).reshape(-1, WIDTH[layer])
    w[_name(layer, "_bnorm/moving_mean")] = a.mean(axis=0).astype(np.float32)
    w[_name(layer, "_bnorm/moving_variance")] = a.var(axis=0).astype(np.float32)


def test_one_signed_weights_in_the_last_layer(base):
    """Layer 4 (K = 256) with non-negative weights on non-negative activations: no cancellation hides an error in the chain (and
    none in the batch norm either: its moving mean stays small against the sums, so the latent is of the chain's own size)."""
    w = dict(base[0])
    w[_name(4, "/W")] = np.abs(np.asarray(w[_name(4, "/W")], np.float32))
    aes = served_models(w)
    assert "f16x2" in aes
    check_served(w, base[1], aes)


@pytest.mark.parametrize("layer", [2, 4])
def test_row_magnitudes_spread_inside_each_chain(base, layer):
    """The input rows of one layer scaled by 2^-20 ... 2^9 (every output channel's chain holds all of them; the column's largest
    weights keep the column at the layer's scale): the small rows' fp16 pieces are subnormal, their share of the chain is not."""
    from conftest import cloud
    w = dict(base[0])
    key = _name(layer, "/W")
    K = WIDTH[layer - 1]
    e = np.random.default_rng(layer).permutation(np.round(np.linspace(-20, 9, K)).astype(int))
    a = np.array(w[key], dtype=np.float64)
    a *= (2.0 ** e)[:, None]
    w[key] = a.astype(np.float32)
    _calibrate_batch_norm(w, layer, cloud(98, 2, N))
    aes = served_models(w)
    assert "f16x2" in aes
    check_served(w, base[1], aes)


def test_identically_zero_channels_do_not_trip_the_guard(base):
    """gamma = beta = 0 (the channel is +0 for every input) and all-zero weight columns say nothing about a layer's spread: f16x2
    stays the default and accurate."""
    w = dict(base[0])
    ch = _channels(128, "8")
    for var in ("_bnorm/gamma", "_bnorm/beta"):
        w[_name(1, var)] = _scaled(w, _name(1, var), ch, 0.0)
    w[_name(3, "/W")] = _scaled(w, _name(3, "/W"), ch, 0.0)
    aes = served_models(w)
    assert "f16x2" in aes
    check_served(w, base[1], aes)


def test_f16x2_stays_the_default_inside_its_window():
    """The benchmark's model (bench.py: synthetic_weights(N, seed=7)), the tests' randomized model and its 64-wide bottleneck (run
    zero-padded to 128 channels) keep f16x2."""
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    for n in (2048, N):
        assert PointNetAE(W.synthetic_weights(n, seed=7), n).encoder_arith == "f16x2"
    assert PointNetAE(W.randomized_weights(N), N).encoder_arith == "f16x2"
    assert PointNetAE(W.randomized_weights(N, bneck=64), N).encoder_arith == "f16x2"
