"""GPU: AtlasNet's data side on the device -- geoadv_normalize_clouds and geoadv_augment_batch (csrc/dataset.hip) through the C
interface, ops.normalize_clouds / ops.augment_batch, device_data.CloudAugmenter and train_atlasnet's device path.

References: the float64 models of tests/_cloud_draws64.py (normalize64; apply = the fp32 operators one after the other in
float64) and the reference's own recorded results (tests/golden/atlas_augment.npz).
Tolerances.  Against the float64 model: one fp32 ulp of the value plus 1e-12 * max|result of the cloud| -- the device
evaluates in float64 and rounds once, so the rounding is the first term and the reassociation of float64 sums and products
(a few 1e-16 of the largest value) the second, with four orders to spare.  Against the reference's fp32 results:
8 * 2^-24 * max|result of the cloud| (test_cloud_prepare_host.py: 2.9 measured between the reference and the model).
Drawn operators: scale, flip, translation and the sampled indices bit-equal to the restatement (integers and fp32 operations
rounded one by one); rotation entries within one fp32 ulp plus 2^-50 (float64 transcendentals whose last bit may differ
between libraries, rounded once; the absolute term covers entries next to zero, where an fp32 ulp is below float64's own
resolution of an O(1) cosine)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cloud_draws64 as D  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
INDEX = [6, 0, 6, 3, 1]
EINVAL = 1
BOUND_UNITS = 8
ALL_ON = dict(rot_axes=7, rot_3d=1, scale=1, flip_axes=5, translate=1)
SAMPLE_KEYS = ((0, 0), (7, 3), (2019, 11))          # test_cloud_prepare_host.py checks the uniformity for these


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "atlas_augment.npz")))


def _clouds(seed, b, n):
    """Anisotropic, off-centre clouds: the centre and the factor both matter."""
    rng = np.random.default_rng(seed)
    return ((rng.random((b, n, 3)) - 0.5) * np.array([1.0, 0.6, 0.3]) + np.array([0.2, -0.1, 0.05])).astype(np.float32)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _guarded(count, offset, pad=64, fill=None):
    """A NaN-filled allocation of count + 2 pad floats; -> (tensor, pointer to element `offset`)."""
    import torch
    t = torch.full((count + 2 * pad,), float("nan"), dtype=torch.float32, device=DEV)
    if fill is not None:
        t[offset:offset + count] = _dev(fill.reshape(-1))
    return t, ctypes.c_void_p(t.data_ptr() + 4 * offset)


def _guards_intact(t, count, offset):
    import torch
    return bool(torch.isnan(t[:offset]).all() and torch.isnan(t[offset + count:]).all())


def _close_to_model(got, model):
    """Per cloud: |got - model| <= one fp32 ulp of the value + 1e-12 * max|model of the cloud|; NaN in the same places."""
    got, model = np.asarray(got, np.float64), np.asarray(model, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(model)):
        return False
    for c in range(len(model)):
        if np.isnan(model[c]).any():
            continue
        if not np.all(np.abs(got[c] - model[c]) <= D.ulp32(model[c]) + 1e-12 * np.abs(model[c]).max()):
            return False
    return True


def _within_units(got, want, units=BOUND_UNITS):
    return all(np.abs(got[c].astype(np.float64) - want[c]).max() <= units * 2.0 ** -24 * np.abs(want[c]).max() for c in range(len(want))
               if not np.isnan(want[c]).any())


def _config(**kw):
    from geometric_adv_amd.ops import CloudAugment
    return CloudAugment(**dict(CloudAugment.DEFAULTS, **kw))


def _raw(L, b, n_out, data_ptr, num_clouds, n_src, index, cfg, params, params_out_ptr, out_ptr):
    from geometric_adv_amd import _lib
    return L.geoadv_augment_batch(b, n_out, data_ptr, ctypes.c_longlong(num_clouds), n_src, _lib.ptr(index),
                                  ctypes.byref(cfg) if cfg is not None else None, _lib.ptr(params), params_out_ptr, out_ptr,
                                  _lib.stream_handle())


# ---- normalisation -----------------------------------------------------------------------------------------------------
NORM_SIZES = (1, 2, 63, 64, 65, 257, 2048, 30000)


@pytest.mark.parametrize("b", [1, 5])
@pytest.mark.parametrize("kind", ["Identity", "UnitBall", "BoundingBox"])
def test_normalize_matches_the_float64_model_and_repeats_bit_for_bit(kind, b):
    from geometric_adv_amd import ops
    for n in NORM_SIZES:
        x = _clouds(100 + n, b, n)
        dev = _dev(x)
        got = ops.normalize_clouds(dev, kind).cpu().numpy()
        again = ops.normalize_clouds(dev, kind).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(again)), "n=%d: two runs differ" % n
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(x))                     # the input is left alone
        if kind == "Identity":
            assert np.array_equal(_bits(got), _bits(x))
            continue
        model = np.stack([D.normalize64(x[c], kind) for c in range(b)])
        assert np.isnan(model).all() == (n == 1)                                       # one point: 0 * 1/0
        assert _close_to_model(got, model), "n=%d" % n
        if n > 1 and kind == "UnitBall":
            assert abs(np.linalg.norm(got.astype(np.float64), axis=2).max(axis=1) - 1).max() < 1e-6
        if n > 1 and kind == "BoundingBox":
            assert np.abs(np.abs(got).max(axis=(1, 2)) - 1).max() < 1e-6


def test_normalize_identity_strides_over_more_clouds_than_the_grid():
    from geometric_adv_amd import ops
    b = 65536 + 3
    x = np.random.default_rng(3).standard_normal((b, 1, 3)).astype(np.float32)
    assert np.array_equal(_bits(ops.normalize_clouds(_dev(x), "Identity").cpu().numpy()), _bits(x))
    # the same stride with arithmetic: two points per cloud, every cloud against the model
    x2 = _clouds(4, b, 2)
    got = ops.normalize_clouds(_dev(x2), "BoundingBox").cpu().numpy().astype(np.float64)
    lo, hi = x2.astype(np.float64).min(axis=1, keepdims=True), x2.astype(np.float64).max(axis=1, keepdims=True)
    model = (x2 - (lo + hi) / 2) / ((hi - lo) / 2).max(axis=2, keepdims=True)
    assert np.all(np.abs(got - model) <= D.ulp32(model) + 1e-12)


@pytest.mark.parametrize("kind", ["UnitBall", "BoundingBox"])
def test_normalize_degenerate_clouds_come_out_nan_beside_an_untouched_neighbour(kind):
    from geometric_adv_amd import ops
    for n in (1, 7, 300):
        x = _clouds(n, 4, n)
        x[1] = x[1, 0]                               # every point the same
        x[2, n // 2, 1] = np.nan                     # one NaN coordinate
        got = ops.normalize_clouds(_dev(x), kind).cpu().numpy()
        assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
        for c in (0, 3):
            alone = ops.normalize_clouds(_dev(x[c:c + 1]), kind).cpu().numpy()
            assert np.array_equal(_bits(got[c]), _bits(alone[0]))
            assert np.isnan(got[c]).all() == (n == 1)
        assert _close_to_model(got, np.stack([D.normalize64(x[c], kind) for c in range(4)]))


@pytest.mark.parametrize("kind", ["UnitBall", "BoundingBox"])
def test_normalize_reproduces_the_references_recorded_results(golden, kind):
    from geometric_adv_amd import ops
    for n in (1, 7, 64):
        x, want = golden["norm__%s__n%d__in" % (kind, n)], golden["norm__%s__n%d__out" % (kind, n)]
        got = ops.normalize_clouds(_dev(x), kind).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want))
        assert _within_units(got, want.astype(np.float64))
        assert _close_to_model(got, np.stack([D.normalize64(x[c], kind) for c in range(len(x))]))


def test_normalize_refusals():
    import torch
    from geometric_adv_amd import _lib, ops
    L = _lib.lib()
    x = _dev(_clouds(0, 2, 8))
    assert L.geoadv_normalize_clouds(2, 8, 1, _lib.ptr(x), _lib.ptr(x), _lib.stream_handle()) == EINVAL
    assert b"in place" in L.geoadv_last_error()
    shifted = ctypes.c_void_p(x.data_ptr() + 12)                        # overlapping, not equal
    assert L.geoadv_normalize_clouds(1, 8, 1, _lib.ptr(x), shifted, _lib.stream_handle()) == EINVAL
    assert L.geoadv_normalize_clouds(2, 8, 3, _lib.ptr(x), _lib.ptr(torch.empty_like(x)), _lib.stream_handle()) == EINVAL
    assert L.geoadv_normalize_clouds(1, (1 << 20) + 1, 1, _lib.ptr(x), _lib.ptr(torch.empty_like(x)), _lib.stream_handle()) == EINVAL
    with pytest.raises(ValueError, match="bad dimensions"):
        ops.normalize_clouds(torch.zeros((2, 0, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.normalize_clouds(torch.zeros((0, 8, 3), device=DEV))
    with pytest.raises(ValueError, match="3d"):
        ops.normalize_clouds(torch.zeros((2, 8, 2), device=DEV))
    with pytest.raises(ValueError, match="normalization"):
        ops.normalize_clouds(x, "unitball")


# ---- the augmented batch: explicit operators -----------------------------------------------------------------------------
def test_explicit_operators_reproduce_the_reference_each_alone_and_all_together(golden):
    """The reference's own fp32 operators, given: the result is the reference's recorded one within the bound and the float64
    model's within an ulp.  The `all` cases pin the order (test_cloud_prepare_host.py shows that another order misses by
    thousands of units)."""
    from geometric_adv_amd import ops
    seen = 0
    for name in golden["cases"]:
        cfg = dict(zip(("rot_axes", "rot_3d", "scale", "flip_axes", "translate"), (int(v) for v in golden["aug__%s__cfg" % name])))
        for key in sorted(k for k in golden if k.startswith("aug__%s__n" % name) and k.endswith("__in")):
            x, rec, want = golden[key], golden[key[:-2] + "rec"], golden[key[:-2] + "out"]
            got, rec_out = ops.augment_batch(_dev(x), None, cfg, params=rec, want_params=True)
            got = got.cpu().numpy()
            assert np.array_equal(_bits(rec_out.cpu().numpy()), _bits(rec)), key
            assert _within_units(got, want.astype(np.float64)), key
            assert _close_to_model(got, np.stack([D.apply(x[c], rec[c]) for c in range(len(x))])), key
            # a GPU tensor of operators, and a seed that must not matter when they are given
            again = ops.augment_batch(_dev(x), None, dict(cfg, seed=99, counter=5), params=_dev(rec)).cpu().numpy()
            assert np.array_equal(_bits(again), _bits(got))
            seen += 1
    assert seen == 10
    # an operator that the configuration leaves off is not applied, whatever the record holds
    x, rec = golden["aug__all__n7__in"], golden["aug__all__n7__rec"]
    got, rec_out = ops.augment_batch(_dev(x), None, dict(scale=1), params=rec, want_params=True)
    only_scale = np.stack([D.identity_record()] * 4)
    only_scale[:, D.SCALE:D.FLIP] = rec[:, D.SCALE:D.FLIP]
    assert np.array_equal(_bits(rec_out.cpu().numpy()), _bits(only_scale))
    assert _close_to_model(got.cpu().numpy(), np.stack([D.apply(x[c], only_scale[c]) for c in range(4)]))


# ---- the augmented batch: drawn operators ----------------------------------------------------------------------------------
def _check_records(got, want):
    for lo, hi in ((D.SCALE, D.FLIP), (D.FLIP, D.TRANS), (D.TRANS, D.RECORD)):
        assert np.array_equal(_bits(got[:, lo:hi]), _bits(want[:, lo:hi])), (lo, hi)
    rot_got, rot_want = got[:, :D.SCALE].astype(np.float64), want[:, :D.SCALE].astype(np.float64)
    assert np.all(np.abs(rot_got - rot_want) <= D.ulp32(rot_want) * (rot_want != 0) + 2.0 ** -50)
    assert np.array_equal(rot_got == 0, rot_want == 0) and np.array_equal(rot_got == 1, rot_want == 1)      # the structural zeros and ones


@pytest.mark.parametrize("seed,counter", [(0, 0), (2 ** 63 + 5, 2 ** 40 + 7)])
def test_drawn_operators_are_the_restatements(seed, counter):
    from geometric_adv_amd import ops
    data = _clouds(11, 7, 65)
    x = _dev(data)
    cfg = dict(ALL_ON, seed=seed, counter=counter)
    out, rec = ops.augment_batch(x, INDEX, cfg, want_params=True)
    out, rec = out.cpu().numpy(), rec.cpu().numpy()
    _check_records(rec, D.records(seed, counter, range(5), **ALL_ON))
    assert _close_to_model(out, np.stack([D.apply(data[INDEX[i]], rec[i]) for i in range(5)]))
    assert np.array_equal(_bits(ops.augment_batch(x, INDEX, cfg).cpu().numpy()), _bits(out))           # run to run, with and without the record
    # each operator alone, other ranges, and the operators that are off hold their identities
    for one in (dict(rot_axes=1), dict(rot_axes=2, range_rot=90.0), dict(rot_axes=4), dict(rot_axes=5), dict(rot_3d=1),
                dict(scale=1, scale_min=0.5, scale_max=0.5), dict(scale=1, scale_min=-2.0, scale_max=3.0), dict(flip_axes=2),
                dict(flip_axes=7), dict(translate=1, translate_scale=0.0), dict(translate=1, translate_scale=1.5)):
        o, r = ops.augment_batch(x, INDEX, dict(one, seed=seed, counter=counter), want_params=True)
        o, r = o.cpu().numpy(), r.cpu().numpy()
        _check_records(r, D.records(seed, counter, range(5), **one))
        assert _close_to_model(o, np.stack([D.apply(data[INDEX[i]], r[i]) for i in range(5)])), one
    # slot independence: rows 2.. of the full call, bit for bit, sampling included
    for n_out in (None, 100):
        full, full_rec = ops.augment_batch(x, INDEX, cfg, n_out=n_out, want_params=True)
        part, part_rec = ops.augment_batch(x, INDEX[2:], dict(cfg, slot_offset=2), n_out=n_out, want_params=True)
        assert np.array_equal(_bits(part.cpu().numpy()), _bits(full.cpu().numpy()[2:]))
        assert np.array_equal(_bits(part_rec.cpu().numpy()), _bits(full_rec.cpu().numpy()[2:]))
    # sampled, then augmented: the model on the source points the restatement names
    j = D.sample_indices(seed, counter, range(5), 100, 65)
    full, full_rec = full.cpu().numpy(), full_rec.cpu().numpy()
    assert np.array_equal(_bits(full_rec), _bits(rec))
    assert _close_to_model(full, np.stack([D.apply(data[INDEX[i]][j[i]], rec[i]) for i in range(5)]))
    # another counter or seed: other operators
    for other in (dict(cfg, counter=counter + 1), dict(cfg, seed=(seed + 1) % 2 ** 64)):
        r2 = ops.augment_batch(x, INDEX, other, want_params=True)[1].cpu().numpy()
        cosines = [4, 9, 18, D.ROT3D]            # an entry of each of the four matrices that is drawn
        assert np.mean(r2[:, cosines] == rec[:, cosines]) < 0.1 and np.mean(r2[:, D.SCALE:D.FLIP] == rec[:, D.SCALE:D.FLIP]) < 0.1
    # no operator: the bits of the gathered clouds, and identity records
    o, r = ops.augment_batch(x, INDEX, dict(seed=seed, counter=counter), want_params=True)
    assert np.array_equal(_bits(o.cpu().numpy()), _bits(data[INDEX])) and np.array_equal(r.cpu().numpy(), np.stack([D.identity_record()] * 5))
    assert np.array_equal(_bits(ops.augment_batch(x).cpu().numpy()), _bits(data))


@pytest.mark.parametrize("seed,counter", SAMPLE_KEYS)
def test_sampling_takes_the_source_points_the_restatement_names(seed, counter):
    from geometric_adv_amd import ops
    for n_src, n_out, clouds in ((30000, 2500, 3), (8, 4096, 7)):
        data = _clouds(n_src, clouds, n_src)
        data[0, 0, 0] = np.inf                                   # copied as bits, not multiplied by an identity
        index = [clouds - 1, 0, 0, 1]
        got = ops.augment_batch(_dev(data), index, dict(seed=seed, counter=counter, sample=1), n_out=n_out).cpu().numpy()
        j = D.sample_indices(seed, counter, range(4), n_out, n_src)
        want = np.stack([data[index[i]][j[i]] for i in range(4)])
        assert np.array_equal(_bits(got), _bits(want))
        if n_src == 8:
            counts = np.stack([np.bincount(j[i], minlength=8) for i in range(4)])
            assert np.abs(counts - 512).max() <= 128
    # n_out == n_src with sampling on still samples; with sampling off it is the cloud in order
    data = _clouds(5, 2, 64)
    got = ops.augment_batch(_dev(data), None, dict(seed=seed, counter=counter, sample=1)).cpu().numpy()
    j = D.sample_indices(seed, counter, range(2), 64, 64)
    assert np.array_equal(_bits(got), _bits(np.stack([data[i][j[i]] for i in range(2)]))) and not np.array_equal(_bits(got), _bits(data))


@pytest.mark.parametrize("n_out", [1, 3, 255, 257])
def test_ragged_sizes_and_a_bad_device_index_inside_guards(n_out):
    """Through the C interface, every buffer inside a NaN-filled allocation at an unaligned start.  Sampling n_out points out
    of 65 and, without sampling, clouds of n_out points; device index with two entries out of range: those slots of out and of
    params_out stay unwritten, the others are the good call's, no guard changes."""
    from geometric_adv_amd import _lib
    L = _lib.lib()
    index = _dev(np.array([6, 99, 0, -1, 3], np.int32))
    good = [0, 2, 4]
    for n_src, sample in ((65, 1), (n_out, 0)):
        data = _clouds(n_out, 7, n_src)
        cfg = _config(seed=3, counter=8, sample=sample, **ALL_ON)
        offset, count = 5, 5 * n_out * 3
        src, src_p = _guarded(data.size, offset, fill=data)
        out, out_p = _guarded(count, offset)
        rec, rec_p = _guarded(5 * D.RECORD, offset)
        _lib.check(_raw(L, 5, n_out, src_p, 7, n_src, index, cfg, None, rec_p, out_p), "augment_batch")
        assert _guards_intact(out, count, offset) and _guards_intact(rec, 5 * D.RECORD, offset) and _guards_intact(src, data.size, offset)
        got = out[offset:offset + count].cpu().numpy().reshape(5, n_out, 3)
        got_rec = rec[offset:offset + 5 * D.RECORD].cpu().numpy().reshape(5, D.RECORD)
        assert np.isnan(got[[1, 3]]).all() and np.isnan(got_rec[[1, 3]]).all()
        _check_records(got_rec[good], D.records(3, 8, good, **ALL_ON))
        j = D.sample_indices(3, 8, range(5), n_out, n_src) if sample else np.tile(np.arange(n_out), (5, 1))
        src_of = {0: 6, 2: 0, 4: 3}
        assert _close_to_model(got[good], np.stack([D.apply(data[src_of[i]][j[i]], got_rec[i]) for i in good]))
        # plain gather (cfg NULL) through the same guards
        out2, out2_p = _guarded(count, offset)
        if not sample:
            _lib.check(_raw(L, 5, n_out, src_p, 7, n_src, index, None, None, None, out2_p), "augment_batch")
            g2 = out2[offset:offset + count].cpu().numpy().reshape(5, n_out, 3)
            assert _guards_intact(out2, count, offset) and np.isnan(g2[[1, 3]]).all()
            assert np.array_equal(_bits(g2[good]), _bits(data[[6, 0, 3]]))


def test_augment_batch_refusals():
    import torch
    from geometric_adv_amd import _lib, ops
    L = _lib.lib()
    data = _clouds(0, 7, 16)
    x = _dev(data)
    out = torch.empty((5, 16, 3), dtype=torch.float32, device=DEV)
    idx = _dev(np.array(INDEX, np.int32))

    def status(cfg, n_out=16, out_ptr=None, rec_ptr=None):
        return _raw(L, 5, n_out, _lib.ptr(x), 7, 16, idx, cfg, None, rec_ptr, out_ptr if out_ptr is not None else _lib.ptr(out))

    assert status(_config(**ALL_ON)) == 0
    assert status(None, out_ptr=ctypes.c_void_p(x.data_ptr() + 16 * 3 * 4)) == EINVAL and b"overlaps" in L.geoadv_last_error()
    assert status(None, rec_ptr=_lib.ptr(out)) == EINVAL and b"overlaps" in L.geoadv_last_error()
    assert status(_config(scale=1, scale_min=1.5, scale_max=1.25)) == EINVAL and b"scale_min" in L.geoadv_last_error()
    assert status(_config(scale=1, scale_max=float("inf"))) == EINVAL
    assert status(_config(scale=1, scale_min=float("nan"))) == EINVAL
    for bad in (-0.01, float("inf"), float("nan")):
        assert status(_config(translate=1, translate_scale=bad)) == EINVAL and b"translate_scale" in L.geoadv_last_error()
    for bad in (0.0, -90.0, 360.5, float("nan")):
        assert status(_config(rot_axes=2, range_rot=bad)) == EINVAL and b"range_rot" in L.geoadv_last_error()
    assert status(_config(rot_axes=8)) == EINVAL and status(_config(flip_axes=-1)) == EINVAL
    assert status(_config(slot_offset=-1)) == EINVAL
    assert status(None, n_out=8) == EINVAL and b"without sampling" in L.geoadv_last_error()
    assert status(_config(**ALL_ON), n_out=8) == EINVAL
    assert status(_config(sample=1), n_out=8) == 0
    assert _raw(L, 0, 16, _lib.ptr(x), 7, 16, idx, None, None, None, _lib.ptr(out)) == EINVAL
    assert _raw(L, 5, 16, None, 7, 16, idx, None, None, None, _lib.ptr(out)) == EINVAL
    # ranges that are wrong but belong to an operator that is off are not looked at
    assert status(_config(range_rot=0.0, scale_min=2.0, scale_max=1.0, translate_scale=-1.0)) == 0
    # the Python side
    with pytest.raises(ValueError, match="scale_min"):
        ops.augment_batch(x, INDEX, dict(scale=1, scale_min=2.0, scale_max=1.0))
    with pytest.raises(ValueError, match="without sampling"):
        ops.augment_batch(x, INDEX, dict(sample=0), n_out=8)
    with pytest.raises(ValueError, match="unknown config fields"):
        ops.augment_batch(x, INDEX, dict(rotate_first=1))
    for bad in ([7], [-1], [0, 1, 2, 3, 99]):
        with pytest.raises(ValueError, match="out of range"):
            ops.augment_batch(x, bad)
    with pytest.raises(ValueError, match="one-dimensional"):
        ops.augment_batch(x, [[0, 1]])
    with pytest.raises(ValueError, match="params must be"):
        ops.augment_batch(x, INDEX, dict(scale=1), params=np.zeros((4, 45), np.float32))
    with pytest.raises(ValueError, match="3d"):
        ops.augment_batch(torch.zeros((2, 8, 2), device=DEV))


# ---- CloudAugmenter and the trainer's command -----------------------------------------------------------------------------
def test_cloud_augmenter_call_is_the_raw_op():
    from geometric_adv_amd import ops
    from geometric_adv_amd.device_data import CloudAugmenter
    data = _clouds(21, 7, 300)
    x = _dev(data)
    aug = CloudAugmenter(translation=True, rotation_axis=[1], rotation_3D=True, anisotropic_scaling=True, flips=[0, 2], seed=4)
    got = aug(x, INDEX, counter=17, slot_offset=3, sample_points=256).cpu().numpy()
    want = ops.augment_batch(x, INDEX, dict(seed=4, counter=17, slot_offset=3, sample=1, rot_axes=2, rot_3d=1, scale=1, flip_axes=5, translate=1),
                             n_out=256).cpu().numpy()
    assert got.shape == (5, 256, 3) and np.array_equal(_bits(got), _bits(want))
    got = aug(x, np.array(INDEX), counter=17).cpu().numpy()
    want = ops.augment_batch(x, INDEX, aug.fields(17)).cpu().numpy()
    assert got.shape == (5, 300, 3) and np.array_equal(_bits(got), _bits(want)) and not np.array_equal(_bits(got), _bits(data[INDEX]))
    assert np.array_equal(_bits(CloudAugmenter()(x, INDEX, counter=1).cpu().numpy()), _bits(data[INDEX]))


def _state(folder):
    import torch
    return torch.load(os.path.join(folder, "network.pth"), map_location="cpu", weights_only=True)


def test_train_atlasnet_on_the_device_path_is_reproducible_and_resumes_its_stream(tmp_path):
    """2 epochs on 5 clouds of 300 points (batches of 2, 2 and a dropped 1) with sampling, normalisation and three operators:
    finite statistics, a folder AtlasNetAE reads, the same network.pth from a second run and from a run interrupted after
    epoch 1 and resumed (the step counter continues the draws)."""
    import torch
    from geometric_adv_amd import train_atlasnet
    from geometric_adv_amd.atlasnet import AtlasNetAE
    top = str(tmp_path)
    np.save(os.path.join(top, "train.npy"), _clouds(10, 5, 300))
    np.save(os.path.join(top, "val.npy"), _clouds(11, 3, 300))
    base = ["--top_dir", top, "--train_pc_path", "train.npy", "--eval_pc_path", "val.npy", "--batch_size", "2", "--batch_size_test", "2",
            "--nb_primitives", "3", "--template_type", "SQUARE", "--num_layers", "1", "--number_points", "96", "--number_points_eval", "75",
            "--custom_data", "--no_metro", "--seed", "3", "--sample_points", "256", "--normalization", "UnitBall",
            "--data_augmentation_axis_rotation", "--anisotropic_scaling", "--random_translation"]
    assert train_atlasnet.main(base + ["--dir_name", "one", "--nepoch", "2"]) == 0
    folder = os.path.join(top, "one")
    lines = [json.loads(l[len("json_stats: "):]) for l in open(os.path.join(folder, "log.txt"))]
    assert [l["epoch"] for l in lines] == [1, 2]
    assert all(np.isfinite(l[k]) for l in lines for k in ("loss_train_total", "loss_val", "fscore"))
    opts = json.load(open(os.path.join(folder, "options.json")))
    assert opts["sample_points"] == 256 and opts["normalization"] == "UnitBall" and opts["anisotropic_scaling"] is True
    assert opts["random_rotation"] is False and opts["start_epoch"] == 2
    one = _state(folder)
    assert int(one["module.encoder.bn1.num_batches_tracked"]) == 4
    ae = AtlasNetAE(folder)
    assert np.isfinite(ae.get_reconstructions(_clouds(12, 2, 256))).all()
    # the same command in a fresh folder: the same bits
    assert train_atlasnet.main(base + ["--dir_name", "two", "--nepoch", "2"]) == 0
    two = _state(os.path.join(top, "two"))
    assert sorted(one) == sorted(two) and all(torch.equal(one[k], two[k]) for k in one)
    # interrupted after epoch 1, then resumed
    assert train_atlasnet.main(base + ["--dir_name", "three", "--nepoch", "1"]) == 0
    assert train_atlasnet.main(base + ["--dir_name", "three", "--nepoch", "2"]) == 0
    three = _state(os.path.join(top, "three"))
    assert all(torch.equal(one[k], three[k]) for k in one)
    lines3 = [json.loads(l[len("json_stats: "):]) for l in open(os.path.join(top, "three", "log.txt"))]
    assert lines3 == lines
