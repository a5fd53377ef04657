"""CPU: AtlasNet's data side without a GPU -- the float64 models of tests/_cloud_draws64.py against the reference's recorded
results (tests/golden/atlas_augment.npz, written by tools/make_golden_atlas_augment.py from the reference's own
pointcloud_processor.py), the restated draws' properties, the sampling's uniformity for the seeds the GPU test uses, the new
train_atlasnet flags and CloudAugmenter's argument checks.

BOUND: the reference chains about a dozen fp32 roundings (three axial products, the 3-D product, scale, flip, translation)
that mostly do not add up; the largest distance from the float64 model measured while writing the fixture is 2.9 units of
2^-24 * max|result of the cloud| (2.4 for the augmentation), 8 leaves a margin of about three."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _cloud_draws64 as D  # noqa: E402

BOUND_UNITS = 8
SAMPLE_KEYS = ((0, 0), (7, 3), (2019, 11))       # (seed, counter) of the GPU test's sampling cases


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(HERE, "golden", "atlas_augment.npz")))


def aug_cases(golden):
    for name in golden["cases"]:
        for key in sorted(golden):
            if key.startswith("aug__%s__n" % name) and key.endswith("__in"):
                stem = key[:-2]
                yield str(name), golden["aug__%s__cfg" % name], golden[stem + "in"], golden[stem + "rec"], golden[stem + "out"]


def worst_units(model, got):
    """The largest |model - got| per cloud in units of 2^-24 * max|model of the cloud|."""
    return max(np.abs(model[c] - got[c]).max() / (2.0 ** -24 * np.abs(model[c]).max()) for c in range(len(got)) if not np.isnan(got[c]).any())


def test_golden_holds_every_operator_alone_and_all_together(golden):
    names = set(str(c) for c in golden["cases"])
    assert names == {"axial0", "axial1", "axial2", "rot3d", "scale", "flip", "trans", "all"}
    sizes = sorted(int(k.split("__n")[1].split("__")[0]) for k in golden if k.startswith("aug__all__n") and k.endswith("__in"))
    assert sizes == [1, 7, 64]
    assert all(v.shape[0] == 4 for k, v in golden.items() if k.endswith("__in"))


def test_float64_model_reproduces_the_references_augmentation(golden):
    n = 0
    for name, cfg, x, rec, want in aug_cases(golden):
        model = np.stack([D.apply(x[c], rec[c]) for c in range(len(x))])
        assert not np.isnan(want).any() and not np.isnan(model).any()
        assert worst_units(model, want) <= BOUND_UNITS, name
        n += 1
    assert n == 10


def test_the_order_of_the_operators_is_pinned_by_the_golden(golden):
    """Applied in another order the model misses the reference's result by far more than the bound: scale before the
    rotations, translation first, the 3-D rotation before the axial ones."""
    x, rec, want = (golden["aug__all__n64__" + k] for k in ("in", "rec", "out"))
    right = ("axial0", "axial1", "axial2", "rot3d", "scale", "flip", "trans")
    for order in (("scale",) + right[:4] + right[5:], ("trans",) + right[:6], ("rot3d", "axial0", "axial1", "axial2") + right[4:],
                  ("axial2", "axial1", "axial0") + right[3:]):
        assert sorted(order) == sorted(right)
        model = np.stack([D.apply(x[c], rec[c], order) for c in range(len(x))])
        assert worst_units(model, want) > 1000 * BOUND_UNITS, order


@pytest.mark.parametrize("kind", ["UnitBall", "BoundingBox"])
def test_float64_model_reproduces_the_references_normalisation(golden, kind):
    for n in (1, 7, 64):
        x, want = golden["norm__%s__n%d__in" % (kind, n)], golden["norm__%s__n%d__out" % (kind, n)]
        model = np.stack([D.normalize64(x[c], kind) for c in range(len(x))])
        assert np.array_equal(np.isnan(model), np.isnan(want))
        if n == 1:
            assert np.isnan(want).all()                 # one point: 0 * 1/0
        else:
            assert np.isnan(want[2:]).all() and not np.isnan(want[:2]).any()        # coincident points, one NaN coordinate
            assert worst_units(model, want) <= BOUND_UNITS


def test_restated_draws_are_uniform_rotations_flips():
    slots = np.arange(64)
    r = D.draw(5, 9, slots[:, None], 0, np.arange(16, 33)[None, :])
    u = D.uniform(r)
    assert u.min() >= 0.0 and u.max() < 1.0 and np.array_equal(u, u.astype(np.float32)) and 0.4 < u.mean() < 0.6
    assert len(np.unique(r)) == r.size                                              # every stream of every slot its own draw
    assert not np.array_equal(D.draw(5, 10, slots, 0, 16), r[:, 0]) and not np.array_equal(D.draw(6, 9, slots, 0, 16), r[:, 0])
    recs = D.records(5, 9, slots, rot_axes=7, rot_3d=1, scale=1, flip_axes=5, translate=1)
    assert recs.dtype == np.float32 and recs.shape == (64, D.RECORD)
    for k in range(4):
        R = recs[:, 9 * k:9 * k + 9].reshape(-1, 3, 3).astype(np.float64)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 4 * 2.0 ** -24
        assert np.abs(np.linalg.det(R) - 1.0).max() <= 8 * 2.0 ** -24           # det = +1: a rotation, not a reflection
        if k < 3:                                                                   # axial: the axis' row and column are the unit vector's
            assert np.all(R[:, k, :] == np.eye(3)[k]) and np.all(R[:, :, k] == np.eye(3)[k])
    scale, flip, trans = recs[:, D.SCALE:D.FLIP], recs[:, D.FLIP:D.TRANS], recs[:, D.TRANS:]
    assert scale.min() >= 0.75 and scale.max() <= 1.25 and scale.std() > 0.1
    assert np.all(flip[:, 1] == 1) and set(np.unique(flip[:, [0, 2]])) == {-1.0, 1.0}
    assert np.abs(trans).max() <= np.float32(0.03) and trans.std() > 0.01
    # range_rot narrows the axial angle: |sin| <= sin(K), K = pi * 90 / 360
    narrow = D.records(5, 9, slots, rot_axes=2, range_rot=90.0)[:, 9:18].reshape(-1, 3, 3)
    assert np.abs(narrow[:, 0, 2]).max() <= np.sin(np.pi / 4) + 1e-7 and narrow[:, 0, 0].min() >= np.cos(np.pi / 4) - 1e-7
    # an operator that is off holds its identity
    assert np.array_equal(D.record(5, 9, 3), D.identity_record())


@pytest.mark.parametrize("seed,counter", SAMPLE_KEYS)
def test_sampling_is_uniform_for_the_gpu_tests_seeds(seed, counter):
    """n_src = 8, n_out = 4096: every source index 512 +- 128 times (6 sigma, sigma = sqrt(4096 * 1/8 * 7/8) = 21.2), per slot."""
    j = D.sample_indices(seed, counter, range(4), 4096, 8)
    assert j.min() == 0 and j.max() == 7
    for s in range(4):
        counts = np.bincount(j[s], minlength=8)
        assert np.abs(counts - 512).max() <= 128, counts
    assert not np.array_equal(j[0], j[1])
    big = D.sample_indices(seed, counter, [0], 2500, 30000)
    assert big.min() >= 0 and big.max() < 30000 and big.max() > 29000 and len(np.unique(big)) > 2300


def test_new_cli_flags_parse_to_their_defaults():
    from geometric_adv_amd import train_atlasnet
    need = ["--train_pc_path", "a.npy", "--eval_pc_path", "b.npy"]
    f = train_atlasnet.build_parser().parse_args(need)
    assert (f.random_rotation, f.data_augmentation_axis_rotation, f.data_augmentation_random_flips, f.random_translation,
            f.anisotropic_scaling) == (False,) * 5
    assert f.normalization == "Identity" and f.sample_points == 0
    assert not train_atlasnet.augmenter_of(f).active
    f = train_atlasnet.build_parser().parse_args(need + ["--random_rotation", "--data_augmentation_axis_rotation", "--data_augmentation_random_flips",
                                                         "--random_translation", "--anisotropic_scaling", "--normalization", "BoundingBox",
                                                         "--sample_points", "2500", "--seed", "4"])
    assert (f.normalization, f.sample_points) == ("BoundingBox", 2500)
    aug = train_atlasnet.augmenter_of(f)
    assert aug.active and aug.fields(counter=12, slot_offset=8) == dict(seed=4, counter=12, slot_offset=8, rot_axes=2, rot_3d=1, scale=1,
                                                                         flip_axes=5, translate=1)
    with pytest.raises(SystemExit):
        train_atlasnet.build_parser().parse_args(need + ["--normalization", "Sphere"])
    assert "data augmentation" not in train_atlasnet.__doc__.split("Left out:")[1].split(".")[0]


def test_cloud_augmenter_rejects_bad_arguments():
    from geometric_adv_amd.device_data import CloudAugmenter
    assert not CloudAugmenter().active
    a = CloudAugmenter(rotation_axis=[2, 0], flips=(1,), seed=-1)
    assert a.active and a.rotation_axis == (0, 2) and a.fields(3)["rot_axes"] == 5 and a.fields(3)["flip_axes"] == 2
    assert a.fields(3)["seed"] == (1 << 64) - 1 and a.fields(-1)["counter"] == (1 << 64) - 1
    for bad in (dict(rotation_axis=[3]), dict(rotation_axis=[-1]), dict(flips=[0, 0]), dict(flips=[1.0]), dict(rotation_axis=[True]),
                dict(translation=1), dict(rotation_3D="yes"), dict(anisotropic_scaling=None)):
        with pytest.raises(ValueError):
            CloudAugmenter(**bad)
    with pytest.raises(TypeError):
        CloudAugmenter(rotation_axis=1)


def test_ops_refuse_before_any_launch():
    """What ops.normalize_clouds / ops.augment_batch refuse on the host, without a GPU."""
    import torch
    from geometric_adv_amd import ops
    with pytest.raises(ValueError, match="normalization"):
        ops.normalize_clouds(torch.zeros((1, 4, 3)), "Sphere")
    with pytest.raises(ValueError, match="GPU"):
        ops.normalize_clouds(torch.zeros((1, 4, 3)))
    with pytest.raises(ValueError, match="GPU"):
        ops.augment_batch(torch.zeros((1, 4, 3)))
    assert ops.AUGMENT_RECORD == D.RECORD


def test_python_mirror_of_the_augment_config_matches_the_header():
    """ops.CloudAugment has the fields of geoadv_cloud_augment in include/geoadv.h, in order and with its types, and the record
    length and the normalisation kinds are the header's."""
    import ctypes
    import re
    from geometric_adv_amd import ops
    text = open(os.path.join(os.path.dirname(HERE), "include", "geoadv.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = re.search(r"typedef\s+struct\s+geoadv_cloud_augment\s*\{(.*?)\}\s*geoadv_cloud_augment\s*;", text, flags=re.S).group(1)
    want = [(t, f.strip()) for t, names in re.findall(r"\b(unsigned long long|int|float)\s+([a-z0-9_, ]+);", body) for f in names.split(",")]
    ctype = {ctypes.c_ulonglong: "unsigned long long", ctypes.c_int: "int", ctypes.c_float: "float"}
    assert [(ctype[t], f) for f, t in ops.CloudAugment._fields_] == want and len(want) == 13
    defines = dict(re.findall(r"#define\s+(GEOADV_[A-Z_]+)\s+(\d+)", text))
    assert int(defines["GEOADV_AUGMENT_RECORD"]) == ops.AUGMENT_RECORD
    assert ops.NORMALIZATIONS == {"Identity": int(defines["GEOADV_NORMALIZE_IDENTITY"]), "UnitBall": int(defines["GEOADV_NORMALIZE_UNIT_BALL"]),
                                  "BoundingBox": int(defines["GEOADV_NORMALIZE_BOUNDING_BOX"])}
    assert set(ops.CloudAugment.DEFAULTS) <= {f for f, _ in ops.CloudAugment._fields_} and set(ops.CloudAugment.DEFAULTS) <= set(D.DEFAULTS)
    assert all(D.DEFAULTS[k] == v for k, v in ops.CloudAugment.DEFAULTS.items())
