"""The generator and parameter formulas of geoadv_augment_batch (csrc/dataset.hip, file header) restated in numpy -- the same
64-bit integer arithmetic, the same fp32 roundings of scale and translation, float64 transcendentals rounded to fp32 once --
and the float64 models of the two operators: apply(x, record) applies a record's fp32 operators one after the other in
float64, normalize64(x, kind) is the normalisation of float64 statistics."""
import numpy as np

from _batch_noise64 import G, mix

RECORD = 45
AXIAL, ROT3D, SCALE, FLIP, TRANS = 0, 27, 36, 39, 42            # the record's layout (include/geoadv.h)
K_AXIAL, K_NORMAL, K_ANGLE, K_SCALE, K_FLIP, K_TRANS, K_SAMPLE = 16, 19, 22, 23, 26, 29, 32
DEFAULTS = dict(sample=0, rot_axes=0, range_rot=360.0, rot_3d=0, scale=0, scale_min=0.75, scale_max=1.25, flip_axes=0, translate=0,
                translate_scale=0.03)
F = np.float32


def identity_record():
    r = np.zeros(RECORD, F)
    r[[0, 4, 8, 9, 13, 17, 18, 22, 26, 27, 31, 35]] = 1
    r[SCALE:TRANS] = 1
    return r


def draw(seed, counter, slot, q, k):
    """r(q, k) of output slot `slot`: uint64, broadcast over slot / q / k."""
    with np.errstate(over="ignore"):
        base = mix(mix(np.uint64(seed) + G) ^ np.uint64(counter))
        key = mix(base ^ ((np.asarray(slot, np.uint64) << np.uint64(32)) | np.asarray(q, np.uint64)))
        return mix(key + np.asarray(k, np.uint64) * G)


def uniform(r):
    """24 bits in [0, 1): exact in fp32 and float64."""
    return (np.asarray(r, np.uint64) >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def normal(r):
    r = np.asarray(r, np.uint64)
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos((2.0 * np.pi) * u2)


def axial_matrix(axis, u, range_rot=360.0):
    """Operation.get_3D_rot_matrix(axis, u * 2K - K), K = pi * range_rot / 360: float64, rounded to fp32."""
    K = np.pi * float(F(range_rot)) / 360.0
    angle = u * (2.0 * K) - K
    c, s = np.cos(angle), np.sin(angle)
    i, j = [a for a in range(3) if a != axis]
    M = np.zeros((3, 3))
    M[axis, axis] = 1
    M[i, i] = M[j, j] = c
    M[i, j], M[j, i] = s, -s
    return M.astype(F)


def rotation_3d(g, u):
    """DataAugmentation.get_random_rotation_matrix (lines 276-302) of the Gaussian axis g[3] and the uniform u."""
    x = g / np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    angle = u * (2.0 * np.pi) + np.pi
    c, s = np.cos(angle), np.sin(angle)
    v = 1.0 - c
    M = np.zeros((3, 3))
    for a in range(3):
        M[a, a] = c + (x[a] * x[a]) * v
    M[0, 1] = (x[0] * x[1]) * v - x[2] * s
    M[1, 0] = (x[0] * x[1]) * v + x[2] * s
    M[0, 2] = (x[0] * x[2]) * v + x[1] * s
    M[2, 0] = (x[0] * x[2]) * v - x[1] * s
    M[1, 2] = (x[1] * x[2]) * v - x[0] * s
    M[2, 1] = (x[1] * x[2]) * v + x[0] * s
    return M.astype(F)


def scale_value(u, scale_min=0.75, scale_max=1.25):
    """u * (max - min) + min: three fp32 operations."""
    return F(F(F(u) * F(F(scale_max) - F(scale_min))) + F(scale_min))


def translation_value(u, translate_scale=0.03):
    """(u * 2) * scale - scale in fp32."""
    return F(F(F(F(u) * F(2)) * F(translate_scale)) - F(translate_scale))


def flip_value(r):
    return F(1.0) if int(r) >> 63 else F(-1.0)


def record(seed, counter, slot, **config):
    """The record the device draws for output slot `slot` under the configuration (fields of geoadv_cloud_augment)."""
    cfg = dict(DEFAULTS, **config)
    rec = identity_record()
    for a in range(3):
        if (cfg["rot_axes"] >> a) & 1:
            rec[AXIAL + 9 * a:AXIAL + 9 * a + 9] = axial_matrix(a, uniform(draw(seed, counter, slot, 0, K_AXIAL + a)), cfg["range_rot"]).ravel()
    if cfg["rot_3d"]:
        g = np.array([normal(draw(seed, counter, slot, 0, K_NORMAL + a)) for a in range(3)])
        rec[ROT3D:ROT3D + 9] = rotation_3d(g, uniform(draw(seed, counter, slot, 0, K_ANGLE))).ravel()
    for a in range(3):
        if cfg["scale"]:
            rec[SCALE + a] = scale_value(uniform(draw(seed, counter, slot, 0, K_SCALE + a)), cfg["scale_min"], cfg["scale_max"])
        if (cfg["flip_axes"] >> a) & 1:
            rec[FLIP + a] = flip_value(draw(seed, counter, slot, 0, K_FLIP + a))
        if cfg["translate"]:
            rec[TRANS + a] = translation_value(uniform(draw(seed, counter, slot, 0, K_TRANS + a)), cfg["translate_scale"])
    return rec


def records(seed, counter, slots, **config):
    return np.stack([record(seed, counter, s, **config) for s in slots])


def sample_indices(seed, counter, slots, n_out, n_src):
    """j(s, p) = ((r >> 32) * n_src) >> 32: int64 [len(slots), n_out]."""
    r = draw(seed, counter, np.asarray(slots, np.uint64)[:, None], np.arange(n_out, dtype=np.uint64)[None, :], K_SAMPLE)
    return (((r >> np.uint64(32)) * np.uint64(n_src)) >> np.uint64(32)).astype(np.int64)


def apply(x, rec, order=("axial0", "axial1", "axial2", "rot3d", "scale", "flip", "trans")):
    """x [n, 3] (any float type) under the fp32 operators of one record, applied one after the other in float64, in the
    Augmenter's order (or `order`, to show that the order matters) -> float64 [n, 3]."""
    y = np.asarray(x, np.float64)
    rec = np.asarray(rec, F).astype(np.float64)
    for name in order:
        if name.startswith("axial"):
            a = int(name[-1])
            y = y @ rec[AXIAL + 9 * a:AXIAL + 9 * a + 9].reshape(3, 3)
        elif name == "rot3d":
            y = y @ rec[ROT3D:ROT3D + 9].reshape(3, 3)
        elif name == "scale":
            y = y * rec[SCALE:SCALE + 3]
        elif name == "flip":
            y = y * rec[FLIP:FLIP + 3]
        else:
            y = y + rec[TRANS:TRANS + 3]
    return y


def normalize64(x, kind):
    """One cloud x [n, 3] -> float64 [n, 3]; NaN and 0 * inf propagate as IEEE has them."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        if kind == "Identity":
            return x
        if kind == "UnitBall":
            c = x.sum(axis=0) / x.shape[0]
            d = x - c
            far = np.max((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])      # np.max propagates NaN
            return d * (1.0 / np.sqrt(far))
        if kind == "BoundingBox":
            lo, hi = x.min(axis=0), x.max(axis=0)
            return (x - (lo + hi) / 2.0) * (1.0 / np.max((hi - lo) / 2.0))
    raise ValueError(kind)


def ulp32(v):
    """One fp32 unit in the last place of |v| (of the smallest normal below it)."""
    return np.spacing(np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126).astype(F)).astype(np.float64)
