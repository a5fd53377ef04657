"""Weights of the PointNet classifier (classifier/pointnet_cls.py, classifier/transform_nets.py): TF variable names,
loading from a V2 checkpoint (tf_checkpoint.py, no TensorFlow) or an .npz with the same names, canonicalisation to the
layer order of geoadv_cls_weights (include/geoadv.h), and a calibrated synthetic model for tests and measurements.

The variable names are DERIVED FROM THE GRAPH CODE, not read from a file TensorFlow wrote: no trained classifier
checkpoint was available when they were written down.  tf_util.conv2d / fully_connected create `<scope>/weights` and
`<scope>/biases`; batch_norm_template (tf_util.py:454-491) creates `<scope>/bn/beta` and `<scope>/bn/gamma` and keeps the
moving statistics as ExponentialMovingAverage shadows of the moments tensors, whose names repeat the scope:
`<scope>/bn/<scope>/bn/moments/Squeeze/ExponentialMovingAverage` (mean) and `.../Squeeze_1/ExponentialMovingAverage`
(variance).  `load` lists every missing name at once, so a real `model-150.ckpt` that differs shows where.
"""
import os

import numpy as np

# (scope, fan_in, fan_out, batch norm, stored weight shape) in the order of geoadv_cls_weights; fan_out None = num_classes
LAYERS = [
    ("transform_net1/tconv1", 3, 64, True, (1, 3, 1, 64)),
    ("transform_net1/tconv2", 64, 128, True, (1, 1, 64, 128)),
    ("transform_net1/tconv3", 128, 1024, True, (1, 1, 128, 1024)),
    ("transform_net1/tfc1", 1024, 512, True, (1024, 512)),
    ("transform_net1/tfc2", 512, 256, True, (512, 256)),
    ("transform_net1/transform_XYZ", 256, 9, False, (256, 9)),
    ("conv1", 3, 64, True, (1, 3, 1, 64)),
    ("conv2", 64, 64, True, (1, 1, 64, 64)),
    ("transform_net2/tconv1", 64, 64, True, (1, 1, 64, 64)),
    ("transform_net2/tconv2", 64, 128, True, (1, 1, 64, 128)),
    ("transform_net2/tconv3", 128, 1024, True, (1, 1, 128, 1024)),
    ("transform_net2/tfc1", 1024, 512, True, (1024, 512)),
    ("transform_net2/tfc2", 512, 256, True, (512, 256)),
    ("transform_net2/transform_feat", 256, 4096, False, (256, 4096)),
    ("conv3", 64, 64, True, (1, 1, 64, 64)),
    ("conv4", 64, 128, True, (1, 1, 64, 128)),
    ("conv5", 128, 1024, True, (1, 1, 128, 1024)),
    ("fc1", 1024, 512, True, (1024, 512)),
    ("fc2", 512, 256, True, (512, 256)),
    ("fc3", 256, None, False, (256, None)),
]
BN_EPS = 1e-3            # tf_util.batch_norm_template (the auto-encoder's is 1e-5)
DEFAULT_EPOCH = 150


def bn_names(scope):
    """{field: variable name} of the batch norm of layer `scope` (gamma, beta, moving mean, moving variance)."""
    ema = "%s/bn/%s/bn/moments/%s/ExponentialMovingAverage"
    return {"gamma": scope + "/bn/gamma", "beta": scope + "/bn/beta",
            "mean": ema % (scope, scope, "Squeeze"), "var": ema % (scope, scope, "Squeeze_1")}


def variable_names():
    """Every variable the inference graph restores."""
    out = []
    for scope, _, _, bn, _ in LAYERS:
        out += [scope + "/weights", scope + "/biases"]
        if bn:
            out += sorted(bn_names(scope).values())
    return out


def checkpoint_prefix(classifier_path, restore_epoch=DEFAULT_EPOCH):
    """<classifier_path>/model-%03d.ckpt (pointnet_classifier.py:17-22 formats epochs < 10 and < 100 by hand to the same)."""
    return os.path.join(classifier_path, "model-%03d.ckpt" % int(restore_epoch))


def save_npz(path, weights):
    np.savez(path, **{k.replace("/", "__"): np.asarray(v) for k, v in weights.items()})


def load(path_or_prefix, restore_epoch=None):
    """{name: array} of the classifier variables from an .npz (save_npz), a TF V2 checkpoint prefix
    ('<dir>/model-150.ckpt'), or a classifier directory plus restore_epoch.  Other variables of the file (Adam slots, the
    `batch` step counter) are ignored; a missing one raises KeyError naming every missing variable."""
    from . import tf_checkpoint
    wanted = set(variable_names())
    if restore_epoch is not None:
        path_or_prefix = checkpoint_prefix(path_or_prefix, restore_epoch)
    if path_or_prefix.endswith(".npz"):
        with np.load(path_or_prefix) as z:
            got = {k.replace("__", "/"): z[k] for k in z.files}
        got = {k: v for k, v in got.items() if k in wanted}
    elif os.path.exists(path_or_prefix + ".index"):
        got = tf_checkpoint.load_checkpoint(path_or_prefix, lambda n: n in wanted)
    else:
        raise FileNotFoundError("%s is neither an .npz nor a TF V2 checkpoint prefix" % path_or_prefix)
    missing = sorted(wanted - set(got))
    if missing:
        raise KeyError("classifier weights %s lack %d variable(s): %s" % (path_or_prefix, len(missing), ", ".join(missing)))
    return got


def num_classes_of(weights):
    return int(np.asarray(weights["fc3/weights"]).shape[-1])


def canonical(weights, num_classes=None):
    """Lists (w, b, gamma, beta, mean, var) of contiguous float32 arrays in LAYERS order, w as [fan_in, fan_out]; the BN
    entries of the three linear layers are None."""
    nc = num_classes_of(weights) if num_classes is None else int(num_classes)
    out = {k: [] for k in ("w", "b", "gamma", "beta", "mean", "var")}

    def get(name, shape):
        if name not in weights:
            raise KeyError("missing classifier variable %r" % name)
        a = np.asarray(weights[name], dtype=np.float32)
        if a.size != int(np.prod(shape)):
            raise ValueError("variable %r has shape %s, expected %s elements as %s" % (name, a.shape, int(np.prod(shape)), shape))
        return np.ascontiguousarray(a.reshape(shape))

    for scope, fi, fo, bn, _ in LAYERS:
        fo = nc if fo is None else fo
        out["w"].append(get(scope + "/weights", (fi, fo)))
        out["b"].append(get(scope + "/biases", (fo,)))
        names = bn_names(scope)
        for k in ("gamma", "beta", "mean", "var"):
            out[k].append(get(names[k], (fo,)) if bn else None)
    return out


def _bn_relu(a, w, scope, calibrate):
    names = bn_names(scope)
    if calibrate:
        flat = a.reshape(-1, a.shape[-1])
        w[names["mean"]] = flat.mean(axis=0)
        w[names["var"]] = flat.var(axis=0)
    g, b, m, v = (np.asarray(w[names[k]], np.float64) for k in ("gamma", "beta", "mean", "var"))
    inv = g / np.sqrt(v + BN_EPS)
    return np.maximum(a * inv + (b - m * inv), 0.0)


def forward64(weights, pc, calibrate=False):
    """float64 forward of the inference graph: pc (b, n, 3) -> logits (b, C).  calibrate=True first sets every batch
    norm's moving statistics to the batch statistics of its pre-BN output (layer by layer), so that output is N(0, 1)-like."""
    w = weights
    mat = lambda scope, fi: np.asarray(w[scope + "/weights"], np.float64).reshape(fi, -1)
    lin = lambda x, scope, fi: x @ mat(scope, fi) + np.asarray(w[scope + "/biases"], np.float64)
    layer = lambda x, scope, fi: _bn_relu(lin(x, scope, fi), w, scope, calibrate)

    def tnet(x, p, fi, last, k):
        h = layer(layer(layer(x, p + "/tconv1", fi), p + "/tconv2", 64), p + "/tconv3", 128).max(axis=1)
        h = layer(layer(h, p + "/tfc1", 1024), p + "/tfc2", 512)
        return (lin(h, p + "/" + last, 256) + np.eye(k).reshape(-1)).reshape(-1, k, k)

    x = np.asarray(pc, np.float64)
    t1 = tnet(x, "transform_net1", 3, "transform_XYZ", 3)
    h = layer(layer(x @ t1, "conv1", 3), "conv2", 64)
    t2 = tnet(h, "transform_net2", 64, "transform_feat", 64)
    h = layer(layer(layer(h @ t2, "conv3", 64), "conv4", 64), "conv5", 128).max(axis=1)
    h = layer(layer(h, "fc1", 1024), "fc2", 512)
    return lin(h, "fc3", 256)


def calibration_batch(clouds=16, points=256):
    """The fixed batch synthetic_weights calibrates on: uniform in the unit cube centred at the origin."""
    return np.random.default_rng(12345).random((clouds, points, 3)) - 0.5


def synthetic_weights(num_classes=13, seed=0):
    """A classifier with the reference's variable names and shapes whose every pre-BN output is about N(0, 1) on unit-cube
    clouds (moving statistics calibrated in float64 on calibration_batch()).  The two transform layers get NON-ZERO,
    non-symmetric weights: the reference's zero initialisation would make both T-Nets the identity and hide a transposed or
    missing transform."""
    rng = np.random.default_rng(seed)
    w = {}
    for scope, fi, fo, bn, shape in LAYERS:
        fo = num_classes if fo is None else fo
        shape = tuple(num_classes if s is None else s for s in shape)
        w[scope + "/weights"] = (rng.standard_normal((fi, fo)) * np.sqrt(2.0 / fi)).reshape(shape)
        w[scope + "/biases"] = rng.standard_normal(fo) * 0.1
        if bn:
            names = bn_names(scope)
            w[names["gamma"]] = rng.uniform(0.8, 1.2, fo)
            w[names["beta"]] = rng.uniform(-0.1, 0.3, fo)
            w[names["mean"]] = np.zeros(fo)
            w[names["var"]] = np.ones(fo)
    # transforms: T1 = I + O(0.3), T2 = I + O(0.05) per entry (about 0.4 of a feature's norm)
    w["transform_net1/transform_XYZ/weights"] = rng.standard_normal((256, 9)) * (0.3 / 16)
    w["transform_net1/transform_XYZ/biases"] = rng.standard_normal(9) * 0.1
    w["transform_net2/transform_feat/weights"] = rng.standard_normal((256, 4096)) * (0.05 / 16)
    w["transform_net2/transform_feat/biases"] = rng.standard_normal(4096) * 0.02
    forward64(w, calibration_batch(), calibrate=True)
    return {k: np.asarray(v, dtype=np.float32) for k, v in w.items()}


# ---- training (cls_trainer.py, train_classifier.py) --------------------------------------------------------------------------
STEP_NAME = "Variable"                     # train_classifier.py: batch = tf.Variable(0), the unnamed global step counter


def trainable_names():
    """The trainable variables (weights, biases, bn/gamma, bn/beta) in LAYERS order."""
    out = []
    for scope, _, _, bn, _ in LAYERS:
        out += [scope + "/weights", scope + "/biases"]
        if bn:
            out += [scope + "/bn/gamma", scope + "/bn/beta"]
    return out


def slot_names(optimizer="adam"):
    """Names of the optimizer's variables as the TF 1.13 optimizers create them: `<var>/Adam`, `<var>/Adam_1` and
    beta1_power / beta2_power (AdamOptimizer), or `<var>/Momentum` (MomentumOptimizer)."""
    if optimizer == "adam":
        return [v + s for v in trainable_names() for s in ("/Adam", "/Adam_1")] + ["beta1_power", "beta2_power"]
    if optimizer == "momentum":
        return [v + "/Momentum" for v in trainable_names()]
    raise ValueError("optimizer must be 'adam' or 'momentum', got %r" % (optimizer,))


def xavier_bound(scope, num_classes=13):
    """TF's xavier_initializer() bound sqrt(6 / (fan_in + fan_out)) with its fan rule: a conv kernel [kh, kw, Cin, Cout] has
    fan_in = kh * kw * Cin and fan_out = kh * kw * Cout (so conv1 / tconv1 [1, 3, 1, 64]: 3 and 192), a matrix its two sides."""
    shape = dict((s, sh) for s, _, _, _, sh in LAYERS)[scope]
    shape = tuple(num_classes if d is None else d for d in shape)
    if len(shape) == 4:
        fan_in, fan_out = shape[0] * shape[1] * shape[2], shape[0] * shape[1] * shape[3]
    else:
        fan_in, fan_out = shape
    return float(np.sqrt(6.0 / (fan_in + fan_out)))


def initial_weights(num_classes=13, seed=0):
    """The variables as tf.global_variables_initializer leaves them (pointnet_cls.py / transform_nets.py / tf_util.py):
    weights U(-b, b) with b = xavier_bound (numpy-seeded: TF's own draws are not reproducible), biases 0, gamma 1, beta 0,
    transform_XYZ / transform_feat weights and biases 0, moving-average shadows 0 (zero slots)."""
    rng = np.random.default_rng(seed)
    w = {}
    for scope, _, fo, bn, shape in LAYERS:
        fo = num_classes if fo is None else fo
        shape = tuple(num_classes if d is None else d for d in shape)
        if scope.endswith("transform_XYZ") or scope.endswith("transform_feat"):
            w[scope + "/weights"] = np.zeros(shape, np.float32)
        else:
            b = xavier_bound(scope, num_classes)
            w[scope + "/weights"] = rng.uniform(-b, b, shape).astype(np.float32)
        w[scope + "/biases"] = np.zeros(fo, np.float32)
        if bn:
            names = bn_names(scope)
            w[names["gamma"]] = np.ones(fo, np.float32)
            w[names["beta"]] = np.zeros(fo, np.float32)
            w[names["mean"]] = np.zeros(fo, np.float32)
            w[names["var"]] = np.zeros(fo, np.float32)
    return w
