"""Weights and options of the AtlasNet auto-encoder of the transfer experiment (transfer/atlasnet): state-dict key names
derived from the module structure, loading <transfer_ae_folder>/network.pth and options.json, the SQUARE template of
eval mode, conversion to the layout of geoadv_atlas_weights (include/geoadv.h), and a calibrated synthetic model for tests
and measurements.

Key names.  The reference saves `nn.DataParallel(EncoderDecoder).state_dict()` (trainer_abstract.py:62-67): prefix
`module.`, then `encoder.` (model_blocks.PointNet: conv1..conv3, lin1, lin2, bn1..bn5, in registration order) and
`decoder.decoder.<p>.` (model_blocks.Mapping2Dto3D per primitive: conv1, conv2, conv_list.<i>, last_conv, bn1, bn2,
bn_list.<i>).  Every BatchNorm1d carries weight, bias, running_mean, running_var and num_batches_tracked; the last is
ignored here.  With remove_all_batchNorms the reference replaces torch.nn.BatchNorm1d AFTER the encoder is built
(atlasnet.py:35-37 runs inside EncoderDecoder.__init__ after PointNet, model.py:21-23), so only the DECODER loses its batch
norms: which one a file holds is read from its keys.
"""
import json
import os

import numpy as np

BN_EPS = 1e-5
BOTTLENECK = 1024
HIDDEN = 512
MAX_PRIMITIVES = 128
MAX_LAYERS = 4
BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")

# auxiliary/argument_parser.py:177-303 (parser_transfer): the defaults options.json overrides, as far as inference uses them
DEFAULT_OPTIONS = {"nb_primitives": 1, "template_type": "SPHERE", "bottleneck_size": 1024, "hidden_neurons": 512,
                   "num_layers": 2, "activation": "relu", "remove_all_batchNorms": False, "number_points_eval": 2500,
                   "SVR": False}
DIM_TEMPLATE = {"SQUARE": 2, "SPHERE": 3}

# (name, fan_in, fan_out) of the encoder's five layers; bn<i+1> follows layer i
ENC_LAYERS = [("conv1", 3, 64), ("conv2", 64, 128), ("conv3", 128, BOTTLENECK), ("lin1", BOTTLENECK, BOTTLENECK),
              ("lin2", BOTTLENECK, BOTTLENECK)]


def dec_layers(num_layers, dim_template=2):
    """(name, fan_in, fan_out, name of its batch norm or None) of one primitive's decoder, in geoadv_atlas_weights order."""
    out = [("conv1", dim_template, BOTTLENECK, "bn1"), ("conv2", BOTTLENECK, HIDDEN, "bn2")]
    out += [("conv_list.%d" % i, HIDDEN, HIDDEN, "bn_list.%d" % i) for i in range(num_layers)]
    return out + [("last_conv", HIDDEN, 3, None)]


def key_names(nb_primitives, num_layers, decoder_bn=True, prefix="module."):
    """The state-dict keys of the reference's network.pth, in state_dict order (num_batches_tracked included)."""
    keys = []
    enc = prefix + "encoder."
    for name, _, _ in ENC_LAYERS:
        keys += [enc + name + ".weight", enc + name + ".bias"]
    for i in range(1, 6):
        keys += ["%sbn%d.%s" % (enc, i, f) for f in BN_FIELDS]
    for p in range(nb_primitives):
        d = "%sdecoder.decoder.%d." % (prefix, p)
        layers = dec_layers(num_layers)
        for name, _, _, _ in layers:
            keys += [d + name + ".weight", d + name + ".bias"]
        if decoder_bn:
            for _, _, _, bn in layers[:-1]:
                keys += [d + bn + "." + f for f in BN_FIELDS]
    return keys


def key_shapes(nb_primitives, num_layers, decoder_bn=True, dim_template=2):
    """{key without `module.`: shape} of every tensor inference reads (num_batches_tracked excluded)."""
    out = {}
    for name, fi, fo in ENC_LAYERS:
        conv = name.startswith("conv")
        out["encoder.%s.weight" % name] = (fo, fi, 1) if conv else (fo, fi)
        out["encoder.%s.bias" % name] = (fo,)
    for i, (_, _, fo) in enumerate(ENC_LAYERS):
        for f in BN_FIELDS[:4]:
            out["encoder.bn%d.%s" % (i + 1, f)] = (fo,)
    for p in range(nb_primitives):
        d = "decoder.decoder.%d." % p
        for name, fi, fo, bn in dec_layers(num_layers, dim_template):
            out[d + name + ".weight"] = (fo, fi, 1)
            out[d + name + ".bias"] = (fo,)
            if bn and decoder_bn:
                for f in BN_FIELDS[:4]:
                    out[d + bn + "." + f] = (fo,)
    return out


# ------------------------------------------------------------------------------------------------ options
def options(folder=None, overrides=None):
    """parser_transfer's options as inference uses them: the defaults, <folder>/options.json, then `overrides`."""
    opt = dict(DEFAULT_OPTIONS)
    path = os.path.join(folder, "options.json") if folder else None
    if path and os.path.exists(path):
        with open(path) as f:
            opt.update(json.load(f))
    if overrides:
        opt.update(overrides)
    return opt


def check_options(opt):
    """Refuses what this implementation does not run, with the reason; returns the checked model shape."""
    if opt.get("SVR"):
        raise ValueError("AtlasNet: SVR (single-view reconstruction, a ResNet image encoder) is not supported; the transfer "
                         "experiment feeds point clouds")
    tt = opt["template_type"]
    if tt == "SPHERE":
        raise ValueError("AtlasNet: template_type SPHERE is not supported: the reference's own transfer path keeps a fixed "
                         "buffer of 2500 points (atlasnet_ae.py:44) that its 2562-vertex icosphere overflows, and the "
                         "icosphere's vertex order comes from pymesh, which cannot be reproduced here")
    if tt != "SQUARE":
        raise ValueError("AtlasNet: unknown template_type %r" % (tt,))
    if opt["activation"] != "relu":
        raise ValueError("AtlasNet: activation %r is not supported (relu only)" % (opt["activation"],))
    if int(opt["bottleneck_size"]) != BOTTLENECK or int(opt["hidden_neurons"]) != HIDDEN:
        raise ValueError("AtlasNet: bottleneck_size %s / hidden_neurons %s are not supported (%d / %d only)"
                         % (opt["bottleneck_size"], opt["hidden_neurons"], BOTTLENECK, HIDDEN))
    nl, nb = int(opt["num_layers"]), int(opt["nb_primitives"])
    if not 0 <= nl <= MAX_LAYERS:
        raise ValueError("AtlasNet: num_layers %d is not supported (0 ... %d)" % (nl, MAX_LAYERS))
    if not 1 <= nb <= MAX_PRIMITIVES:
        raise ValueError("AtlasNet: nb_primitives %d is not supported (1 ... %d)" % (nb, MAX_PRIMITIVES))
    g = grain(int(opt["number_points_eval"]), nb)
    if g < 2:
        raise ValueError("AtlasNet: number_points_eval %s over %d primitives leaves fewer than 4 template points per "
                         "primitive" % (opt["number_points_eval"], nb))
    return {"nb_primitives": nb, "num_layers": nl, "grain": g, "dim_template": DIM_TEMPLATE[tt]}


# ------------------------------------------------------------------------------------------------ template
def grain(number_points_eval, nb_primitives):
    """Template.get_regular_points: npts = number_points_eval // nb_primitives points asked for, int(sqrt(npts)) per side."""
    return int(np.sqrt(number_points_eval // nb_primitives))


def square_template(g):
    """SquareTemplate.generate_square(g) (template.py:96-117) as the decoder sees it: vertices (i / (g-1), j / (g-1)),
    i outer and j inner, as float32 [g*g, 2]."""
    i, j = np.meshgrid(np.arange(g), np.arange(g), indexing="ij")
    v = np.stack([i.reshape(-1) / (g - 1), j.reshape(-1) / (g - 1)], axis=1)
    return v.astype(np.float32)


def template(nb_primitives, g):
    """[nb_primitives, g*g, 2]: the same square for every primitive."""
    return np.ascontiguousarray(np.broadcast_to(square_template(g), (nb_primitives, g * g, 2)))


# ------------------------------------------------------------------------------------------------ loading
def has_decoder_bn(state):
    return any(".bn1." in k for k in state if k.startswith("decoder."))


def validate(state, nb_primitives, num_layers, dim_template=2):
    """Raises KeyError listing every missing, unexpected or wrong-shape key at once; returns decoder_bn."""
    state = {k: v for k, v in state.items() if not k.endswith("num_batches_tracked")}
    dbn = has_decoder_bn(state)
    want = key_shapes(nb_primitives, num_layers, dbn, dim_template)
    missing = sorted(set(want) - set(state))
    unexpected = sorted(set(state) - set(want))
    wrong = sorted("%s %s (expected %s)" % (k, tuple(np.shape(state[k])), want[k]) for k in set(want) & set(state)
                   if tuple(np.shape(state[k])) != want[k])
    if missing or unexpected or wrong:
        parts = []
        if missing:
            parts.append("%d missing: %s" % (len(missing), ", ".join(missing)))
        if unexpected:
            parts.append("%d unexpected: %s" % (len(unexpected), ", ".join(unexpected)))
        if wrong:
            parts.append("%d of the wrong shape: %s" % (len(wrong), ", ".join(wrong)))
        raise KeyError("AtlasNet weights (nb_primitives %d, num_layers %d, decoder batch norm %s): %s"
                       % (nb_primitives, num_layers, "on" if dbn else "off", "; ".join(parts)))
    return dbn


def strip_prefix(state):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}


def load(folder, overrides=None):
    """(options, {key without `module.`: float32 array}) of <folder>/network.pth + <folder>/options.json."""
    import torch
    opt = options(folder, overrides)
    shape = check_options(opt)
    sd = torch.load(os.path.join(folder, "network.pth"), map_location="cpu", weights_only=True)
    state = {k: v.numpy() for k, v in strip_prefix(sd).items() if not k.endswith("num_batches_tracked")}
    validate(state, shape["nb_primitives"], shape["num_layers"], shape["dim_template"])
    return opt, {k: np.asarray(v, np.float32) for k, v in state.items()}


def parameter_names(nb_primitives, num_layers, decoder_bn=True):
    """The trainable tensors in EncoderDecoder.parameters() order (the index torch's optimizer state uses): the state-dict
    order without the running statistics and counters, no `module.` prefix."""
    return [k for k in key_names(nb_primitives, num_layers, decoder_bn, prefix="") if not k.endswith(BN_FIELDS[2:])]


def optimizer_state_dict(optimizer, nb_primitives, num_layers, decoder_bn=True):
    """A real torch.optim.Adam state_dict from optimizer = {'step': int, 'lr': float, 'exp_avg': {key: array}, 'exp_avg_sq':
    {key: array}}: state[i] = {step, exp_avg, exp_avg_sq} in parameter_names() order, plus this torch's param_groups."""
    import torch
    shapes = key_shapes(nb_primitives, num_layers, decoder_bn)
    names = parameter_names(nb_primitives, num_layers, decoder_bn)
    params = [torch.zeros(shapes[k], dtype=torch.float32, requires_grad=True) for k in names]
    opt = torch.optim.Adam(params, lr=float(optimizer.get("lr", 1e-3)), betas=(0.9, 0.999))
    for k, p in zip(names, params):
        opt.state[p] = {"step": torch.tensor(float(optimizer["step"])),
                        "exp_avg": torch.from_numpy(np.ascontiguousarray(optimizer["exp_avg"][k], np.float32).reshape(shapes[k])),
                        "exp_avg_sq": torch.from_numpy(np.ascontiguousarray(optimizer["exp_avg_sq"][k], np.float32).reshape(shapes[k]))}
    return opt.state_dict()


def save(folder, opt, state, optimizer=None, tracked=None):
    """Writes network.pth (DataParallel prefix, num_batches_tracked included, as the reference's trainer does) and
    options.json.  tracked: the value of every num_batches_tracked (the training steps taken; 7 where not given).
    optimizer (see optimizer_state_dict): also writes optimizer.pth, a torch.optim.Adam state_dict, as
    trainer_abstract.py:76-80 does."""
    import torch
    os.makedirs(folder, exist_ok=True)
    sd = {}
    dbn = has_decoder_bn(state)
    for k in key_names(int(opt["nb_primitives"]), int(opt["num_layers"]), dbn):
        short = k[len("module."):]
        sd[k] = torch.tensor(7 if tracked is None else int(tracked), dtype=torch.int64) if k.endswith("num_batches_tracked") \
            else torch.from_numpy(np.ascontiguousarray(state[short], np.float32))
    torch.save(sd, os.path.join(folder, "network.pth"))
    if optimizer is not None:
        torch.save(optimizer_state_dict(optimizer, int(opt["nb_primitives"]), int(opt["num_layers"]), dbn),
                   os.path.join(folder, "optimizer.pth"))
    with open(os.path.join(folder, "options.json"), "w") as f:
        json.dump(opt, f)


def load_training(folder, overrides=None):
    """(options, state, optimizer, tracked) of a folder `save` (or the reference's trainer) wrote: optimizer = {'step', 'lr',
    'exp_avg', 'exp_avg_sq'} keyed by parameter_names(), or None where optimizer.pth is absent or holds no state; tracked =
    the file's num_batches_tracked."""
    import torch
    opt, state = load(folder, overrides)
    sd = torch.load(os.path.join(folder, "network.pth"), map_location="cpu", weights_only=True)
    tracked = int(strip_prefix(sd)["encoder.bn1.num_batches_tracked"])
    path = os.path.join(folder, "optimizer.pth")
    optimizer = None
    if os.path.exists(path):
        osd = torch.load(path, map_location="cpu", weights_only=False)
        st = osd.get("state", {})
        if st:
            names = parameter_names(int(opt["nb_primitives"]), int(opt["num_layers"]), has_decoder_bn(state))
            if sorted(st) != list(range(len(names))):
                raise KeyError("%s: the optimizer state has %d entries, the model %d parameters" % (path, len(st), len(names)))
            optimizer = {"step": int(float(st[0]["step"])), "lr": float(osd["param_groups"][0]["lr"]),
                         "exp_avg": {k: st[i]["exp_avg"].numpy() for i, k in enumerate(names)},
                         "exp_avg_sq": {k: st[i]["exp_avg_sq"].numpy() for i, k in enumerate(names)}}
    return opt, state, optimizer, tracked


def initial_weights(seed=0, nb_primitives=25, num_layers=2, decoder_bn=True, number_points_eval=2500):
    """(options, state) of a fresh model as the reference builds it: every Conv1d / Linear weight and bias U(-1 / sqrt(fan_in),
    1 / sqrt(fan_in)) (torch's default), then weights_init (model.py:37-41): every BatchNorm1d weight N(1, 0.02), bias 0;
    running_mean 0, running_var 1.  Drawn from np.random.default_rng(seed) in state-dict order -- the same distributions as
    torch's, not its random stream."""
    rng = np.random.default_rng(seed)
    opt = dict(DEFAULT_OPTIONS, nb_primitives=nb_primitives, num_layers=num_layers, template_type="SQUARE",
               remove_all_batchNorms=not decoder_bn, number_points_eval=number_points_eval)
    s = {}

    def layer(k, fi, fo, conv):
        bound = 1.0 / np.sqrt(fi)
        s[k + ".weight"] = rng.uniform(-bound, bound, (fo, fi, 1) if conv else (fo, fi)).astype(np.float32)
        s[k + ".bias"] = rng.uniform(-bound, bound, fo).astype(np.float32)

    def bn(k, fo):
        s[k + ".weight"] = (1.0 + 0.02 * rng.standard_normal(fo)).astype(np.float32)
        s[k + ".bias"] = np.zeros(fo, np.float32)
        s[k + ".running_mean"] = np.zeros(fo, np.float32)
        s[k + ".running_var"] = np.ones(fo, np.float32)

    for name, fi, fo in ENC_LAYERS:
        layer("encoder." + name, fi, fo, name.startswith("conv"))
    for i, (_, _, fo) in enumerate(ENC_LAYERS):
        bn("encoder.bn%d" % (i + 1), fo)
    for p in range(nb_primitives):
        d = "decoder.decoder.%d." % p
        for name, fi, fo, _ in dec_layers(num_layers):
            layer(d + name, fi, fo, True)
        if decoder_bn:
            for _, _, fo, b in dec_layers(num_layers)[:-1]:
                bn(d + b, fo)
    return opt, s


# ------------------------------------------------------------------------------------------------ train-mode template
_M64 = (1 << 64) - 1
_GOLDEN = 0x9e3779b97f4a7c15


def _mix64(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def train_template(seed, tracked, nb_primitives, points):
    """The template points the device draws at training step `tracked` (csrc/atlas_train.hip restated): float32
    [nb_primitives, points, 2] in [0, 1), coordinate d of point j of primitive q from
    key = mix(mix(mix(seed + G) ^ tracked) ^ (q << 32 | j)), r = mix(key + (d + 1) G), value = (r >> 40) * 2^-24."""
    with np.errstate(over="ignore"):
        base = _mix64(_mix64(np.uint64((int(seed) + _GOLDEN) & _M64)) ^ np.uint64(int(tracked) & _M64))
        q = np.arange(nb_primitives, dtype=np.uint64)[:, None, None]
        j = np.arange(points, dtype=np.uint64)[None, :, None]
        d = np.arange(2, dtype=np.uint64)[None, None, :]
        key = _mix64(base ^ ((q << np.uint64(32)) | j))
        r = _mix64(key + (d + np.uint64(1)) * np.uint64(_GOLDEN))
    return ((r >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ canonical layout
def canonical(state, nb_primitives, num_layers):
    """Arrays of geoadv_atlas_weights: enc_* lists of 5, dec_* lists of 3 + num_layers; w as [fan_in, fan_out] (decoder:
    stacked over primitives), BN entries None where the layer has none."""
    dbn = has_decoder_bn(state)
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    out = {k: [] for k in ("enc_w", "enc_b", "enc_gamma", "enc_beta", "enc_mean", "enc_var",
                           "dec_w", "dec_b", "dec_gamma", "dec_beta", "dec_mean", "dec_var")}
    for i, (name, fi, fo) in enumerate(ENC_LAYERS):
        out["enc_w"].append(f32(np.asarray(state["encoder.%s.weight" % name]).reshape(fo, fi).T))
        out["enc_b"].append(f32(state["encoder.%s.bias" % name]))
        bn = "encoder.bn%d." % (i + 1)
        for k, f in (("enc_gamma", "weight"), ("enc_beta", "bias"), ("enc_mean", "running_mean"), ("enc_var", "running_var")):
            out[k].append(f32(state[bn + f]))
    for name, fi, fo, bn in dec_layers(num_layers, 2):
        pre = ["decoder.decoder.%d." % p for p in range(nb_primitives)]
        w0 = np.asarray(state[pre[0] + name + ".weight"])
        fi = w0.shape[1]
        out["dec_w"].append(f32(np.stack([np.asarray(state[q + name + ".weight"]).reshape(fo, fi).T for q in pre])))
        out["dec_b"].append(f32(np.stack([state[q + name + ".bias"] for q in pre])))
        for k, f in (("dec_gamma", "weight"), ("dec_beta", "bias"), ("dec_mean", "running_mean"), ("dec_var", "running_var")):
            out[k].append(f32(np.stack([state[q + bn + "." + f] for q in pre])) if (bn and dbn) else None)
    return out


# ------------------------------------------------------------------------------------------------ float64 forward
def _bn(x, state, bn, calibrate):
    if calibrate:
        flat = x.reshape(-1, x.shape[-1])
        state[bn + ".running_mean"] = flat.mean(axis=0)
        state[bn + ".running_var"] = flat.var(axis=0)
    g, b, m, v = (np.asarray(state[bn + "." + f], np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + BN_EPS) * g + b


def forward64(state, pc, tmpl, num_layers, calibrate=False, calibrate_decoder=None):
    """float64 forward: pc (b, n, 3), tmpl (nb, g2, dim) -> (latent (b, 1024), recon (b, nb * g2, 3)).  calibrate=True first
    sets every encoder batch norm's running statistics to the batch statistics of its input (layer by layer);
    calibrate_decoder (default: calibrate) does the same for the decoder's."""
    s = state
    cal_dec = calibrate if calibrate_decoder is None else calibrate_decoder
    w = lambda k: np.asarray(s[k + ".weight"], np.float64)
    lin = lambda x, k: x @ w(k).reshape(w(k).shape[0], -1).T + np.asarray(s[k + ".bias"], np.float64)
    x = np.asarray(pc, np.float64)
    h = np.maximum(_bn(lin(x, "encoder.conv1"), s, "encoder.bn1", calibrate), 0)
    h = np.maximum(_bn(lin(h, "encoder.conv2"), s, "encoder.bn2", calibrate), 0)
    h = _bn(lin(h, "encoder.conv3"), s, "encoder.bn3", calibrate).max(axis=1)
    h = np.maximum(_bn(lin(h, "encoder.lin1"), s, "encoder.bn4", calibrate), 0)
    z = np.maximum(_bn(lin(h, "encoder.lin2"), s, "encoder.bn5", calibrate), 0)
    dbn = has_decoder_bn(s)
    outs = []
    for p in range(len(tmpl)):
        d = "decoder.decoder.%d." % p
        norm = (lambda a, bn: _bn(a, s, d + bn, cal_dec)) if dbn else (lambda a, bn: a)
        t = np.asarray(tmpl[p], np.float64)
        a = lin(t, d + "conv1")[None] + z[:, None, :]
        a = np.maximum(norm(a, "bn1"), 0)
        a = np.maximum(norm(lin(a, d + "conv2"), "bn2"), 0)
        for i in range(num_layers):
            a = np.maximum(norm(lin(a, d + "conv_list.%d" % i), "bn_list.%d" % i), 0)
        outs.append(lin(a, d + "last_conv"))
    return z, (np.concatenate(outs, axis=1) if outs else np.zeros((len(x), 0, 3)))


def calibration_batch(clouds=16, points=1024):
    """The fixed batch synthetic_state calibrates on: uniform in the unit cube centred at the origin."""
    return np.random.default_rng(12345).random((clouds, points, 3)) - 0.5


def synthetic_state(nb_primitives=25, num_layers=2, decoder_bn=True, g=None, seed=0, number_points_eval=2500):
    """(options, state) of a model with the reference's keys and shapes whose activations are O(1) through every layer:
    He-scaled weights, the batch norms' running statistics calibrated in float64 on calibration_batch() with gamma in
    [0.8, 1.2] and beta in [-0.3, 0.3] (so that roughly half of every ReLU layer is active), and the output layer scaled to
    coordinates of about 0.5.  Without decoder batch norm the biases centre each pre-activation instead."""
    rng = np.random.default_rng(seed)
    opt = dict(DEFAULT_OPTIONS, nb_primitives=nb_primitives, num_layers=num_layers, template_type="SQUARE",
               remove_all_batchNorms=not decoder_bn, number_points_eval=number_points_eval)
    g = grain(number_points_eval, nb_primitives) if g is None else g
    s = {}

    def layer(k, fi, fo, conv):
        s[k + ".weight"] = rng.standard_normal((fo, fi, 1) if conv else (fo, fi)) * np.sqrt(2.0 / fi)
        s[k + ".bias"] = rng.standard_normal(fo) * 0.1

    def bn(k, fo):
        s[k + ".weight"] = rng.uniform(0.8, 1.2, fo)
        s[k + ".bias"] = rng.uniform(-0.3, 0.3, fo)
        s[k + ".running_mean"] = np.zeros(fo)
        s[k + ".running_var"] = np.ones(fo)

    for i, (name, fi, fo) in enumerate(ENC_LAYERS):
        layer("encoder." + name, fi, fo, name.startswith("conv"))
        bn("encoder.bn%d" % (i + 1), fo)
    for p in range(nb_primitives):
        d = "decoder.decoder.%d." % p
        for name, fi, fo, b in dec_layers(num_layers):
            layer(d + name, fi, fo, True)
            if b and decoder_bn:
                bn(d + b, fo)
    tmpl = template(nb_primitives, g)
    x = calibration_batch()
    z, _ = forward64(s, x, tmpl[:0], 0, calibrate=True)               # the encoder, on all 16 clouds
    x = x[:4]                                                          # the decoder, on the first 4 (25 x 100 rows each)
    if decoder_bn:
        forward64(s, x, tmpl, num_layers, calibrate=False, calibrate_decoder=True)
    else:
        # no batch norm to standardise the decoder: centre every pre-activation on the calibration batch through its bias
        # (and scale the weights to unit spread), layer by layer
        z = z[:4]
        for p in range(nb_primitives):
            d = "decoder.decoder.%d." % p
            t = np.asarray(tmpl[p], np.float64)
            w1 = s[d + "conv1.weight"].reshape(BOTTLENECK, -1)
            pre = ((t @ w1.T)[None] + z[:, None, :]).reshape(-1, BOTTLENECK)      # the latent enters unscaled
            s[d + "conv1.bias"] = -pre.mean(axis=0) + rng.uniform(-0.3, 0.3, BOTTLENECK) * pre.std(axis=0)
            a = np.maximum(pre + s[d + "conv1.bias"], 0)
            for name, fi, fo, _ in dec_layers(num_layers)[1:-1]:
                w = s[d + name + ".weight"].reshape(fo, fi)
                pre = a @ w.T
                sd = pre.std(axis=0) + 1e-3
                s[d + name + ".weight"] = (w / sd[:, None]).reshape(fo, fi, 1)
                s[d + name + ".bias"] = -pre.mean(axis=0) / sd + rng.uniform(-0.3, 0.3, fo)
                a = np.maximum(pre / sd + s[d + name + ".bias"], 0)
    # output scale: coordinates of about 0.5
    _, rec = forward64(s, x, tmpl, num_layers)
    for p in range(nb_primitives):
        d = "decoder.decoder.%d." % p
        g2 = tmpl.shape[1]
        r = rec[:, p * g2:(p + 1) * g2].reshape(-1, 3)
        f = 0.5 / (r.std(axis=0) + 1e-6)
        s[d + "last_conv.weight"] = s[d + "last_conv.weight"] * f[:, None, None]
        s[d + "last_conv.bias"] = s[d + "last_conv.bias"] * f + rng.uniform(-0.2, 0.2, 3) - r.mean(axis=0) * f
    return opt, {k: np.asarray(v, np.float32) for k, v in s.items()}
