"""Weights of the FoldingNet auto-encoder of the transfer experiment (transfer/foldingnet): state-dict key names derived
from the module structure, loading <transfer_ae_folder>/checkpoint_<epoch>.pth, the decoder's 45 x 45 grid, conversion to
the layout of geoadv_fold_weights (include/geoadv.h), a float64 forward, and a calibrated synthetic model for tests and
measurements.

Key names.  train_foldingnet.py:173-177 saves {'epoch', 'model': FoldingNet_graph().state_dict(), 'optimizer'}: no
DataParallel, so no `module.` prefix (one is accepted).  FoldingNet_graph registers `encoder` (FoldingNetEnc_with_graph:
conv1..conv5, fc1, fc2, graph_pooling -- no parameters --, bn1..bn6) and `decoder` (FoldingNetDec: fold1, fold2, each
conv1..conv3 and a parameter-free ReLU).  Every BatchNorm1d carries weight, bias, running_mean, running_var and
num_batches_tracked; the last is ignored here.
"""
import os

import numpy as np

BN_EPS = 1e-5
CODE = 512
GRID = 45
NUM_NEIGHBOURS = 16
BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")

# (name, fan_in, fan_out, conv) of the encoder's seven layers; bn<i+1> follows layer i for the first six
ENC_LAYERS = [("conv1", 12, 64, True), ("conv2", 64, 64, True), ("conv3", 64, 64, True), ("conv4", 64, 128, True),
              ("conv5", 128, 1024, True), ("fc1", 1024, CODE, False), ("fc2", CODE, CODE, False)]
# (name, fan_in, fan_out) of the decoder's six layers, in geoadv_fold_weights order
DEC_LAYERS = [("fold1.conv1", CODE + 2, 512), ("fold1.conv2", 512, 512), ("fold1.conv3", 512, 3),
              ("fold2.conv1", CODE + 3, 512), ("fold2.conv2", 512, 512), ("fold2.conv3", 512, 3)]


def key_names(prefix=""):
    """The state-dict keys of FoldingNet_graph, in state_dict order (num_batches_tracked included)."""
    keys = []
    for name, _, _, _ in ENC_LAYERS:
        keys += ["%sencoder.%s.%s" % (prefix, name, f) for f in ("weight", "bias")]
    for i in range(1, 7):
        keys += ["%sencoder.bn%d.%s" % (prefix, i, f) for f in BN_FIELDS]
    for name, _, _ in DEC_LAYERS:
        keys += ["%sdecoder.%s.%s" % (prefix, name, f) for f in ("weight", "bias")]
    return keys


def key_shapes():
    """{key without prefix: shape} of every tensor inference reads (num_batches_tracked excluded)."""
    out = {}
    for i, (name, fi, fo, conv) in enumerate(ENC_LAYERS):
        out["encoder.%s.weight" % name] = (fo, fi, 1) if conv else (fo, fi)
        out["encoder.%s.bias" % name] = (fo,)
        if i < 6:
            for f in BN_FIELDS[:4]:
                out["encoder.bn%d.%s" % (i + 1, f)] = (fo,)
    for name, fi, fo in DEC_LAYERS:
        out["decoder.%s.weight" % name] = (fo, fi, 1)
        out["decoder.%s.bias" % name] = (fo,)
    return out


def grid():
    """GridSamplingLayer's [[-0.3, 0.3, 45], [-0.3, 0.3, 45]] grid (foldingnet.py:138-157) as float32 [2025, 2]: point
    p = r * 45 + c is (x_c, y_r)."""
    lin = np.linspace(-0.3, 0.3, GRID)
    xs, ys = np.meshgrid(lin, lin)
    return np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)


# ------------------------------------------------------------------------------------------------ loading
def strip_prefix(state):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}


def validate(state):
    """Raises KeyError listing every missing, unexpected or wrong-shape key at once."""
    state = {k: v for k, v in state.items() if not k.endswith("num_batches_tracked")}
    want = key_shapes()
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
        raise KeyError("FoldingNet weights: %s" % "; ".join(parts))


def checkpoint_path(folder, epoch):
    return os.path.join(folder, "checkpoint_%s.pth" % epoch)


def load(folder, epoch):
    """{key without `module.`: float32 array} of <folder>/checkpoint_<epoch>.pth (its 'model' entry)."""
    import torch
    ck = torch.load(checkpoint_path(folder, epoch), map_location="cpu", weights_only=False)
    if not isinstance(ck, dict) or "model" not in ck:
        raise KeyError("FoldingNet checkpoint %s has no 'model' entry" % checkpoint_path(folder, epoch))
    state = {k: np.asarray(v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in strip_prefix(ck["model"]).items()
             if not k.endswith("num_batches_tracked")}
    validate(state)
    return {k: np.asarray(v, np.float32) for k, v in state.items()}


def parameter_names():
    """The trainable tensors in FoldingNet_graph().parameters() order (the index torch's optimizer state uses): the state-dict
    order without the running statistics and counters."""
    return [k for k in key_names() if not k.endswith(BN_FIELDS[2:])]


def optimizer_state_dict(optimizer):
    """A real torch.optim.Adam state_dict from optimizer = {'step': int, 'exp_avg': {key: array}, 'exp_avg_sq': {key: array},
    'lr', 'weight_decay'}: state[i] = {step, exp_avg, exp_avg_sq} in parameter_names() order, plus this torch's param_groups."""
    import torch
    shapes = key_shapes()
    names = parameter_names()
    params = [torch.zeros(shapes[k], dtype=torch.float32, requires_grad=True) for k in names]
    opt = torch.optim.Adam(params, lr=float(optimizer.get("lr", 1e-4)), betas=(0.9, 0.999),
                           weight_decay=float(optimizer.get("weight_decay", 1e-6)))
    for k, p in zip(names, params):
        opt.state[p] = {"step": torch.tensor(float(optimizer["step"])),
                        "exp_avg": torch.from_numpy(np.ascontiguousarray(optimizer["exp_avg"][k], np.float32).reshape(shapes[k])),
                        "exp_avg_sq": torch.from_numpy(np.ascontiguousarray(optimizer["exp_avg_sq"][k], np.float32).reshape(shapes[k]))}
    return opt.state_dict()


def save(folder, epoch, state, prefix="", optimizer=None, extra=None):
    """Writes checkpoint_<epoch>.pth as train_foldingnet.py:173-177 does: {'epoch', 'model', 'optimizer'}.  Without
    `optimizer` the optimizer entry is empty; with it (see optimizer_state_dict) it is a torch.optim.Adam state_dict and
    every num_batches_tracked is the optimizer's step count.  extra: further top-level entries (the trainer's counters)."""
    import torch
    os.makedirs(folder, exist_ok=True)
    tracked = 7 if optimizer is None else int(optimizer["step"])
    sd = {}
    for k in key_names(prefix):
        short = k[len(prefix):]
        sd[k] = torch.tensor(tracked, dtype=torch.int64) if k.endswith("num_batches_tracked") else torch.from_numpy(
            np.ascontiguousarray(state[short], np.float32))
    ck = {"epoch": epoch, "model": sd,
          "optimizer": {"state": {}, "param_groups": []} if optimizer is None else optimizer_state_dict(optimizer)}
    ck.update(extra or {})
    torch.save(ck, checkpoint_path(folder, epoch))


def load_training(folder, epoch):
    """(state, optimizer, checkpoint) of a checkpoint `save` wrote with an optimizer: optimizer = {'step', 'exp_avg',
    'exp_avg_sq'} keyed by parameter_names(), or None where the checkpoint's optimizer entry is empty."""
    import torch
    ck = torch.load(checkpoint_path(folder, epoch), map_location="cpu", weights_only=False)
    st = ck["optimizer"].get("state", {})
    opt = None
    if st:
        names = parameter_names()
        if sorted(st) != list(range(len(names))):
            raise KeyError("checkpoint %s: the optimizer state has %d entries, the model %d parameters"
                           % (checkpoint_path(folder, epoch), len(st), len(names)))
        opt = {"step": int(float(st[0]["step"])), "exp_avg": {k: st[i]["exp_avg"].numpy() for i, k in enumerate(names)},
               "exp_avg_sq": {k: st[i]["exp_avg_sq"].numpy() for i, k in enumerate(names)}}
    return load(folder, epoch), opt, ck


def initial_weights(seed=0):
    """A fresh model as torch initialises FoldingNet_graph(): every Conv1d / Linear weight and bias U(-1 / sqrt(fan_in),
    1 / sqrt(fan_in)) (kaiming_uniform_(a = sqrt(5)) on the weight and the matching bound on the bias both come to that),
    every BatchNorm1d weight 1, bias 0, running_mean 0, running_var 1.  Drawn from np.random.default_rng(seed), layer by
    layer in state-dict order -- the same distribution as torch's, not its random stream."""
    rng = np.random.default_rng(seed)
    s = {}
    layers = [("encoder." + name, fi, fo, conv) for name, fi, fo, conv in ENC_LAYERS] + \
             [("decoder." + name, fi, fo, True) for name, fi, fo in DEC_LAYERS]
    for k, fi, fo, conv in layers:
        bound = 1.0 / np.sqrt(fi)
        s[k + ".weight"] = rng.uniform(-bound, bound, (fo, fi, 1) if conv else (fo, fi)).astype(np.float32)
        s[k + ".bias"] = rng.uniform(-bound, bound, fo).astype(np.float32)
    for i, (_, _, fo, _) in enumerate(ENC_LAYERS[:6]):
        bn = "encoder.bn%d." % (i + 1)
        s[bn + "weight"] = np.ones(fo, np.float32)
        s[bn + "bias"] = np.zeros(fo, np.float32)
        s[bn + "running_mean"] = np.zeros(fo, np.float32)
        s[bn + "running_var"] = np.ones(fo, np.float32)
    return s


# ------------------------------------------------------------------------------------------------ canonical layout
def canonical(state):
    """Arrays of geoadv_fold_weights: enc_* lists of 7 (fc2's BN entries None), dec_* lists of 6; w as [fan_in, fan_out]."""
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    out = {k: [] for k in ("enc_w", "enc_b", "enc_gamma", "enc_beta", "enc_mean", "enc_var", "dec_w", "dec_b")}
    for i, (name, fi, fo, _) in enumerate(ENC_LAYERS):
        out["enc_w"].append(f32(np.asarray(state["encoder.%s.weight" % name]).reshape(fo, fi).T))
        out["enc_b"].append(f32(state["encoder.%s.bias" % name]))
        bn = "encoder.bn%d." % (i + 1)
        for k, f in (("enc_gamma", "weight"), ("enc_beta", "bias"), ("enc_mean", "running_mean"), ("enc_var", "running_var")):
            out[k].append(f32(state[bn + f]) if i < 6 else None)
    for name, fi, fo in DEC_LAYERS:
        out["dec_w"].append(f32(np.asarray(state["decoder.%s.weight" % name]).reshape(fo, fi).T))
        out["dec_b"].append(f32(state["decoder.%s.bias" % name]))
    return out


# ------------------------------------------------------------------------------------------------ float64 forward
def knn_graph(pc):
    """prepare_graph.knn_search of each cloud by brute force in float64: (knn [b, n, 16] with column 0 of the 17 nearest
    dropped, cov [b, n, 9] rounded to float32 as the reference stores it, rows: per cloud a list of the sorted symmetric
    adjacency rows)."""
    pc = np.asarray(pc, np.float64)
    b, n, _ = pc.shape
    knn = np.zeros((b, n, NUM_NEIGHBOURS), np.int64)
    cov = np.zeros((b, n, 9), np.float32)
    rows = []
    for c in range(b):
        x = pc[c]
        d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        nb = np.argsort(d, axis=1, kind="stable")[:, 1:NUM_NEIGHBOURS + 1]
        knn[c] = nb
        g = x[nb] - x[nb].mean(axis=1, keepdims=True)
        cov[c] = (np.einsum("nki,nkj->nij", g, g) / (NUM_NEIGHBOURS - 1)).reshape(n, 9)
        adj = [set(r) for r in nb.tolist()]
        for i in range(n):
            for j in nb[i]:
                adj[j].add(i)
        rows.append([np.array(sorted(a), np.int64) for a in adj])
    return knn, cov, rows


def _bn(x, state, bn, calibrate, axes):
    if calibrate:
        state[bn + ".running_mean"] = x.mean(axis=axes)
        state[bn + ".running_var"] = x.var(axis=axes)
    g, b, m, v = (np.asarray(state[bn + "." + f], np.float64) for f in ("weight", "bias", "running_mean", "running_var"))
    return (x - m) / np.sqrt(v + BN_EPS) * g + b


def forward64(state, pc, cov, cols, calibrate=False):
    """float64 forward of pc (b, n, 3) with cov (b, n, 9) and the neighbour columns cols (2, b, n, 16) of the two graph
    pools -> (code (b, 512), p1 (b, 2025, 3), recon (b, 2025, 3)).  calibrate=True first sets every encoder batch norm's
    running statistics to the batch statistics of its input."""
    s = state
    w = lambda k: np.asarray(s[k + ".weight"], np.float64)
    lin = lambda x, k: x @ w(k).reshape(w(k).shape[0], -1).T + np.asarray(s[k + ".bias"], np.float64)
    bn = lambda x, i, axes: _bn(x, s, "encoder.bn%d" % i, calibrate, axes)
    b = len(pc)
    ar = np.arange(b)[:, None, None]

    def pool(h, c):
        return np.maximum(h[ar, c].max(axis=2), h)

    h = np.concatenate([np.asarray(pc, np.float64), np.asarray(cov, np.float64)], axis=2)
    for i in (1, 2, 3):
        h = np.maximum(bn(lin(h, "encoder.conv%d" % i), i, (0, 1)), 0)
    h = np.maximum(pool(h, cols[0]), 0)
    h = np.maximum(bn(lin(h, "encoder.conv4"), 4, (0, 1)), 0)
    h = np.maximum(pool(h, cols[1]), 0)
    h = bn(lin(h, "encoder.conv5"), 5, (0, 1)).max(axis=1)
    h = np.maximum(bn(lin(h, "encoder.fc1"), 6, 0), 0)
    code = lin(h, "encoder.fc2")
    g = np.broadcast_to(grid().astype(np.float64), (b, GRID * GRID, 2))
    rep = np.broadcast_to(code[:, None, :], (b, GRID * GRID, CODE))
    a = np.maximum(lin(np.concatenate([rep, g], axis=2), "decoder.fold1.conv1"), 0)
    a = np.maximum(lin(a, "decoder.fold1.conv2"), 0)
    p1 = lin(a, "decoder.fold1.conv3")
    a = np.maximum(lin(np.concatenate([rep, p1], axis=2), "decoder.fold2.conv1"), 0)
    a = np.maximum(lin(a, "decoder.fold2.conv2"), 0)
    return code, p1, lin(a, "decoder.fold2.conv3")


def first_positions(rows, b, n):
    """Positions 0 .. 15 of every row, both pool layers: the fixed picks synthetic_state calibrates with."""
    return np.broadcast_to(np.arange(NUM_NEIGHBOURS), (2, b, n, NUM_NEIGHBOURS))


def resolve(rows, picks):
    """Neighbour columns (2, b, n, 16) of positions picks (2, b, n, 16) in the sorted adjacency rows."""
    picks = np.asarray(picks)
    out = np.zeros(picks.shape, np.int64)
    for c, rc in enumerate(rows):
        for i, r in enumerate(rc):
            out[:, c, i] = r[picks[:, c, i]]
    return out


def calibration_batch(clouds=16, points=512):
    """The fixed batch synthetic_state calibrates on: uniform in the unit cube centred at the origin."""
    return np.random.default_rng(12345).random((clouds, points, 3)) - 0.5


def synthetic_state(seed=0):
    """A model with the reference's keys and shapes whose activations are O(1) through every layer: He-scaled weights
    (conv1's input columns divided by each input channel's spread, so that the covariance channels weigh as much as the
    coordinates), the encoder's batch norms calibrated in float64 on calibration_batch() with gamma in [0.8, 1.2] and beta in
    [-0.3, 0.3], the decoder's hidden layers (which have no batch norm) centred through their biases and scaled to unit
    spread -- the point rows of each fold's first layer (grid, p1) first scaled to weigh as much as the code rows --, and
    both folds' outputs scaled to coordinates of about 0.5."""
    rng = np.random.default_rng(seed)
    s = {}

    def layer(k, fi, fo, conv):
        s[k + ".weight"] = rng.standard_normal((fo, fi, 1) if conv else (fo, fi)) * np.sqrt(2.0 / fi)
        s[k + ".bias"] = rng.standard_normal(fo) * 0.1

    for i, (name, fi, fo, conv) in enumerate(ENC_LAYERS):
        layer("encoder." + name, fi, fo, conv)
        if i < 6:
            s["encoder.bn%d.weight" % (i + 1)] = rng.uniform(0.8, 1.2, fo)
            s["encoder.bn%d.bias" % (i + 1)] = rng.uniform(-0.3, 0.3, fo)
    for name, fi, fo in DEC_LAYERS:
        layer("decoder." + name, fi, fo, True)
    x = calibration_batch()
    _, cov, rows = knn_graph(x)
    spread = np.concatenate([x, cov], axis=2).reshape(-1, 12).std(axis=0)
    s["encoder.conv1.weight"] = s["encoder.conv1.weight"] / spread[None, :, None]
    cols = resolve(rows, first_positions(rows, *x.shape[:2]))
    code, _, _ = forward64(s, x, cov, cols, calibrate=True)
    # the decoder: centre and scale every hidden pre-activation on the calibration codes, layer by layer
    b = len(x)
    g = np.broadcast_to(grid().astype(np.float64), (b, GRID * GRID, 2))
    rep = np.broadcast_to(code[:, None, :], (b, GRID * GRID, CODE))
    inp = np.concatenate([rep, g], axis=2)
    for f in ("fold1", "fold2"):
        # a trained decoder folds its grid: give the point rows of conv1 (grid, then p1) as much weight as the code rows
        k = "decoder.%s.conv1" % f
        wt = s[k + ".weight"][:, :, 0]
        flat = inp.reshape(-1, inp.shape[-1])
        ratio = (flat[:, :CODE] @ wt[:, :CODE].T).std() / (flat[:, CODE:] @ wt[:, CODE:].T).std()
        wt[:, CODE:] *= ratio
        s[k + ".weight"] = wt[:, :, None]
        a = inp
        for name in ("conv1", "conv2"):
            k = "decoder.%s.%s" % (f, name)
            wt = s[k + ".weight"][:, :, 0]
            pre = a.reshape(-1, a.shape[-1]) @ wt.T
            sd = pre.std(axis=0) + 1e-3
            s[k + ".weight"] = (wt / sd[:, None])[:, :, None]
            s[k + ".bias"] = -pre.mean(axis=0) / sd + rng.uniform(-0.3, 0.3, len(sd))
            a = np.maximum(pre / sd + s[k + ".bias"], 0).reshape(b, GRID * GRID, -1)
        k = "decoder.%s.conv3" % f
        out = a.reshape(-1, 512) @ s[k + ".weight"][:, :, 0].T
        sc = 0.5 / (out.std(axis=0) + 1e-6)
        s[k + ".weight"] = s[k + ".weight"] * sc[:, None, None]
        s[k + ".bias"] = rng.uniform(-0.2, 0.2, 3) - out.mean(axis=0) * sc
        p1 = (out * sc + s[k + ".bias"]).reshape(b, GRID * GRID, 3)
        inp = np.concatenate([rep, p1], axis=2)
    return {k: np.asarray(v, np.float32) for k, v in s.items()}
