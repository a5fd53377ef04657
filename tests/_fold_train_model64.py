"""float64 model of ONE FoldingNet training step (csrc/fold_train.hip restated): the train-mode forward as torch functional
ops on the CPU (F.batch_norm(training=True) updates the running statistics itself), differentiated by autograd, then
torch.optim.Adam itself.  The graph (cov) and both pools' neighbour columns are inputs, as in _fold_model64.model.

The rules autograd would not pick by itself are written out: a graph pool takes the FIRST maximum among (the point itself,
its 16 columns in slot order) and passes its gradient there if that maximum is positive; the global maximum over points
takes the first maximal row; Chamfer's nearest neighbours are found first and the loss is gathered at them.

Pins: the step's discrete decisions can be fixed to given ones instead of fp64's own --
  pins["relu"][i]    bool [rows][C]            ReLU mask after bn<i> (i = 1, 2, 3, 4, 6)
  pins["win"][p]     int [B][n][C]             pool p's winning row in the cloud, -1 = no positive maximum
  pins["gmax"]       int [B][1024]             the global maximum's row
  pins["hidden"][k]  bool [B * 2025][512]      ReLU masks of fold1.conv1, fold1.conv2, fold2.conv1, fold2.conv2
  pins["chamfer"]    (int [B][n], int [B][2025])
Pinning fp64's own decisions reproduces the unpinned step.  res["disagree"][name] = (pins that differ from fp64's own,
number of pins, the largest fp64 distance from its boundary of a differing pin: |ReLU input|, or own maximum minus the
pinned element's value, or pinned distance minus the smallest).

tie: candidates within `tie` of a maximum count as attaining it, and the first of them wins (pools and the global maximum).
0.0, the default, is the plain first maximum.  A cloud whose points share their pooled features (n = 17: every point pools over
nearly all others) has rows that are EQUAL in exact arithmetic and on the device, where equal inputs meet equal arithmetic, while
float64 matrix products of equal rows differ by their own rounding (1e-15): a `tie` far above that and far below any fp32 ulp
lets the float64 model see those ties as the ties they are.

perturb (tests only) restates the step wrongly: "no_weight_decay", "tf_adam_eps" (sqrt(v) + eps before the bias correction),
"biased_running_var", "bn_no_m2" = i (bn<i>'s backward without its xhat * mean(dy xhat) term), "pool_all" (the pool gradient
credited to all 16 columns as well), "pool_no_self", "chamfer_no_batch_mean" (gradient without 1 / B), "relu_after_bn5".
"""
import numpy as np
import torch
import torch.nn.functional as F

from geometric_adv_amd import fold_weights as FW

EPS = 1e-5
G2 = FW.GRID * FW.GRID
PARAM_KEYS = [k for k in FW.key_names() if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


DTYPE = [torch.float64]          # decisions() runs the same forward in float32


def _t(a):
    return torch.as_tensor(np.asarray(a, np.float64)).to(DTYPE[0])


def forward(P, run, pc, cov, cols, pins=None, perturb=None, tie=0.0):
    """P: {parameter key: float64 tensor in torch's shape}; run: {bn index: [running_mean, running_var]} updated in place.
    Returns (loss, mid_loss, extras)."""
    pins, perturb = pins or {}, perturb or {}
    ex = {"disagree": {}, "relu": {}, "win": [], "hidden": [], "bn_mean": {}, "bn_var": {}}
    B, n = pc.shape[:2]

    def lin(x, k):
        w = P[k + ".weight"]
        return x @ w.reshape(w.shape[0], -1).t() + P[k + ".bias"]

    def note(name, differ, dist):
        differ = np.asarray(differ)
        ex["disagree"][name] = (int(differ.sum()), int(differ.size), float(np.asarray(dist)[differ].max()) if differ.any() else 0.0)

    def bn(a, i, relu=True):
        flat = a.reshape(-1, a.shape[-1])
        rm, rv = run[i]
        ex["bn_mean"][i] = flat.detach().mean(0).numpy()
        ex["bn_var"][i] = flat.detach().var(0, unbiased=False).numpy()
        if perturb.get("bn_no_m2") == i or perturb.get("biased_running_var"):
            m = flat.mean(0)
            v = ((flat - m) ** 2).mean(0)
            rows = flat.shape[0]
            rm.mul_(0.9).add_(0.1 * m.detach())
            rv.mul_(0.9).add_(0.1 * v.detach() * (1.0 if perturb.get("biased_running_var") else rows / (rows - 1.0)))
            if perturb.get("bn_no_m2") == i:
                v = v.detach()
            z = (flat - m) / torch.sqrt(v + EPS) * P["encoder.bn%d.weight" % i] + P["encoder.bn%d.bias" % i]
        else:
            z = F.batch_norm(flat, rm, rv, P["encoder.bn%d.weight" % i], P["encoder.bn%d.bias" % i], training=True,
                             momentum=0.1, eps=EPS)
        z = z.reshape(a.shape)
        if not relu:
            return z
        own = (z.detach() > 0).numpy().reshape(-1, z.shape[-1])
        ex["relu"][i] = own
        if i in pins.get("relu", {}):
            mask = np.asarray(pins["relu"][i], bool).reshape(own.shape)
            note("relu%d" % i, mask != own, z.detach().abs().numpy().reshape(own.shape))
            return z * torch.as_tensor(mask.reshape(z.shape))
        return torch.relu(z)

    ar = torch.arange(B)[:, None, None]

    def pool(h, p):
        c = torch.as_tensor(np.asarray(cols[p], np.int64))                      # (B, n, 16)
        cand_rows = torch.cat([torch.arange(n)[None, :, None].expand(B, n, 1), c], 2)     # (B, n, 17): self, then the slots
        if perturb.get("pool_no_self"):
            cand_rows = c
        hd = h.detach()
        cand = hd[ar, cand_rows]                                                # (B, n, 17, C)
        own_val = cand.max(dim=2)[0]
        first = (cand >= own_val[:, :, None, :] - tie).numpy().argmax(axis=2)   # first maximum
        own = np.take_along_axis(cand_rows.numpy()[:, :, :, None], first[:, :, None, :], 2)[:, :, 0, :]
        own = np.where(own_val.numpy() > 0, own, -1)
        win = own
        if "win" in pins:
            win = np.asarray(pins["win"][p], np.int64).reshape(own.shape)
            at = torch.gather(hd, 1, torch.as_tensor(np.maximum(win, 0))).numpy()
            gap = np.where(win >= 0, own_val.numpy() - at, own_val.numpy())     # how far the pinned element lies below the maximum
            note("win%d" % p, win != own, np.maximum(gap, 0.0))
        ex["win"].append(win)
        w = torch.as_tensor(np.maximum(win, 0))
        out = torch.gather(h, 1, w) * torch.as_tensor(win >= 0)
        if perturb.get("pool_all"):
            nb = h[ar, c].sum(2)
            out = out + (nb - nb.detach())
        return out

    x = torch.cat([_t(pc), _t(cov)], 2)
    for i in (1, 2, 3):
        x = bn(lin(x, "encoder.conv%d" % i), i)
    x = pool(x, 0)
    x = bn(lin(x, "encoder.conv4"), 4)
    x = pool(x, 1)
    y5 = bn(lin(x, "encoder.conv5"), 5, relu=False)
    if perturb.get("relu_after_bn5"):
        y5 = torch.relu(y5)
    yn = y5.detach().numpy()
    own = (yn >= yn.max(axis=1, keepdims=True) - tie).argmax(axis=1)
    row = own
    if "gmax" in pins:
        row = np.asarray(pins["gmax"], np.int64)
        note("gmax", row != own, yn.max(axis=1) - np.take_along_axis(yn, row[:, None, :], 1)[:, 0, :])
    ex["gmax"] = row
    x = torch.gather(y5, 1, torch.as_tensor(row)[:, None, :]).squeeze(1)
    x = bn(lin(x, "encoder.fc1"), 6)
    code = lin(x, "encoder.fc2")
    grid = _t(FW.grid())[None].expand(B, G2, 2)
    rep = code[:, None, :].expand(B, G2, FW.CODE)

    def hidden(z, k):
        own = (z.detach() > 0).numpy().reshape(-1, 512)
        ex["hidden"].append(own)
        if "hidden" in pins:
            mask = np.asarray(pins["hidden"][k], bool).reshape(own.shape)
            note("hidden%d" % k, mask != own, z.detach().abs().numpy().reshape(own.shape))
            return z * torch.as_tensor(mask.reshape(z.shape))
        return torch.relu(z)

    a = hidden(lin(torch.cat([rep, grid], 2), "decoder.fold1.conv1"), 0)
    a = hidden(lin(a, "decoder.fold1.conv2"), 1)
    mid = lin(a, "decoder.fold1.conv3")
    a = hidden(lin(torch.cat([rep, mid], 2), "decoder.fold2.conv1"), 2)
    a = hidden(lin(a, "decoder.fold2.conv2"), 3)
    recon = lin(a, "decoder.fold2.conv3")
    pts = _t(pc)

    def chamfer(r, name, idx=None):
        own1, own2, gap = [], [], 0.0
        with torch.no_grad():
            for b in range(B):
                d = ((pts[b][:, None, :] - r[b][None, :, :]) ** 2).sum(-1)       # (n, 2025)
                own1.append(d.argmin(1).numpy())
                own2.append(d.argmin(0).numpy())
                if idx is not None:
                    g1 = d[torch.arange(n), torch.as_tensor(np.asarray(idx[0][b], np.int64))] - d.min(1)[0]
                    g2 = d[torch.as_tensor(np.asarray(idx[1][b], np.int64)), torch.arange(G2)] - d.min(0)[0]
                    gap = max(gap, float(g1.max()), float(g2.max()))
        own1, own2 = np.stack(own1), np.stack(own2)
        i1, i2 = (own1, own2) if idx is None else (np.asarray(idx[0], np.int64), np.asarray(idx[1], np.int64))
        if idx is not None:
            ex["disagree"][name] = (int((i1 != own1).sum() + (i2 != own2).sum()), int(i1.size + i2.size), gap)
        d1 = ((pts - torch.gather(r, 1, torch.as_tensor(i1)[:, :, None].expand(B, n, 3))) ** 2).sum(-1)
        d2 = ((r - torch.gather(pts, 1, torch.as_tensor(i2)[:, :, None].expand(B, G2, 3))) ** 2).sum(-1)
        per_cloud = d1.mean(1) + d2.mean(1)
        return per_cloud.sum() if perturb.get("chamfer_no_batch_mean") else per_cloud.mean(), (i1, i2)

    loss, ex["chamfer"] = chamfer(recon, "chamfer", pins.get("chamfer"))
    with torch.no_grad():
        mid_loss, _ = chamfer(mid.detach(), "chamfer_mid")
        if perturb.get("chamfer_no_batch_mean"):
            mid_loss = mid_loss / B
    ex.update(code=code.detach().numpy(), mid=mid.detach().numpy(), recon=recon.detach().numpy())
    return loss, float(mid_loss), ex


def decisions(state, pc, cov, cols, dtype=torch.float64):
    """The forward's discrete decisions in the given precision: {"relu<i>", "win<p>", "gmax", "hidden<k>": array}."""
    DTYPE[0] = dtype
    try:
        with torch.no_grad():
            P = {k: _t(state[k]) for k in PARAM_KEYS}
            run = {i: [_t(state["encoder.bn%d.running_mean" % i]).clone(), _t(state["encoder.bn%d.running_var" % i]).clone()]
                   for i in range(1, 7)}
            _, _, ex = forward(P, run, np.asarray(pc, np.float64), cov, cols)
    finally:
        DTYPE[0] = torch.float64
    out = {"relu%d" % i: m for i, m in ex["relu"].items()}
    out.update({"win%d" % p: w for p, w in enumerate(ex["win"])})
    out.update({"hidden%d" % k: m for k, m in enumerate(ex["hidden"])})
    out["gmax"] = ex["gmax"]
    return out


def step(state, pc, cov, cols, lr=1e-4, weight_decay=1e-6, steps_done=0, slots=None, pins=None, perturb=None, tie=0.0):
    """One training step in float64.  state: {state-dict key: array} (running statistics included); slots: {key: (exp_avg,
    exp_avg_sq)} of the PARAM_KEYS, None = fresh.  Returns a dict: loss, mid_loss, code, mid, recon, grads {key: array},
    new_state, slots, bn_mean / bn_var {bn index: array}, relu / win / gmax / hidden / chamfer (the decisions used) and
    disagree."""
    perturb = perturb or {}
    P = {k: _t(state[k]).clone().requires_grad_(True) for k in PARAM_KEYS}
    run = {i: [_t(state["encoder.bn%d.running_mean" % i]).clone(), _t(state["encoder.bn%d.running_var" % i]).clone()]
           for i in range(1, 7)}
    loss, mid_loss, ex = forward(P, run, np.asarray(pc, np.float64), cov, cols, pins, perturb, tie)
    loss.backward()
    grads = {k: P[k].grad.numpy().copy() for k in PARAM_KEYS}
    wd = 0.0 if perturb.get("no_weight_decay") else weight_decay
    new_slots = {}
    if perturb.get("tf_adam_eps"):
        t = steps_done + 1
        alpha = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        new = {}
        for k in PARAM_KEYS:
            p = P[k].detach().numpy()
            g = grads[k] + wd * p
            m0, v0 = slots[k] if slots else (0.0, 0.0)
            m, v = 0.9 * m0 + 0.1 * g, 0.999 * v0 + 0.001 * g * g
            new_slots[k] = (m, v)
            new[k] = p - alpha * m / (np.sqrt(v) + 1e-8)
    else:
        params = [P[k] for k in PARAM_KEYS]
        opt = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.999), weight_decay=wd)
        if slots is not None:
            sd = opt.state_dict()
            sd["state"] = {i: {"step": torch.tensor(float(steps_done)), "exp_avg": _t(slots[k][0]).clone(),
                               "exp_avg_sq": _t(slots[k][1]).clone()} for i, k in enumerate(PARAM_KEYS)}
            opt.load_state_dict(sd)
        opt.step()
        new = {k: P[k].detach().numpy().copy() for k in PARAM_KEYS}
        new_slots = {k: (opt.state[P[k]]["exp_avg"].numpy().copy(), opt.state[P[k]]["exp_avg_sq"].numpy().copy())
                     for k in PARAM_KEYS}
    for i in range(1, 7):
        new["encoder.bn%d.running_mean" % i] = run[i][0].numpy()
        new["encoder.bn%d.running_var" % i] = run[i][1].numpy()
    out = dict(loss=float(loss.item()) / (len(pc) if perturb.get("chamfer_no_batch_mean") else 1), mid_loss=mid_loss, grads=grads,
               new_state=new, slots=new_slots)
    out.update(ex)
    return out
