"""float64 model of ONE AtlasNet training step (csrc/atlas_train.hip restated), hand-derived in numpy: the train-mode forward
of the PointNet encoder and the nb Mapping2Dto3D decoders, fuse_primitives, the Chamfer loss, every gradient written out, the
running statistics and torch-form Adam.  Only the matrix products go through torch (CPU), in the model's dtype.

    res = step(state, pc, tmpl, num_layers)          # state: {key without `module.`: array}, tmpl (nb, p, 2)

The rules a framework would pick by itself are written out: the maximum over points takes the FIRST maximal row; Chamfer's
nearest neighbours are found first (first minimum) and the loss is gathered at them; a decoder batch norm takes its
statistics per primitive over batch x p rows.

Pins: the step's discrete decisions can be fixed to given ones instead of fp64's own --
  pins["relu"]["enc1" | "enc2" | "enc4" | "enc5"]   bool [rows][C]         ReLU mask after the encoder's bn1, bn2, bn4, bn5
  pins["relu"]["dec<l>"]                            bool [nb][B * p][C]    ReLU mask of decoder layer l (0 = conv1, 1 = conv2, ...)
  pins["gmax"]                                      int [B][1024]          the maximum's row
  pins["chamfer"]                                   (int [B][n], int [B][nb * p])
Pinning fp64's own decisions reproduces the unpinned step.  res["disagree"][name] = (pins that differ from fp64's own, number
of pins, the largest fp64 distance from its boundary of a differing pin: |ReLU input|, or own maximum minus the pinned row's
value, or pinned distance minus the smallest).

perturb (tests only) restates the step wrongly: "tf_adam_eps" (sqrt(v) + eps before the bias correction),
"biased_running_var", "bn_no_m2" = name (that norm's backward without its xhat * mean(dy xhat) term; names "enc1" ..
"enc5", "dec<l>"), "chamfer_no_batch_mean" (the gradient without 1 / B), "chamfer_same_count" (both directions' means over
the input's point count, where the reconstruction has another), "dec_bn1_var_t_only" (the
decoder's bn1 variance without the latent's var_b z), "dec_stats_over_all_primitives" (one set of statistics per decoder layer).
"""
import numpy as np
import torch

from geometric_adv_amd import atlas_weights as AW

EPS = 1e-5


def param_keys(state, nb, num_layers):
    return AW.parameter_names(nb, num_layers, AW.has_decoder_bn(state))


def _mm(a, b):
    return (torch.from_numpy(np.ascontiguousarray(a)) @ torch.from_numpy(np.ascontiguousarray(b))).numpy()


class _Net:
    """One forward (and, in float64, backward) over caches."""

    def __init__(self, state, num_layers, dtype, pins, perturb):
        self.s = {k: np.asarray(v, dtype) for k, v in state.items() if not k.endswith("num_batches_tracked")}
        self.L, self.dt, self.pins, self.pb = num_layers, dtype, pins or {}, perturb or {}
        self.dbn = AW.has_decoder_bn(state)
        self.disagree, self.relu, self.bn_mean, self.bn_var, self.run = {}, {}, {}, {}, {}
        self.grads = {}

    def W(self, k):
        w = self.s[k + ".weight"]
        return w.reshape(w.shape[0], -1)

    def lin(self, x, k):
        return _mm(x, self.W(k).T) + self.s[k + ".bias"]

    def note(self, name, differ, dist):
        differ = np.asarray(differ)
        self.disagree[name] = (int(differ.sum()), int(differ.size), float(np.asarray(dist)[differ].max()) if differ.any() else 0.0)

    # a (rows, C) -> y, cache; bn: state prefix, name: the statistics' label, stats: (mean, var, rows) given instead of a's own
    def bn_fwd(self, a, bn, name, stats=None):
        m, v, rows = stats if stats is not None else (a.mean(0), a.var(0), a.shape[0])
        self.bn_mean[name], self.bn_var[name] = m, v
        scale = 1.0 if self.pb.get("biased_running_var") else rows / (rows - 1.0)
        self.run[bn + ".running_mean"] = 0.9 * self.s[bn + ".running_mean"] + 0.1 * m
        self.run[bn + ".running_var"] = 0.9 * self.s[bn + ".running_var"] + 0.1 * v * scale
        rs = 1.0 / np.sqrt(v + self.dt(EPS))
        xh = (a - m) * rs
        return xh * self.s[bn + ".weight"] + self.s[bn + ".bias"], (xh, rs)

    def bn_bwd(self, dy, cache, bn, name):
        xh, rs = cache
        self.grads[bn + ".weight"] = (dy * xh).sum(0)
        self.grads[bn + ".bias"] = dy.sum(0)
        m2 = 0.0 if self.pb.get("bn_no_m2") == name else (dy * xh).mean(0)
        return self.s[bn + ".weight"] * rs * (dy - dy.mean(0) - xh * m2)

    def relu_fwd(self, y, name, group=None):
        own = y > 0
        mask = own
        pin = self.pins.get("relu", {}).get(name)
        if pin is not None:
            mask = np.asarray(pin, bool)
            mask = (mask[group] if group is not None else mask).reshape(own.shape)
            if group is None:
                self.note("relu_" + name, mask != own, np.abs(y))
            else:
                c0, t0, d0 = self.disagree.get("relu_" + name, (0, 0, 0.0))
                differ = mask != own
                self.disagree["relu_" + name] = (c0 + int(differ.sum()), t0 + differ.size,
                                                 max(d0, float(np.abs(y)[differ].max()) if differ.any() else 0.0))
        if group is None:
            self.relu[name] = mask
        else:
            self.relu.setdefault(name, {})[group] = mask
        return y * mask, mask

    def lin_bwd(self, k, x, da, conv, need_dx=True):
        w = self.s[k + ".weight"]
        self.grads[k + ".weight"] = _mm(da.T, x).reshape(w.shape)
        self.grads[k + ".bias"] = da.sum(0)
        return _mm(da, self.W(k)) if need_dx else None


def run(state, pc, tmpl, num_layers, dtype=np.float64, pins=None, perturb=None, backward=True):
    """The forward (and backward).  Returns the _Net with loss, latent, recon, grads (if backward), run (new running
    statistics), relu / gmax / chamfer (the decisions used), bn_mean / bn_var and disagree."""
    N = _Net(state, num_layers, dtype, pins, perturb)
    pb, L = N.pb, num_layers
    pc = np.asarray(pc, dtype)
    tmpl = np.asarray(tmpl, dtype)
    B, n = pc.shape[:2]
    nb, p = tmpl.shape[:2]
    m = nb * p
    e = "encoder."
    # ---- encoder ----
    x0 = pc.reshape(B * n, 3)
    y1, c1 = N.bn_fwd(N.lin(x0, e + "conv1"), e + "bn1", "enc1")
    h1, k1 = N.relu_fwd(y1, "enc1")
    y2, c2 = N.bn_fwd(N.lin(h1, e + "conv2"), e + "bn2", "enc2")
    h2, k2 = N.relu_fwd(y2, "enc2")
    y3, c3 = N.bn_fwd(N.lin(h2, e + "conv3"), e + "bn3", "enc3")
    y3 = y3.reshape(B, n, -1)
    own = y3.argmax(axis=1)
    row = own
    if "gmax" in N.pins:
        row = np.asarray(N.pins["gmax"], np.int64)
        N.note("gmax", row != own, y3.max(axis=1) - np.take_along_axis(y3, row[:, None, :], 1)[:, 0, :])
    N.gmax = row
    pooled = np.take_along_axis(y3, row[:, None, :], 1)[:, 0, :]
    y4, c4 = N.bn_fwd(N.lin(pooled, e + "lin1"), e + "bn4", "enc4")
    h4, k4 = N.relu_fwd(y4, "enc4")
    y5, c5 = N.bn_fwd(N.lin(h4, e + "lin2"), e + "bn5", "enc5")
    z, k5 = N.relu_fwd(y5, "enc5")
    N.latent = z
    # ---- decoders ----
    names = AW.dec_layers(L)
    recon = np.zeros((B, m, 3), dtype)
    caches = []
    pooled_stats = {}
    if pb.get("dec_stats_over_all_primitives") and N.dbn:
        # the mistake: statistics over every primitive's rows at once (a forward per layer to get them)
        acts = []
        for q in range(nb):
            d = "decoder.decoder.%d." % q
            t1 = _mm(tmpl[q], N.W(d + "conv1").T) + N.s[d + "conv1.bias"]
            acts.append((t1[None] + z[:, None, :]).reshape(B * p, -1))
        for li in range(2 + L):
            allr = np.concatenate(acts)
            pooled_stats[li] = (allr.mean(0), allr.var(0), allr.shape[0])
            if li == 1 + L:
                break
            nxt = []
            for q in range(nb):
                d = "decoder.decoder.%d." % q
                bn = d + names[li][3]
                y = (acts[q] - pooled_stats[li][0]) / np.sqrt(pooled_stats[li][1] + EPS) * N.s[bn + ".weight"] + N.s[bn + ".bias"]
                nxt.append(N.lin(np.maximum(y, 0), d + names[li + 1][0]))
            acts = nxt
    for q in range(nb):
        d = "decoder.decoder.%d." % q
        t1 = _mm(tmpl[q], N.W(d + "conv1").T) + N.s[d + "conv1.bias"]                  # (p, 1024)
        a = (t1[None] + z[:, None, :]).reshape(B * p, -1)
        cq = []
        hin = None
        for li in range(2 + L):
            name, _, _, bnn = names[li]
            if li > 0:
                a = N.lin(hin, d + name)
            cache = None
            if N.dbn:
                stats = pooled_stats.get(li)
                if li == 0 and stats is None:
                    # over the grid (b, j): mean = mean_j t1 + mean_b z, variance = var_j t1 + var_b z
                    vt = t1.var(0) if pb.get("dec_bn1_var_t_only") else t1.var(0) + z.var(0)
                    stats = (t1.mean(0) + z.mean(0), vt, B * p)
                y, cache = N.bn_fwd(a, d + bnn, "dec%d.%d" % (li, q), stats)
            else:
                y = a
            h, mask = N.relu_fwd(y, "dec%d" % li, q)
            cq.append((hin, cache, mask))
            hin = h
        out = N.lin(hin, d + "last_conv")                                          # (B * p, 3)
        recon[:, q * p:(q + 1) * p] = out.reshape(B, p, 3)
        caches.append((cq, hin))
    N.recon = recon
    # ---- Chamfer ----
    own1, own2 = np.zeros((B, n), np.int64), np.zeros((B, m), np.int64)
    gap = 0.0
    idx = N.pins.get("chamfer")
    for b in range(B):
        dm = ((pc[b][:, None, :] - recon[b][None, :, :]) ** 2).sum(-1)            # (n, m)
        own1[b], own2[b] = dm.argmin(1), dm.argmin(0)
        if idx is not None:
            g1 = dm[np.arange(n), np.asarray(idx[0][b], np.int64)] - dm.min(1)
            g2 = dm[np.asarray(idx[1][b], np.int64), np.arange(m)] - dm.min(0)
            gap = max(gap, float(g1.max()), float(g2.max()))
    i1, i2 = (own1, own2) if idx is None else (np.asarray(idx[0], np.int64), np.asarray(idx[1], np.int64))
    if idx is not None:
        N.disagree["chamfer"] = (int((i1 != own1).sum() + (i2 != own2).sum()), int(i1.size + i2.size), gap)
    N.chamfer = (i1, i2)
    r1 = np.take_along_axis(recon, i1[:, :, None], 1)                              # nearest recon point of every input point
    x2 = np.take_along_axis(pc, i2[:, :, None], 1)                                 # nearest input point of every recon point
    N.loss = float(((pc - r1) ** 2).sum(-1).mean() + ((recon - x2) ** 2).sum(-1).mean())
    if not backward:
        return N
    # ---- backward ----
    s1 = 1.0 / n if pb.get("chamfer_no_batch_mean") else 1.0 / (B * n)
    s2 = 1.0 / m if pb.get("chamfer_no_batch_mean") else 1.0 / (B * (n if pb.get("chamfer_same_count") else m))
    drecon = 2.0 * (recon - x2) * s2
    g1 = 2.0 * (r1 - pc) * s1
    for b in range(B):
        np.add.at(drecon[b], i1[b], g1[b])
    dz = np.zeros_like(z)
    for q in range(nb):
        d = "decoder.decoder.%d." % q
        cq, hlast = caches[q]
        dh = N.lin_bwd(d + "last_conv", hlast, np.ascontiguousarray(drecon[:, q * p:(q + 1) * p]).reshape(B * p, 3), True)
        for li in range(1 + L, -1, -1):
            name, _, _, bnn = names[li]
            hin, cache, mask = cq[li]
            dy = dh * mask
            da = N.bn_bwd(dy, cache, d + bnn, "dec%d" % li) if N.dbn else dy
            if li > 0:
                dh = N.lin_bwd(d + name, hin, da, True)
            else:
                dpre = da.reshape(B, p, -1)
                dz += dpre.sum(1)
                dt1 = dpre.sum(0)                                                  # (p, 1024)
                N.grads[d + "conv1.weight"] = _mm(dt1.T, tmpl[q]).reshape(N.s[d + "conv1.weight"].shape)
                N.grads[d + "conv1.bias"] = dt1.sum(0)
    da5 = N.bn_bwd(dz * k5, c5, e + "bn5", "enc5")
    dh4 = N.lin_bwd(e + "lin2", h4, da5, False)
    da4 = N.bn_bwd(dh4 * k4, c4, e + "bn4", "enc4")
    dpooled = N.lin_bwd(e + "lin1", pooled, da4, False)
    dy3 = np.zeros((B, n, dpooled.shape[1]), dtype)
    np.put_along_axis(dy3, row[:, None, :], dpooled[:, None, :], 1)
    dy3 = dy3.reshape(B * n, -1)
    da3 = N.bn_bwd(dy3, c3, e + "bn3", "enc3")
    dh2 = N.lin_bwd(e + "conv3", h2, da3, True)
    da2 = N.bn_bwd(dh2 * k2, c2, e + "bn2", "enc2")
    dh1 = N.lin_bwd(e + "conv2", h1, da2, True)
    da1 = N.bn_bwd(dh1 * k1, c1, e + "bn1", "enc1")
    N.lin_bwd(e + "conv1", x0, da1, True, need_dx=False)
    return N


def decisions(state, pc, tmpl, num_layers, dtype=np.float64):
    """The forward's discrete decisions in the given precision: {"relu_enc1", ..., "relu_dec<l>", "gmax": array}."""
    N = run(state, pc, tmpl, num_layers, dtype=dtype, backward=False)
    out = {"gmax": N.gmax}
    for k, v in N.relu.items():
        out["relu_" + k] = np.stack([v[q] for q in sorted(v)]) if isinstance(v, dict) else v
    return out


def adam(p, g, m0, v0, t, lr, tf_eps=False):
    """torch.optim.Adam's update at its step t (1-based): betas .9 / .999, eps 1e-8 outside the square root, after the bias
    correction of the second moment."""
    m = m0 + (g - m0) * 0.1
    v = 0.999 * v0 + 0.001 * g * g
    if tf_eps:
        return p - lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-8), m, v
    return p - lr / (1 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8), m, v


def step(state, pc, tmpl, num_layers, lr=1e-3, steps_done=0, slots=None, pins=None, perturb=None):
    """One training step in float64.  slots: {key: (exp_avg, exp_avg_sq)}, None = fresh.  Returns a dict: loss, latent, recon,
    grads {key: array}, new_state, slots, bn_mean / bn_var {label: array}, relu / gmax / chamfer (the decisions used), disagree."""
    perturb = perturb or {}
    N = run(state, pc, tmpl, num_layers, pins=pins, perturb=perturb)
    nb = len(tmpl)
    keys = param_keys(state, nb, num_layers)
    new, new_slots = {}, {}
    for k in keys:
        p0 = np.asarray(state[k], np.float64)
        m0, v0 = slots[k] if slots else (np.zeros_like(p0), np.zeros_like(p0))
        new[k], mm, vv = adam(p0, N.grads[k].reshape(p0.shape), np.asarray(m0, np.float64).reshape(p0.shape),
                              np.asarray(v0, np.float64).reshape(p0.shape), steps_done + 1, lr, bool(perturb.get("tf_adam_eps")))
        new_slots[k] = (mm, vv)
    new.update(N.run)
    relu = {k: (np.stack([v[q] for q in sorted(v)]) if isinstance(v, dict) else v) for k, v in N.relu.items()}
    return dict(loss=N.loss, latent=N.latent, recon=N.recon, grads={k: N.grads[k].reshape(np.shape(state[k])) for k in keys},
                new_state=new, slots=new_slots, bn_mean=N.bn_mean, bn_var=N.bn_var, relu=relu, gmax=N.gmax, chamfer=N.chamfer,
                disagree=N.disagree)
