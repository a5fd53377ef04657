"""float64 yardstick of the classifier's input gradient (csrc/cls_grad.hip): the graph of tests/_cls_model64.py in torch
autograd, every max pool written as an explicit gather at its winner rows -- the model's own FIRST arg-max (found with
numpy, not torch's pooling tie rule) or rows handed in -- and the three logit losses of include/geoadv.h written with their
sub-gradient rules spelled out.  `dtype` runs the same graph in float32 (the measurement behind the GPU tolerance);
detach_transforms=True holds T1 and T2 constant (the guard that the tests can tell a gradient without the T-Net paths).

grad_model also returns, per cloud, the DECISION MARGINS: the smallest normalised distance from a discontinuity of the
gradient --
  relu: |pre-activation| / max |pre-activation of that layer in the cloud|, over the units on a winner row's path (the
        per-point layers under each pool at that pool's winner rows, and the fc1 / fc2 units of the three heads); also per
        layer (margin_layers), for a caller that knows each layer's forward error;
  pool: (winner - best value on ANOTHER point) / max of the pooled layer, over the columns with a positive maximum;
  loss: the CW max against its runner-up among the other classes, and against the clamp -kappa, over max |Z|.

A unit that close to zero can be masked the other way by a float32 forward.  relu_override pins the DERIVATIVE of named units
(the forward value stays relu(pre)), and open_units lists the units of a result that lie inside a window, so that a caller
can resolve such a unit -- try it the other way -- instead of leaving the whole cloud out.  `mutate` builds deliberately
wrong gradients of the same forward (what a kernel that drops part of a dW sum would give): the comparison's own test."""
import numpy as np
import torch

EPS = 1e-3
EMA = "%s/bn/%s/bn/moments/%s/ExponentialMovingAverage"
LOSSES = ("xent", "cw_targeted", "cw_untargeted")
# the per-point layers under each pool (their units at the pool's winner rows are on a gradient path), and the head layers
UNDER = {0: ["transform_net1/tconv1", "transform_net1/tconv2"],
         1: ["conv1", "conv2", "transform_net2/tconv1", "transform_net2/tconv2"],
         2: ["conv1", "conv2", "conv3", "conv4"]}
HEADS = ("transform_net1/tfc1", "transform_net1/tfc2", "transform_net2/tfc1", "transform_net2/tfc2", "fc1", "fc2")


def first_argmax(values, axis):
    """numpy: the lowest index among equal maxima along `axis`."""
    v = np.asarray(values)
    return (v == v.max(axis=axis, keepdims=True)).argmax(axis=axis)


def cw_other_max(Z, labels):
    """numpy (b, C) -> (j, m): the FIRST maximum over i != labels[c] and its index."""
    Z = np.asarray(Z, np.float64)
    masked = Z.copy()
    masked[np.arange(len(Z)), labels] = -np.inf
    j = first_argmax(masked, 1)
    return j, Z[np.arange(len(Z)), j]


def loss_numpy(Z, labels, loss="xent", kappa=0.0):
    """The per-cloud loss of float64 logits, numpy only (the finite-difference side)."""
    Z = np.asarray(Z, np.float64)
    labels = np.asarray(labels)
    r = np.arange(len(Z))
    if loss == "xent":
        m = Z.max(1, keepdims=True)
        return np.log(np.exp(Z - m).sum(1)) + m[:, 0] - Z[r, labels]
    _, m = cw_other_max(Z, labels)
    diff = m - Z[r, labels] if loss == "cw_targeted" else Z[r, labels] - m
    return np.maximum(diff, -float(kappa))


def loss_torch(Z, labels, loss="xent", kappa=0.0):
    """(loss (b,), active (b,) bool) of torch logits with the header's sub-gradient rules: the CW kinds differentiate through
    the first maximum over the other classes only, and only where the unclamped value is strictly above -kappa."""
    b = Z.shape[0]
    r = torch.arange(b)
    y = torch.as_tensor(np.asarray(labels, np.int64))
    if loss == "xent":
        return torch.logsumexp(Z, 1) - Z[r, y], np.ones(b, bool)
    j, _ = cw_other_max(Z.detach().numpy(), np.asarray(labels))
    m = Z[r, torch.as_tensor(j)]
    diff = m - Z[r, y] if loss == "cw_targeted" else Z[r, y] - m
    active = diff.detach() > -float(kappa)
    floor = torch.full_like(diff, -float(kappa))
    return torch.where(active, diff, floor), active.numpy()


class ModelClassifier:
    """The float64 model behind PointNetClassifier's interface, as far as cls_attack uses it: the host stand-in with which the
    attack tests' sources, targets and parameters were chosen on the CPU."""
    device, dtype = torch.device("cpu"), torch.float64

    def __init__(self, weights, batch_size=4):
        self.w, self.batch_size = weights, batch_size
        self.num_classes = int(np.asarray(weights["fc3/weights"]).shape[-1])

    def input_gradient(self, x, labels, loss="xent", kappa=0.0, return_logits=False, return_winners=False):
        r = grad_model(self.w, x.numpy(), labels.numpy(), loss, kappa)
        out = (torch.as_tensor(r["loss"]), torch.as_tensor(r["grad"]))
        return out + ((torch.as_tensor(r["logits"]),) if return_logits else ())


def winner_rows(ref, c, p):
    """The distinct rows of cloud c that win a live (positive) column of pool p, ascending: the op's slots."""
    return np.unique(ref["winners"][c, p][ref["pooled"][c, p] > 0])


def open_units(ref, window):
    """Sorted [(scope, cloud, row, unit)] of a grad_model result: the units on a gradient path with |pre| / max |pre of that
    layer in the cloud| <= window[scope] (a dict, or one number for all layers) -- the per-point layers of UNDER at each
    pool's winner rows (a unit under two pools is listed once), and the head layers of HEADS with row None."""
    win_of = (lambda s: window[s]) if isinstance(window, dict) else (lambda s: window)
    found = set()
    for c in range(len(ref["loss"])):
        for p in range(3):
            rows = winner_rows(ref, c, p)
            for s in UNDER[p]:
                a = np.abs(ref["pres"][s][c])
                scale = a.max()
                if not len(rows) or not scale > 0:
                    continue
                r, u = np.nonzero(a[rows] / scale <= win_of(s))
                found.update((s, c, int(rows[i]), int(j)) for i, j in zip(r, u))
        for s in HEADS:
            a = np.abs(ref["pres"][s][c])
            if a.max() > 0:
                found.update((s, c, None, int(j)) for j in np.nonzero(a / a.max() <= win_of(s))[0])
    return sorted(found, key=lambda k: (k[0], k[1], -1 if k[2] is None else k[2], k[3]))


def grad_model(w, pc, labels, loss="xent", kappa=0.0, winners=None, dtype=torch.float64, detach_transforms=False,
               relu_override=None, mutate=None, margins=True):
    """dict(loss (b,), grad (b, n, 3), logits (b, C), winners (b, 3, 1024) int64, pooled (b, 3, 1024), columns (3 x (b, n, 1024):
    the pooled layers before the pool), margin_relu / margin_pool / margin_loss / margin (b,)) as numpy arrays.
    relu_override {scope: [(cloud, row or None, unit, on), ...] or a boolean array of the layer's shape}: the derivative
    [pre > 0] of those units is replaced by `on`; the forward value is untouched (straight-through).
    mutate {"dw3_drop_rows": per cloud the rows left out of dW3' = h2^T g, "dw1_drop_pool1": True to leave pool 1's path
    out of dW1' = x^T g}: wrong gradients of the same forward.
    margins=False leaves the margin_* entries out (most of a run's time at thousands of points)."""
    assert loss in LOSSES
    relu_override, mutate = relu_override or {}, mutate or {}
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)
    x = torch.as_tensor(np.asarray(pc, np.float64)).to(dtype).requires_grad_(True)
    b, n = x.shape[0], x.shape[1]
    pres = {}

    def layer(h, scope, relu=True):
        W = T(w[scope + "/weights"])
        a = h @ W.reshape(-1, W.shape[-1]) + T(w[scope + "/biases"])
        if not relu:
            return a
        inv = T(w[scope + "/bn/gamma"]) / torch.sqrt(T(w[EMA % (scope, scope, "Squeeze_1")]) + EPS)
        pre = a * inv + (T(w[scope + "/bn/beta"]) - T(w[EMA % (scope, scope, "Squeeze")]) * inv)
        pres[scope] = pre.detach().numpy().astype(np.float64, copy=False)
        ov = relu_override.get(scope)
        if ov is None:
            return torch.relu(pre)
        own = pre.detach() > 0
        if isinstance(ov, np.ndarray) or torch.is_tensor(ov):
            on = torch.as_tensor(np.asarray(ov, bool)).reshape(own.shape)
        else:
            on = own.clone()
            for c, row, unit, val in ov:
                on[(c, unit) if row is None else (c, row, unit)] = bool(val)
        return torch.relu(pre) + (on.to(dtype) - own.to(dtype)) * (pre - pre.detach())

    got_winners, pooled_vals, columns = [], [], []

    def pool(h, p):
        hv = h.detach().numpy()
        idx = first_argmax(hv, 1) if winners is None else np.asarray(winners)[:, p].astype(np.int64)
        got_winners.append(np.where(hv.max(1) > 0, idx, 0) if winners is None else idx)
        columns.append(hv.astype(np.float64, copy=False))
        out = torch.gather(h, 1, torch.as_tensor(idx)[:, None, :])[:, 0]
        pooled_vals.append(out.detach().numpy().astype(np.float64, copy=False))
        return out

    def tnet(h, prefix, last, K, p):
        for s in ("tconv1", "tconv2", "tconv3"):
            h = layer(h, prefix + "/" + s)
        h = pool(h, p)
        for s in ("tfc1", "tfc2"):
            h = layer(h, prefix + "/" + s)
        t = (layer(h, prefix + "/" + last, relu=False) + torch.eye(K, dtype=dtype).flatten()).view(-1, K, K)
        return t.detach() if detach_transforms else t

    t1 = tnet(x, "transform_net1", "transform_XYZ", 3, 0)
    h = torch.bmm(x, t1)
    for s in ("conv1", "conv2"):
        h = layer(h, s)
    h_t2 = h
    if mutate.get("dw1_drop_pool1"):                # T-Net2's input: the same values, T1 held constant
        h_t2 = torch.bmm(x, t1.detach())
        for s in ("conv1", "conv2"):
            h_t2 = layer(h_t2, s)
    t2 = tnet(h_t2, "transform_net2", "transform_feat", 64, 1)
    if mutate.get("dw3_drop_rows") is not None:     # those rows see T2 as a constant
        cut = torch.zeros((b, n, 1), dtype=torch.bool)
        for c, r in enumerate(mutate["dw3_drop_rows"]):
            cut[c, np.asarray(r, np.int64)] = True
        h = torch.where(cut, torch.bmm(h, t2.detach()), torch.bmm(h, t2))
    else:
        h = torch.bmm(h, t2)
    for s in ("conv3", "conv4", "conv5"):
        h = layer(h, s)
    h = pool(h, 2)
    for s in ("fc1", "fc2"):
        h = layer(h, s)
    Z = layer(h, "fc3", relu=False)
    L, active = loss_torch(Z, labels, loss, kappa)
    L.sum().backward()
    win = np.stack(got_winners, 1)
    result = dict(loss=L.detach().numpy(), grad=x.grad.numpy(), logits=Z.detach().numpy(), winners=win,
                  pooled=np.stack(pooled_vals, 1), columns=columns, active=active, pres=pres)
    if not margins:
        return result

    # ---- decision margins (meaningful in float64)
    def rel(pre, rows=None):                       # per cloud: min |pre| / max |pre| over the given rows
        out = np.full(b, np.inf)
        for c in range(b):
            a = np.abs(pre[c])
            scale = a.max()
            if rows is not None:
                a = a[rows[c]]
            if a.size and scale > 0:
                out[c] = a.min() / scale
        return out

    live = [pooled_vals[p] > 0 for p in range(3)]
    rows = [[np.unique(win[c, p][live[p][c]]) for c in range(b)] for p in range(3)]
    m_layers = {}
    for p in range(3):
        for s in UNDER[p]:
            m_layers[s] = np.minimum(m_layers.get(s, np.inf), rel(pres[s], rows[p]))
    for s in HEADS:
        m_layers[s] = rel(pres[s])
    m_relu = np.min(np.stack(list(m_layers.values())), axis=0)
    m_pool = np.full(b, np.inf)
    if n > 1:
        for p in range(3):
            col = columns[p]
            for c in range(b):
                k = np.nonzero(live[p][c])[0]
                if not len(k):
                    continue
                v = col[c][:, k].copy()
                top = v[win[c, p][k], np.arange(len(k))]
                v[win[c, p][k], np.arange(len(k))] = -np.inf
                m_pool[c] = min(m_pool[c], float(((top - v.max(0)) / col[c].max()).min()))
    m_loss = np.full(b, np.inf)
    if loss != "xent":
        Zn = Z.detach().numpy().astype(np.float64)
        y = np.asarray(labels)
        j, m = cw_other_max(Zn, y)
        r = np.arange(b)
        diff = m - Zn[r, y] if loss == "cw_targeted" else Zn[r, y] - m
        scale = np.abs(Zn).max(1)
        m_loss = np.abs(diff + float(kappa)) / scale
        if Zn.shape[1] > 2:
            rest = Zn.copy()
            rest[r, y] = -np.inf
            rest[r, j] = -np.inf
            m_loss = np.minimum(m_loss, (m - rest.max(1)) / scale)
    result.update(margin_layers=m_layers, margin_relu=m_relu, margin_pool=m_pool, margin_loss=m_loss,
                  margin=np.minimum(np.minimum(m_relu, m_pool), m_loss))
    return result
