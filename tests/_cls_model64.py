"""float64 oracle of the PointNet classifier (classifier/pointnet_cls.py:30-84, transform_nets.py), written twice and
independently from the graph -- once in numpy, once with torch.nn.functional in float64 -- the way the auto-encoder has two
models.  Both take the variables by their TF names (geometric_adv_amd.cls_weights.variable_names).

transpose=True multiplies by T1^T / T2^T instead of T1 / T2 (a test that the GPU results can tell the two apart);
with_transforms=False drops both transforms (the identity test)."""
import numpy as np

EPS = 1e-3
EMA = "%s/bn/%s/bn/moments/%s/ExponentialMovingAverage"


# ------------------------------------------------------------------------------------------------ numpy
def _np_dense(x, w, scope):
    W = np.asarray(w[scope + "/weights"], np.float64)
    W = W.reshape(-1, W.shape[-1])                       # conv2d W[1, kw, Cin, Cout] -> [kw * Cin, Cout]
    return x @ W + np.asarray(w[scope + "/biases"], np.float64)


def _np_bn_relu(x, w, scope):
    g, b = (np.asarray(w["%s/bn/%s" % (scope, k)], np.float64) for k in ("gamma", "beta"))
    m = np.asarray(w[EMA % (scope, scope, "Squeeze")], np.float64)
    v = np.asarray(w[EMA % (scope, scope, "Squeeze_1")], np.float64)
    inv = 1.0 / np.sqrt(v + EPS) * g                      # tf.nn.batch_normalization
    return np.maximum(x * inv + (b - m * inv), 0.0)


def _np_tnet(x, w, p, last, K):
    h = x
    for s in ("tconv1", "tconv2", "tconv3"):
        h = _np_bn_relu(_np_dense(h, w, p + "/" + s), w, p + "/" + s)
    h = h.max(axis=1)
    for s in ("tfc1", "tfc2"):
        h = _np_bn_relu(_np_dense(h, w, p + "/" + s), w, p + "/" + s)
    W = np.asarray(w[p + "/" + last + "/weights"], np.float64)
    bias = np.asarray(w[p + "/" + last + "/biases"], np.float64) + np.eye(K).flatten()
    return (h @ W + bias).reshape(len(h), K, K)


def numpy_model(w, pc, transpose=False, with_transforms=True):
    """(logits (b, C), T1 (b, 3, 3), T2 (b, 64, 64)) in float64."""
    x = np.asarray(pc, np.float64)
    t1 = _np_tnet(x, w, "transform_net1", "transform_XYZ", 3)
    if transpose:
        t1 = t1.transpose(0, 2, 1)
    h = np.matmul(x, t1) if with_transforms else x
    for s in ("conv1", "conv2"):
        h = _np_bn_relu(_np_dense(h, w, s), w, s)
    t2 = _np_tnet(h, w, "transform_net2", "transform_feat", 64)
    if transpose:
        t2 = t2.transpose(0, 2, 1)
    if with_transforms:
        h = np.matmul(h, t2)
    for s in ("conv3", "conv4", "conv5"):
        h = _np_bn_relu(_np_dense(h, w, s), w, s)
    h = h.max(axis=1)
    for s in ("fc1", "fc2"):
        h = _np_bn_relu(_np_dense(h, w, s), w, s)
    return _np_dense(h, w, "fc3"), t1, t2


# ------------------------------------------------------------------------------------------------ torch.nn.functional
def torch_model(w, pc):
    """The same graph as conv2d / linear / batch_norm modules of torch.nn.functional in float64 (NCHW, like the TF graph's
    [B, N, 1, C] images transposed); returns (logits, T1, T2) as numpy."""
    import torch
    import torch.nn.functional as F
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))

    def conv(img, scope):                                 # img [B, Cin, N, kw]; TF W [1, kw, Cin, Cout] -> [Cout, Cin, 1, kw]
        W = T(w[scope + "/weights"])
        return F.conv2d(img, W.permute(3, 2, 0, 1), T(w[scope + "/biases"]))

    def bn(x, scope):
        return F.relu(F.batch_norm(x, T(w[EMA % (scope, scope, "Squeeze")]), T(w[EMA % (scope, scope, "Squeeze_1")]),
                                   T(w[scope + "/bn/gamma"]), T(w[scope + "/bn/beta"]), training=False, eps=EPS))

    def fc(x, scope):
        return F.linear(x, T(w[scope + "/weights"]).T, T(w[scope + "/biases"]))

    def tnet(img, p, last, K):
        for s in ("tconv1", "tconv2", "tconv3"):
            img = bn(conv(img, p + "/" + s), p + "/" + s)
        h = F.max_pool2d(img, (img.shape[2], 1)).flatten(1)
        for s in ("tfc1", "tfc2"):
            h = bn(fc(h, p + "/" + s), p + "/" + s)
        return (fc(h, p + "/" + last) + torch.eye(K, dtype=torch.float64).flatten()).view(-1, K, K)

    x = T(pc)                                             # [B, N, 3]
    t1 = tnet(x.unsqueeze(1), "transform_net1", "transform_XYZ", 3)          # image [B, 1, N, 3]
    net = bn(conv(torch.bmm(x, t1).unsqueeze(1), "conv1"), "conv1")          # [B, 64, N, 1]
    net = bn(conv(net, "conv2"), "conv2")
    t2 = tnet(net, "transform_net2", "transform_feat", 64)
    feat = torch.bmm(net.squeeze(3).transpose(1, 2), t2)                      # [B, N, 64]
    net = feat.transpose(1, 2).unsqueeze(3)
    for s in ("conv3", "conv4", "conv5"):
        net = bn(conv(net, s), s)
    h = F.max_pool2d(net, (net.shape[2], 1)).flatten(1)
    for s in ("fc1", "fc2"):
        h = bn(fc(h, s), s)
    return fc(h, "fc3").numpy(), t1.numpy(), t2.numpy()
