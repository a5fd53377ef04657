"""An independent float64 model of the FoldingNet auto-encoder (transfer/foldingnet/foldingnet.py) for the tests: the graph
written out in numpy (brute-force kNN, np.cov, the symmetric adjacency as sorted rows), the network as torch functional ops
(conv1d, batch_norm in eval mode, linear) on the raw state dict in torch's own layouts, given the positions of both graph
pools.  The mistake switches give the variants the tests must tell apart.  Also: a numpy restatement of the device
sampler of csrc/foldingnet.hip."""
import numpy as np
import torch
import torch.nn.functional as F

GRID = 45
M64 = (1 << 64) - 1
GOLDEN_RATIO = 0x9e3779b97f4a7c15


def knn(pc):
    """(b, n, 16): the 17 nearest by float64 squared distance (stable order), column 0 dropped."""
    out = []
    for x in np.asarray(pc, np.float64):
        d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
        out.append(np.argsort(d, axis=1, kind="stable")[:, 1:17])
    return np.stack(out)


def graph_from_knn(pc, nb, ddof=1):
    """(cov (b, n, 9) rounded to float32, rows: per cloud the sorted symmetric adjacency rows) of neighbours nb (b, n, 16)."""
    pc = np.asarray(pc, np.float64)
    nb = np.asarray(nb, np.int64)
    covs, rows = [], []
    for x, L in zip(pc, nb):
        covs.append(np.stack([np.cov(x[r].T, ddof=ddof).reshape(-1) for r in L]).astype(np.float32))
        n = len(x)
        src = np.concatenate([np.repeat(np.arange(n), 16), L.reshape(-1)])
        dst = np.concatenate([L.reshape(-1), np.repeat(np.arange(n), 16)])
        key = np.unique(src * n + dst)
        r, c = key // n, key % n
        bounds = np.searchsorted(r, np.arange(n + 1))
        rows.append([c[bounds[i]:bounds[i + 1]] for i in range(n)])
    return np.stack(covs), rows


def degrees(rows):
    return np.array([[len(r) for r in rc] for rc in rows])


def resolve(rows, picks):
    picks = np.asarray(picks, np.int64)
    out = np.zeros(picks.shape, np.int64)
    for c, rc in enumerate(rows):
        for i, r in enumerate(rc):
            out[:, c, i] = r[picks[:, c, i]]
    return out


def model(state, pc, cov, cols, no_self=False, swap_grid=False, fold2_grid=False):
    """pc (b, n, 3), cov (b, n, 9), neighbour columns cols (2, b, n, 16) -> (code (b, 512), p1, recon (b, 2025, 3)) float64."""
    s = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in state.items()
         if not k.endswith("num_batches_tracked")}
    s = {(k[7:] if k.startswith("module.") else k): v for k, v in s.items()}
    bn = lambda x, i: F.batch_norm(x, s["encoder.bn%d.running_mean" % i], s["encoder.bn%d.running_var" % i],
                                   s["encoder.bn%d.weight" % i], s["encoder.bn%d.bias" % i], training=False, eps=1e-5)
    conv = lambda x, k: F.conv1d(x, s[k + ".weight"], s[k + ".bias"])

    def pool(x, c):                       # x (b, ch, n); c (b, n, 16)
        c = torch.as_tensor(np.asarray(c), dtype=torch.int64)
        g = torch.stack([x[k][:, c[k]] for k in range(len(x))])              # (b, ch, n, 16)
        m = g.max(dim=3)[0]
        return m if no_self else torch.max(m, x)

    with torch.no_grad():
        x = torch.as_tensor(np.concatenate([np.asarray(pc, np.float64), np.asarray(cov, np.float64)], 2)).transpose(1, 2)
        for i in (1, 2, 3):
            x = F.relu(bn(conv(x, "encoder.conv%d" % i), i))
        x = F.relu(pool(x, cols[0]))
        x = F.relu(bn(conv(x, "encoder.conv4"), 4))
        x = F.relu(pool(x, cols[1]))
        x = bn(conv(x, "encoder.conv5"), 5).max(dim=2)[0]
        x = F.relu(bn(F.linear(x, s["encoder.fc1.weight"], s["encoder.fc1.bias"]), 6))
        code = F.linear(x, s["encoder.fc2.weight"], s["encoder.fc2.bias"])
        b = code.shape[0]
        lin = np.linspace(-0.3, 0.3, GRID)
        gx, gy = np.meshgrid(lin, lin)
        g = np.stack([gx.reshape(-1), gy.reshape(-1)]).astype(np.float32)                # (2, 2025) as the reference
        if swap_grid:
            g = g[::-1]
        g = torch.as_tensor(g.copy(), dtype=torch.float64).unsqueeze(0).expand(b, 2, GRID * GRID)
        rep = code.unsqueeze(2).expand(b, 512, GRID * GRID)
        a = F.relu(conv(torch.cat([rep, g], 1), "decoder.fold1.conv1"))
        a = F.relu(conv(a, "decoder.fold1.conv2"))
        p1 = conv(a, "decoder.fold1.conv3")
        feed = torch.cat([g, torch.zeros_like(g[:, :1])], 1) if fold2_grid else p1
        a = F.relu(conv(torch.cat([rep, feed], 1), "decoder.fold2.conv1"))
        a = F.relu(conv(a, "decoder.fold2.conv2"))
        out = conv(a, "decoder.fold2.conv3")
    return code.numpy(), p1.transpose(1, 2).numpy(), out.transpose(1, 2).numpy()


# ------------------------------------------------------------------------------------------------ the device sampler
def _mix(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return z ^ (z >> np.uint64(31))


def device_picks(seed, ordinals, degree):
    """Positions (2, b, n, 16) the device sampler draws for clouds of the given ordinals (b,) and degrees (b, n)."""
    degree = np.asarray(degree, np.int64)
    b, n = degree.shape
    G = np.uint64(GOLDEN_RATIO)
    with np.errstate(over="ignore"):
        k0 = _mix(np.uint64(int(seed) & M64) + G)
        out = np.zeros((2, b, n, 16), np.int64)
        for layer in (0, 1):
            key = _mix(_mix(k0 ^ np.asarray(ordinals, np.uint64))[:, None]
                       ^ ((np.uint64(layer) << np.uint64(32)) | np.arange(n, dtype=np.uint64))[None, :])
            picked = np.zeros((b, n, 16), np.int64)
            for t in range(16):
                j = degree - 16 + t
                r = _mix(key + np.uint64(t + 1) * G)
                x = (((r >> np.uint64(32)) * (j + 1).astype(np.uint64)) >> np.uint64(32)).astype(np.int64)
                seen = (picked[:, :, :t] == x[:, :, None]).any(axis=2)
                picked[:, :, t] = np.where(seen, j, x)
            out[layer] = picked
    return out
