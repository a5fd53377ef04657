"""Writes tests/golden/foldingnet_train.npz from the REFERENCE's own FoldingNet modules in TRAIN mode (TEST INFRASTRUCTURE;
needs a checkout of the reference project with scipy and scikit-learn -- never run on the GPU machines, where the tests
only read the .npz):

    python tools/make_golden_foldingnet_train.py --reference <checkout of the reference project>

One forward of train_foldingnet.py:88-100 on the CPU in float64: build_graph (prepare_graph.py: knn_search, edges2A),
FoldingNet_graph().double().train() and ChamferLoss against the reconstruction and against fold1's output.  The modules are
imported by path, as make_golden_foldingnet.py does.  torch.set_default_dtype(torch.float64) comes first: Graph_Pooling
allocates torch.zeros(x.size()) in the default dtype and would otherwise round the pooled neighbours to float32.  The
backward is not run: Graph_Pooling cannot be differentiated at batch > 1.

Contents: the seed and sha256 of the repository's synthetic weights (fold_weights.synthetic_state), 3 clouds of 512 points,
every point's degree and every np.random.choice position drawn (uint8, [pool layer, cloud, point, 16]; np.random.seed
(GRAPH_SEED) once before the forward), the covariance build_graph returned, loss, mid loss, the code, the first
RECON_POINTS points of each reconstruction and of fold1's output, and every batch norm's running mean / variance and
num_batches_tracked after the forward.
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from geometric_adv_amd import fold_weights as FW  # noqa: E402
from make_golden_foldingnet import _load, neighbour_gap, weights_sha256  # noqa: E402

GRAPH_SEED = 77
WEIGHT_SEED = 11
B, N = 3, 512
RECON_POINTS = 256
MIN_GAP = 1e-7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "foldingnet_train.npz"))
    a = ap.parse_args()
    fdir = os.path.join(a.reference, "transfer", "foldingnet")
    PG = _load("ref_prepare_graph", os.path.join(fdir, "prepare_graph.py"))
    FN = _load("ref_foldingnet", os.path.join(fdir, "foldingnet.py"))
    torch.set_default_dtype(torch.float64)

    state = FW.synthetic_state(WEIGHT_SEED)
    model = FN.FoldingNet_graph().double()
    sd = {k: (torch.tensor(0, dtype=torch.int64) if k.endswith("num_batches_tracked")
              else torch.from_numpy(np.asarray(state[k], np.float64))) for k in model.state_dict().keys()}
    model.load_state_dict(sd)
    model.train()

    xs, seeds, s = [], [], 300
    while len(xs) < B:
        x = (np.random.default_rng(s).random((N, 3)) - 0.5).astype(np.float32)
        if neighbour_gap(x) > MIN_GAP:
            xs.append(x)
            seeds.append(s)
        s += 1
    x = np.stack(xs)

    draws = []
    choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        r = choice(a, size, replace, p)
        draws.append((int(a), np.array(r)))
        return r

    points = torch.tensor(x)
    opts = PG.GraphOptions()
    opts.num_points = N
    batch_graph, Cov = PG.build_graph(points, opts)
    np.random.choice = recording_choice
    np.random.seed(GRAPH_SEED)
    with torch.no_grad():
        pts = points.transpose(2, 1).double()
        recon, mid, code = model(pts, Cov.transpose(2, 1).double(), batch_graph)
        loss = FN.ChamferLoss()(pts.transpose(2, 1), recon.transpose(2, 1))
        mid_loss = FN.ChamferLoss()(pts.transpose(2, 1), mid.transpose(2, 1))
    np.random.choice = choice
    assert len(draws) == 2 * B * N, len(draws)
    degree = np.zeros((B, N), np.int64)
    positions = np.zeros((2, B, N, 16), np.int64)
    for blk in range(2 * B):                    # pool 1 of every cloud, then pool 2
        layer, c = divmod(blk, B)
        for i in range(N):
            deg, r = draws[blk * N + i]
            degree[c, i] = deg
            positions[layer, c, i] = r
    assert degree.max() < 256 and degree.min() >= 16
    out = dict(graph_seed=GRAPH_SEED, weight_seed=WEIGHT_SEED, sha256=weights_sha256(state), clouds=x, cloud_seeds=np.array(seeds),
               degree=degree.astype(np.uint8), positions=positions.astype(np.uint8), cov=Cov.numpy().astype(np.float64),
               loss=float(loss), mid_loss=float(mid_loss), code=code.numpy(),
               recon=recon.transpose(2, 1).numpy()[:, :RECON_POINTS], mid=mid.transpose(2, 1).numpy()[:, :RECON_POINTS])
    for k, v in model.state_dict().items():
        if "running" in k or k.endswith("num_batches_tracked"):
            out[k] = v.numpy()
    np.savez_compressed(a.out, **out)
    print("wrote %s (%d bytes): loss %.6f mid %.6f degrees %d..%d" % (a.out, os.path.getsize(a.out), float(loss), float(mid_loss),
                                                                      degree.min(), degree.max()))


if __name__ == "__main__":
    main()
