"""Writes tests/golden/foldingnet.npz from the REFERENCE's own FoldingNet modules (TEST INFRASTRUCTURE; needs a checkout of
the reference project with scipy and scikit-learn, run on a host that has one -- never on the GPU machines, where the tests
only read the .npz):

    python tools/make_golden_foldingnet.py --reference <checkout of the reference project>

  - transfer/foldingnet/foldingnet.py (FoldingNet_graph, Graph_Pooling, GridSamplingLayer) and prepare_graph.py
    (build_graph: KDTree, np.cov, the symmetric CSR adjacency, a multiprocessing.Pool) are imported by path, as they are;
    prepare_graph is registered in sys.modules so that the pool can pickle build_graph_core,
  - FoldingNetAutoEncoder.get_reconstructions' loop (foldingnet_ae.py:40-66: a DataLoader of 4 clouds per chunk,
    build_graph, the model) is repeated on the CPU, since the reference's method calls .cuda(), with the model in float64
    (torch.set_default_dtype: Graph_Pooling allocates with the default dtype),
  - np.random.seed(SEED) once, then two successive calls -- 5 clouds (crossing a chunk boundary), then 1 cloud -- exactly
    as a reference run would make them; np.random.choice is wrapped to record every draw.

Contents: the graph seed, the seed and sha256 of the repository's synthetic weights (fold_weights.synthetic_state), the
reference model's state-dict keys, 6 clouds of 2048 points (their seeds chosen so that the float64 gap between the 16th
and 17th neighbour's squared distance is far above fp32 rounding), every point's degree, every position drawn (uint8,
[pool layer, cloud, point, 16]), the covariance of the first COV_POINTS points of each cloud, the code, p1 and
reconstruction in float64, and the decoder's grid.
"""
import argparse
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometric_adv_amd import fold_weights as FW  # noqa: E402

GRAPH_SEED = 2024
WEIGHT_SEED = 11
N = 2048
CALLS = (5, 1)
COV_POINTS = 256
MIN_GAP = 1e-7          # squared distance; fp32 rounding of a squared distance of ~0.02 is ~1e-9


def weights_sha256(state):
    h = hashlib.sha256()
    for k in FW.key_names():
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(state[k], np.float32).tobytes())
    return h.hexdigest()


def neighbour_gap(x):
    """min over points of d_(17) - d_(16) (float64 squared distances, self at d_(0) = 0): the margin of the 16-set."""
    x = x.astype(np.float64)
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    d.sort(axis=1)
    assert (d[:, 1] > 0).all()
    return float((d[:, 17] - d[:, 16]).min())


def clouds(count):
    out, seeds, s = [], [], 100
    while len(out) < count:
        x = (np.random.default_rng(s).random((N, 3)) - 0.5).astype(np.float32)
        if neighbour_gap(x) > MIN_GAP:
            out.append(x)
            seeds.append(s)
        s += 1
    return np.stack(out), np.array(seeds)


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "foldingnet.npz"))
    a = ap.parse_args()
    fdir = os.path.join(a.reference, "transfer", "foldingnet")
    PG = _load("ref_prepare_graph", os.path.join(fdir, "prepare_graph.py"))
    FN = _load("ref_foldingnet", os.path.join(fdir, "foldingnet.py"))
    torch.set_default_dtype(torch.float64)

    state = FW.synthetic_state(WEIGHT_SEED)
    model = FN.FoldingNet_graph()
    keys = list(model.state_dict().keys())
    sd = {k: (torch.tensor(0, dtype=torch.int64) if k.endswith("num_batches_tracked")
              else torch.from_numpy(np.asarray(state[k], np.float64))) for k in keys}
    model.load_state_dict(sd)
    model.eval()

    x, cloud_seeds = clouds(sum(CALLS))
    draws = []
    choice = np.random.choice

    def recording_choice(a, size=None, replace=True, p=None):
        r = choice(a, size, replace, p)
        draws.append((int(a), np.array(r)))
        return r

    np.random.choice = recording_choice
    np.random.seed(GRAPH_SEED)
    codes, p1s, recons, order = [], [], [], []           # order: (pool layer, cloud) of each block of N draws
    start = 0
    with torch.no_grad():
        for count in CALLS:
            pc_input = x[start:start + count]
            dl = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.tensor(pc_input)), batch_size=4,
                                             num_workers=0, drop_last=False)
            c0 = start
            for data in dl:
                batch = data[0]
                batch_graph, Cov = PG.build_graph(batch)
                recon, p1, code = model(batch.transpose(2, 1).double(), Cov.transpose(2, 1), batch_graph)
                codes.append(code.numpy()); p1s.append(p1.transpose(2, 1).numpy()); recons.append(recon.transpose(2, 1).numpy())
                order += [(layer, c0 + k) for layer in (0, 1) for k in range(len(batch))]
                c0 += len(batch)
            start += count
    np.random.choice = choice
    b = len(x)
    assert len(draws) == 2 * b * N, len(draws)
    degree = np.zeros((b, N), np.int64)
    positions = np.zeros((2, b, N, 16), np.int64)
    for blk, (layer, c) in enumerate(order):
        for i in range(N):
            deg, r = draws[blk * N + i]
            if layer == 0:
                degree[c, i] = deg
            assert degree[c, i] == deg
            positions[layer, c, i] = r
    assert degree.max() < 256 and degree.min() >= 16
    # the covariance as build_graph computes it (knn_search), for the first points
    cov = np.stack([PG.knn_search(x[c].astype(np.float64))[2][:COV_POINTS] for c in range(b)])
    grid = FN.GridSamplingLayer(1, [[-0.3, 0.3, 45], [-0.3, 0.3, 45]])[0]
    np.savez_compressed(a.out, graph_seed=GRAPH_SEED, weight_seed=WEIGHT_SEED, sha256=weights_sha256(state),
                        keys=np.array(keys), clouds=x, cloud_seeds=cloud_seeds, calls=np.array(CALLS),
                        degree=degree.astype(np.uint8), positions=positions.astype(np.uint8), cov=cov.astype(np.float32),
                        code=np.concatenate(codes), p1=np.concatenate(p1s), recon=np.concatenate(recons),
                        grid=grid.astype(np.float32))
    print("wrote %s (%d bytes): cloud seeds %s, degrees %d..%d" % (a.out, os.path.getsize(a.out), cloud_seeds.tolist(),
                                                                   degree.min(), degree.max()))


if __name__ == "__main__":
    main()
