"""GPU: the two stream-taking entry points of the neighbour lists (csrc/chamfer_lists.hip) in the delayed-call protocol of
tests/_stream_order.py: geoadv_nn_distance_lists (a clear, the build, the query and the read-out kernel: must only enqueue) and
geoadv_attack_list_state (synchronises, as its declaration says: held to the ordering alone) behind an attack run with the lists
pinned on.  The cases are registered in the table of tests/test_gpu_stream_order.py at import, which its coverage test
(every stream-taking entry point of the header has a case) reads when the suite runs; they are run here.

This file sorts AFTER tests/test_gpu_stream_order.py on purpose, as tests/test_gpu_stream_order_attack_knn.py explains; the delay
is the session's (the 50 ms floor when this file runs alone)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _recon_lists_model as M  # noqa: E402
import _stream_order as SO  # noqa: E402
import test_gpu_stream_order as TSO  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, DEV = 3, 1000, "cuda:0"
SYNC_LIST_STATE = "(host memory; synchronises the stream)"


def _dev(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v)).to(DEV)


@TSO.case("nn_distance_lists", ["geoadv_nn_distance_lists"])
def _nn_distance_lists():
    import torch
    from geometric_adv_amd import ops
    sets = []                     # two well-formed inputs: (anchor, columns, the anchor's exact minima, skin, moved rows)
    for seed in (980, 990):
        a, c = M.uniform(seed, B, N), M.uniform(seed + 1, B, N)
        d1, _, d2, _ = ops.nn_distance(_dev(a), _dev(c))
        sets.append([_dev(a), _dev(c), d1, d2, _dev(np.full(B, 8e-3 if seed == 980 else 1.2e-2, np.float32)),
                     _dev(M.moved_by(a, seed + 2, 2e-3))])
    torch.cuda.synchronize()
    feeds = [(x.clone(), x, y) for x, y in zip(*sets)]
    return SO.Rig(feeds, lambda: list(ops.nn_distance_lists(*[f[0] for f in feeds])))


@TSO.case("attack_list_state", ["geoadv_attack_list_state"], stateful=True, blocks=SYNC_LIST_STATE)
def _attack_list_state():
    import torch
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    from geometric_adv_amd.autoencoder import PointNetAE
    b, n = 8, 256
    if "ae" not in _KEEP:
        _KEEP["ae"] = PointNetAE(W.randomized_weights(n), n, encoder_arith="bf16x3")
    at = AdvAE("stream-order-lists", Configuration(batch_size=b, n_points=n, weights=None, num_iterations=20, num_iterations_thresh=1,
                                                   chamfer_kernel="symmetric", chamfer_prune="always", recon_lists="pinned"), ae=_KEEP["ae"])
    rng = np.random.default_rng(970)
    feeds = [(x.clone(), x, y) for x, y in
             ((_dev(M.uniform(971, b, n)), _dev(M.uniform(972, b, n))), (_dev(M.uniform(973, b, n)), _dev(M.uniform(974, b, n))),
              (_dev((0.5 + rng.random(b)).astype(np.float32)), _dev((0.25 + rng.random(b)).astype(np.float32))))]
    hist = torch.zeros((20, 6, b), dtype=torch.float32, device=DEV)

    def call():
        x, gt, w = (f[0] for f in feeds)
        at.set_inputs(x, gt, None, w)
        at.init_pert(None, reset_optimizer=True)
        at.run(0, 20, 1, hist)                       # an anchor, 15 list iterations, an anchor, 4 list iterations
        st = at.list_state()
        peek = at.peek()
        return [hist] + [st[k] for k in sorted(st)] + [peek[k] for k in sorted(peek)]
    return SO.Rig(feeds, call, keep=at)


_KEEP = {}


@pytest.mark.parametrize("name", ["nn_distance_lists", "attack_list_state"])
def test_the_list_entry_points_are_held_to_their_stream(name):
    build, _, stateful, blocks = TSO.CASES[name]
    SO.check(name, build, SO.session_delay(), stateful=stateful, blocks=blocks)
