"""GPU: geoadv_attack_run with the kNN term under the surface rule (geoadv_attack_config.knn_rule = 1) and
geoadv_knn_outlier_loss with GEOADV_KNN_LOSS_SURFACE are held to the stream they are given and do not block the host -- the
delayed-call protocol of tests/_stream_order.py, as tests/test_gpu_stream_order_attack_knn.py applies it to the SOR rule's term
and tests/test_gpu_stream_order.py to the op without the flag.  The surface rule is a second pair of instances of the one
gradient launch (csrc/knn_loss.hip): a launch of it that went to the null stream would run at once, on the other input.

This file sorts AFTER tests/test_gpu_stream_order.py on purpose, for the reason tests/test_gpu_stream_order_attack_knn.py states:
that module's first control test must be the first in the session to take a side stream from torch's pool.  The Delay is this
module's own, calibrated when it runs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, DEV = 16, 256, "cuda:0"
W_TERM, K, THRESH = 3.0, 2, 0.04         # random clouds in the unit cube, 256 points: the mean distance to two neighbours is about 0.09


_DELAY = []


def _delay():
    """This module's Delay, calibrated once."""
    if not _DELAY:
        _DELAY.append(SO.Delay())
    return _DELAY[0]


def _clouds(seed, b=B):
    return (np.random.default_rng(seed).random((b, N, 3)) - 0.5).astype(np.float32)


def _feed(a, b):
    import torch
    ta, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (a, b))
    return (ta.clone(), ta, tb)


def test_run_with_the_surface_term_is_held_to_its_stream():
    """Stateful: every step of the protocol gets a twin handle (a zero-filled arena) on one victim.  At thresh = 0.04 nearly every
    point of these clouds is masked, so the term's launch has work that depends on the input."""
    import torch
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    from geometric_adv_amd.autoencoder import PointNetAE
    ae = PointNetAE(W.randomized_weights(N), N, encoder_arith="bf16x3")

    def build():
        conf = Configuration(batch_size=B, n_points=N, weights=None, num_iterations=2, num_iterations_thresh=1,
                             knn_weight=W_TERM, knn_k=K, knn_rule="surface", knn_thresh=THRESH)
        at = AdvAE("stream-order-surface", conf, ae=ae)
        rng = np.random.default_rng(970)
        feeds = [_feed(_clouds(971), _clouds(972)), _feed(_clouds(973), _clouds(974)),
                 _feed(np.abs(rng.standard_normal((B, 128))).astype(np.float32), np.abs(rng.standard_normal((B, 128))).astype(np.float32)),
                 _feed((0.5 + rng.random(B)).astype(np.float32), (0.25 + rng.random(B)).astype(np.float32)),
                 _feed((0.01 * rng.standard_normal((B, N, 3))).astype(np.float32), (0.01 * rng.standard_normal((B, N, 3))).astype(np.float32))]
        hist = torch.zeros((2, 6, B), dtype=torch.float32, device=DEV)

        def call():
            x, gt, tz, w, init = (f[0] for f in feeds)
            at.set_inputs(x, gt, tz, w)
            at.init_pert(init, reset_optimizer=True)
            at.run(0, 2, 1, hist)
            peek = at.peek()
            return [hist] + [peek[k] for k in sorted(peek)]
        return SO.Rig(feeds, call, keep=at)

    SO.check("attack_run_surface_term", build, _delay(), stateful=True)


def test_the_op_under_the_flag_is_held_to_its_stream():
    """geoadv_knn_outlier_loss with GEOADV_KNN_LOSS_SURFACE on buffers the case owns: the search's launches and the surface
    instance of the loss launch."""
    import torch
    from geometric_adv_amd import _abi, _lib
    b, k = 3, 7
    pc = _feed(_clouds(975, b), _clouds(976, b))
    z = lambda dtype, *shape: torch.zeros(shape, dtype=dtype, device=DEV)      # noqa: E731
    loss, grad, score = z(torch.float64, b), z(torch.float32, b, N, 3), z(torch.float64, b, N)
    mask, idx, stats = z(torch.uint8, b * N), z(torch.int32, b, N, k), z(torch.float64, b, 4)
    wb = int(_lib.lib().geoadv_knn_outlier_loss_workspace_bytes(b, N, k))
    ws = z(torch.uint8, wb)

    def call():
        with torch.cuda.device(DEV):
            _lib.check(_lib.lib().geoadv_knn_outlier_loss(_abi.GEOADV_KNN_LOSS_SURFACE, b, N, k, 0.1, _lib.ptr(pc[0]), _lib.ptr(loss),
                                                          _lib.ptr(grad), _lib.ptr(score), _lib.ptr(mask), _lib.ptr(idx), _lib.ptr(stats),
                                                          _lib.ptr(ws), wb, _lib.stream_handle()), "knn_outlier_loss | surface")
        return loss, grad, score, mask, idx, stats
    SO.check("knn_outlier_loss_surface", lambda: SO.Rig([pc], call, keep=ws), _delay())
