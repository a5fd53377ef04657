"""GPU: geoadv_attack_run with the kNN outlier term (geoadv_attack_config.knn_weight) is held to the stream it is given and does
not block the host -- the delayed-call protocol of tests/_stream_order.py, as tests/test_gpu_stream_order.py applies it to the
attack handle without the term.  The search's launches and the term's launch (csrc/knn_loss.hip, called from do_step) must wait
behind the delay on the side stream like the rest of the iteration; a launch that went to the null stream instead would run at
once, on clouds derived from the other input.

This file sorts AFTER tests/test_gpu_stream_order.py on purpose: that module's first control test holds the first side stream a
process takes from torch's pool against the null stream, and a test that takes a side stream earlier in the session hands it the
second one instead (seen on the MI355X: the control then finds the null stream waiting behind the side stream's delay).  The
Delay is this test's own, calibrated when it runs; the session's belongs to that module."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stream_order as SO  # noqa: E402

pytestmark = pytest.mark.gpu

B, N, DEV = 16, 256, "cuda:0"
W_TERM, K, ALPHA = 3.0, 5, 1.05


def test_run_with_the_knn_term_is_held_to_its_stream():
    """Stateful: every step of the protocol gets a twin handle (a zero-filled arena) on one victim.  Random clouds: at alpha = 1.05
    about a tenth of the points are masked, so the term's launch has work that depends on the input."""
    import torch
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    from geometric_adv_amd.autoencoder import PointNetAE
    ae = PointNetAE(W.randomized_weights(N), N, encoder_arith="bf16x3")

    def feed(a, b):
        ta, tb = (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for v in (a, b))
        return (ta.clone(), ta, tb)

    def clouds(seed):
        return (np.random.default_rng(seed).random((B, N, 3)) - 0.5).astype(np.float32)

    def build():
        conf = Configuration(batch_size=B, n_points=N, weights=None, num_iterations=2, num_iterations_thresh=1,
                             knn_weight=W_TERM, knn_k=K, knn_alpha=ALPHA)
        at = AdvAE("stream-order-knn", conf, ae=ae)
        rng = np.random.default_rng(960)
        feeds = [feed(clouds(961), clouds(962)), feed(clouds(963), clouds(964)),
                 feed(np.abs(rng.standard_normal((B, 128))).astype(np.float32), np.abs(rng.standard_normal((B, 128))).astype(np.float32)),
                 feed((0.5 + rng.random(B)).astype(np.float32), (0.25 + rng.random(B)).astype(np.float32)),
                 feed((0.01 * rng.standard_normal((B, N, 3))).astype(np.float32), (0.01 * rng.standard_normal((B, N, 3))).astype(np.float32))]
        hist = torch.zeros((2, 6, B), dtype=torch.float32, device=DEV)

        def call():
            x, gt, tz, w, init = (f[0] for f in feeds)
            at.set_inputs(x, gt, tz, w)
            at.init_pert(init, reset_optimizer=True)
            at.run(0, 2, 1, hist)
            peek = at.peek()
            return [hist] + [peek[k] for k in sorted(peek)]
        return SO.Rig(feeds, call, keep=at)

    SO.check("attack_run_knn_term", build, SO.Delay(), stateful=True)
