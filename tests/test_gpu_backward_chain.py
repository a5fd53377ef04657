"""GPU: the loop's loss / Chamfer-gradient launch in its short form -- row minima of the symmetric scan as packed (distance, index)
words from 8 column slices on, read directly by the loss row, and the one-pass gradient body with two load round trips
(csrc/loss_cgrad.h) -- against the forms it replaced, which stay reachable through geoadv_attack_test_loss_form: one partial per
slice at 8 slices, the general multi-pass gradient body, packed words folded through LDS.  Everything must agree bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_MODELS = {}


def _model(n, arith=None):
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    if (n, arith) not in _MODELS:
        w = W.synthetic_weights(n, seed=7)
        _MODELS[(n, arith)] = (w, PointNetAE(w, n, encoder_arith=arith))
    return _MODELS[(n, arith)]


def _inputs(b, n, inf_row):
    """Clouds with duplicated target / source columns in the first and the last column slice (the lowest index must win), cloud 0
    perturbed far enough that the paired search hands it back, and optionally one point of cloud 1 so far out that every one of its
    squared distances overflows: a row whose minimum is +inf."""
    from conftest import cloud
    x, gt = cloud(601, b, n), cloud(602, b, n)
    for a in (x, gt):
        a[:, n // 2] = a[:, 3]
        a[:, n - 1] = a[:, 3]
    rng = np.random.default_rng(603)
    p0 = (1e-3 * rng.standard_normal((b, n, 3))).astype(np.float32)
    p0[0] = (0.3 * (rng.random((n, 3)) - 0.5)).astype(np.float32)
    if inf_row:
        p0[1 % b, 7, 0] = 1.9e19                  # (1.9e19)^2 > FLT_MAX; differences of finite numbers: no NaN
    return x, gt, p0


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _run(b, n, prune, form, iters, inf_row=False, loss_in_scan=True):
    import torch
    from geometric_adv_amd.adv_ae import AdvAE, Configuration
    w, ae = _model(n, "f32" if inf_row else None)
    x, gt, p0 = _inputs(b, n, inf_row)
    at = AdvAE("a", Configuration(batch_size=b, n_points=n, weights=w, num_iterations=iters + 1, num_iterations_thresh=1, learning_rate=1e-4,
                                  chamfer_prune=prune, chamfer_kernel="symmetric", loss_in_scan=loss_in_scan), ae=ae)
    at._test_loss_form(form)
    at.set_inputs(x, gt, None, 1.0)
    at.init_pert(p0, reset_optimizer=True)
    out = {}
    if iters:
        hist = torch.empty((iters, 6, b), device=ae.device)
        at.run(0, iters, 1, hist)
        out["hist"] = hist
    out.update(at.peek())
    out.update(at._test_loss_state())
    torch.cuda.synchronize()
    searched, handed_back = at.search_state()
    out = {k: v.clone() for k, v in out.items()}
    del at
    return out, searched, handed_back


def _assert_same(got, want, what):
    import torch
    assert got.keys() == want.keys()
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("prune", ["always", False])
@pytest.mark.parametrize("b,n", [(1, 256), (8, 256), (33, 256), (1, 2048), (8, 2048), (33, 2048)])
def test_loss_launch_equals_the_forms_it_replaced(b, n, prune):
    """g_recon, g_dist, idx1 of both problems, the row minima and every loss row after three iterations (the search's verdicts
    reach the scan one call late), in the pruned and in the all-pairs loop: the default against form 3 (the parent's: partials
    per slice at 8 slices -- B = 33 at 2048 points --, general gradient body, words folded through LDS) and against each bit alone."""
    new, searched, handed_back = _run(b, n, prune, 0, 3)
    assert searched == (prune == "always")
    if searched:
        assert handed_back >= 1, "cloud 0 was scattered: the search must hand it back"
        assert b == 1 or handed_back < b, "the other clouds barely moved: the search must keep them"
    assert new["g_recon"].abs().max() > 0 and new["g_dist"].abs().max() > 0
    # duplicated columns: the copies at n / 2 and n - 1 never win against the original at 3
    for k in ("idx_r1", "idx_a1"):
        assert not ((new[k] == n // 2) | (new[k] == n - 1)).any(), k
    if b > 1:
        assert (new["idx_a1"][1:, n - 1] == 3).all() and (new["idx_a1"][1:, n // 2] == 3).all()
    for form in (3, 1, 2):
        old, _, hb = _run(b, n, prune, form, 3)
        assert hb == handed_back
        _assert_same(new, old, "form %d" % form)


@pytest.mark.parametrize("form", [3, 1])
def test_a_row_whose_minimum_is_inf(form):
    """B = 33 at 2048 points is exactly 8 column slices: packed words by default, partials per slice in the parent's form.  One
    adversarial point lies so far out that all its squared distances are +inf (all-pairs loop: the scan answers nn_distance(adv, x));
    the first forward must give the same bits either way, the +inf row included, and index 0 for it."""
    import torch
    b, n = 33, 2048
    new, _, _ = _run(b, n, False, 0, 0, inf_row=True)
    assert torch.isinf(new["dist_a1"][1, 7]) and new["dist_a1"][1, 7] > 0
    assert new["idx_a1"][1, 7] == 0
    old, _, _ = _run(b, n, False, form, 0, inf_row=True)
    _assert_same(new, old, "form %d" % form)


@pytest.mark.parametrize("b", [8, 32])
def test_riding_loss_workgroups_equal_the_forms_they_replaced(b):
    """The same bodies as the last riders of the scan's launch (loss_in_scan='always'): 16 and 8 column slices."""
    new, _, _ = _run(b, 2048, "always", 0, 3, loss_in_scan="always")
    for form in (3, 0):
        old, _, _ = _run(b, 2048, "always", form, 3, loss_in_scan=False)
        _assert_same(new, old, "own launch, form %d" % form)
