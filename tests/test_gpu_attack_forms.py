"""GPU: the attack iteration against the float64 model (oracle/attack_model.py) and the pinned C oracle in EVERY form do_forward /
do_step choose among -- by batch, cloud size and loss configuration -- with the method of
test_gpu_attack.py::test_single_iterations_match_model: two consecutive iterations, each checked from the GPU's own state
(adv / latent / recon, all four index arrays exactly, the gradient with the matches pinned to the GPU's, Adam from the GPU's own
gradient, the six history rows of the updated state).  Every case first asserts, through AdvAE._test_plan() (what the library
recorded of its last forward: geoadv_attack_test_plan), that it runs the form it was written for.

Shapes (smallest that take the form; read-out of an MI355X run):

  case    shape                                    scan             rows leave as (cc)         loss row / gradient (cc)
  A       16 x 256, all-pairs, auto kernel         plain, 1 x 8     packed words               own fused launch, 1-pass body, 256 live points
  A-ride  as A, loss_in_scan="always"              plain, 1 x 8     packed words               riders of the scan's launch, 1-pass body
  B       33 x 2048, search on, cloud 0 scattered  plain, 1 x 8     packed words               own fused launch, 1-pass body, 4 points / thread
  C       32 x 1025, all-pairs                     plain, 1 x 5     5 partials (loss_premerge) own fused launch, 1-pass body, last point alone
  C-ride  as C, loss_in_scan="always"              plain, 1 x 5     5 partials                 riders
  D       64 x 2048, all-pairs                     screened, 1 x 2  2 partials                 own fused launch, 1-pass body
  E       3 x 2049, search on                      plain, 2 x 33    merge launch               fused, general body, H = 1
  F       2 x 5000 / 2 x 5001, all-pairs           plain, 3 x 40    merge launch               fused, general body, H = 1 / H = 2
  G       1 x 10001 / 1 x 15000                    plain, 5 x 40 / 8 x 59   merge launch       fused, general body, H = 3
  H       1 x 15001 / 1 x 16385                    plain 8 x 59 / screened 9 x 65, merge launch   loss_metrics_kernel, sorted gradient kernel in the step

(rows x slices = row super-tiles x row partials per row.)  Every loss configuration but chamfer / chamfer takes the merge launch
wherever the scan has more than one slice; the max-point-distance variants (ccm, lcm) and latent / pert take loss_metrics_kernel,
and ccm / lcm form the Chamfer gradient in the step (the bodies' `j == jstar` branch).  32768 points -- the handle's limit -- are
left out: the CPU reference alone takes tens of seconds there.

Tolerances: those of test_gpu_attack.py (adv 1e-7, latent / recon 2e-6 absolute, indices exact, gradient 1e-4 of each cloud's
largest component, loss rows 1e-5 relative -- the latent loss 3e-5 --, Adam rtol 2e-6 / atol 2e-8).  They were established up to
8192 points; above that the project's float32 numpy model (AEModel(..., np.float32) under AttackModel) was run against float64 on
the same inputs (F32_MODEL below): where IT misses a bound, the bound of that case is 4 x its error (the margin the training tests
keep over a measured worst case); nowhere is a bound derived from the kernels' output.  MEASURED holds the worst errors of one
GPU run (pytest -s prints them per case).  tests/test_attack_forms_f32_model.py (CPU) regenerates F32_MODEL's comparison and
asserts that the float32 model meets TOL on those inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR = 1e-3          # Adam's first steps move every coordinate by ~LR: small against the steering entry below, so that the max-point
                   # terms stay on the steered point in the second iteration as well
STEER = 0.05       # one large perturbation entry per cloud: arg-max of dist(adv_j, x) and of |pert_j|^2 by a wide margin

VARIANTS = {       # name: loss_adv, loss_dist, extra weight
    "cc": ("chamfer", "chamfer", {}),
    "lc": ("latent", "chamfer", {}),
    "cp": ("chamfer", "pert", {}),
    "lp": ("latent", "pert", {"max_point_pert_weight": 0.5}),
    "ccm": ("chamfer", "chamfer", {"max_point_dist_weight": 2.0}),
    "lcm": ("latent", "chamfer", {"max_point_dist_weight": 0.5}),
}
ALL = tuple(VARIANTS)

TOL = dict(adv=1e-7, latent=2e-6, recon=2e-6, grad=1e-4, grad_rest=1e-4, rows=1e-5, latent_loss=3e-5, adam=1.0)
# (adam: in units of rtol 2e-6 |want| + atol 2e-8; grad_rest: the gradient without the point of the max-point term, see _Run.iteration)

# float32 numpy model against float64 on the inputs of the cases above 8192 points (first forward and gradient), as printed by
# tests/test_attack_forms_f32_model.py: worst error per quantity, in the units of TOL.  Every entry is within its bound, so no bound is widened.
F32_MODEL = {
    "G10001-cc": dict(adv=0.0, latent=1.8e-07, recon=1.44e-08, grad=2.49e-07, rows=3.62e-08),
    "G10001-lo-ccm": dict(adv=0.0, latent=1.8e-07, recon=1.44e-08, grad=4.43e-08, rows=7.66e-08),
    "G10001-hi-ccm": dict(adv=0.0, latent=1.8e-07, recon=1.44e-08, grad=3.11e-08, rows=5.30e-08),
    "G15000-cc": dict(adv=0.0, latent=1.8e-07, recon=1.75e-08, grad=5.28e-07, rows=2.98e-08),
    "H15001-cc": dict(adv=0.0, latent=1.8e-07, recon=1.45e-08, grad=4.51e-07, rows=5.01e-08),
    "H15001-ccm": dict(adv=0.0, latent=1.8e-07, recon=1.45e-08, grad=7.21e-09, rows=5.01e-08),
    "H15001-cp": dict(adv=0.0, latent=1.8e-07, recon=1.45e-08, grad=4.08e-08, rows=5.01e-08),
    "H15001-lc": dict(adv=0.0, latent=1.8e-07, recon=1.45e-08, grad=9.78e-06, latent_loss=7.81e-06, rows=5.01e-08),
    "H16385-cc": dict(adv=0.0, latent=1.8e-07, recon=1.28e-08, grad=4.99e-07, rows=5.91e-08),
}
# worst error per quantity and case of one MI355X run (both iterations), in the units of TOL
MEASURED = {
    "A-cc": dict(adv=0.0, latent=3.27e-07, recon=6.87e-08, grad=4.08e-07, rows=1.27e-07, adam=1.63e-02),
    "A-lc": dict(adv=0.0, latent=2.26e-07, recon=6.12e-08, grad=8.40e-06, rows=9.05e-08, latent_loss=2.19e-06, adam=1.67e-02),
    "A-cp": dict(adv=0.0, latent=2.07e-07, recon=6.56e-08, grad=8.55e-08, rows=1.31e-07, adam=1.11e-02),
    "A-lp": dict(adv=0.0, latent=1.96e-07, recon=6.12e-08, grad=1.26e-06, grad_rest=1.06e-05, rows=2.30e-07, latent_loss=1.12e-06, adam=1.11e-02),
    "A-ccm": dict(adv=0.0, latent=3.27e-07, recon=6.87e-08, grad=4.49e-08, grad_rest=4.08e-07, rows=9.21e-08, adam=1.63e-02),
    "A-lcm": dict(adv=0.0, latent=2.26e-07, recon=6.12e-08, grad=8.40e-06, grad_rest=8.40e-06, rows=1.05e-07, latent_loss=2.19e-06, adam=1.67e-02),
    "A-ride-cc": dict(adv=0.0, latent=3.27e-07, recon=6.87e-08, grad=4.08e-07, rows=1.27e-07, adam=1.63e-02),
    "B-cc": dict(adv=0.0, latent=1.61e-07, recon=3.19e-08, grad=4.88e-07, rows=8.85e-08, adam=5.39e-02),
    "B-lc": dict(adv=0.0, latent=1.66e-07, recon=3.19e-08, grad=1.48e-05, rows=7.93e-08, latent_loss=3.95e-06, adam=5.36e-02),
    "B-ccm": dict(adv=0.0, latent=1.61e-07, recon=3.19e-08, grad=5.60e-08, grad_rest=5.07e-07, rows=1.37e-07, adam=5.39e-02),
    "C-cc": dict(adv=0.0, latent=2.68e-07, recon=3.78e-08, grad=4.21e-07, rows=8.91e-08, adam=1.62e-02),
    "C-cp": dict(adv=0.0, latent=2.68e-07, recon=3.77e-08, grad=8.60e-08, rows=1.19e-07, adam=1.11e-02),
    "C-ride-cc": dict(adv=0.0, latent=2.68e-07, recon=3.78e-08, grad=4.21e-07, rows=8.91e-08, adam=1.62e-02),
    "D-cc": dict(adv=0.0, latent=1.87e-07, recon=3.89e-08, grad=4.10e-07, rows=7.44e-08, adam=1.66e-02),
    "D-ccm": dict(adv=0.0, latent=1.87e-07, recon=3.89e-08, grad=7.99e-08, grad_rest=4.10e-07, rows=9.52e-08, adam=1.66e-02),
    "E-cc": dict(adv=0.0, latent=2.14e-07, recon=3.56e-08, grad=4.71e-07, rows=1.06e-07, adam=3.12e-02),
    "E-lc": dict(adv=0.0, latent=1.94e-07, recon=2.71e-08, grad=1.49e-05, rows=1.39e-07, latent_loss=4.50e-06, adam=3.12e-02),
    "E-cp": dict(adv=0.0, latent=2.12e-07, recon=2.89e-08, grad=1.30e-07, rows=1.25e-07, adam=1.12e-02),
    "E-lp": dict(adv=0.0, latent=1.32e-07, recon=2.71e-08, grad=2.32e-06, grad_rest=1.58e-05, rows=2.41e-07, latent_loss=7.59e-06, adam=1.12e-02),
    "E-ccm": dict(adv=0.0, latent=2.14e-07, recon=3.56e-08, grad=6.50e-08, grad_rest=4.71e-07, rows=1.21e-07, adam=1.10e-02),
    "E-lcm": dict(adv=0.0, latent=1.94e-07, recon=2.71e-08, grad=1.49e-05, grad_rest=1.49e-05, rows=1.32e-07, latent_loss=4.50e-06, adam=1.67e-02),
    "F5000-cc": dict(adv=0.0, latent=1.99e-07, recon=2.11e-08, grad=1.70e-07, rows=1.29e-07, adam=3.05e-02),
    "F5000-ccm": dict(adv=0.0, latent=1.99e-07, recon=2.11e-08, grad=3.46e-08, grad_rest=1.70e-07, rows=1.16e-07, adam=1.64e-02),
    "F5000-lcm": dict(adv=0.0, latent=2.78e-07, recon=2.18e-08, grad=3.44e-05, grad_rest=3.44e-05, rows=9.03e-08, latent_loss=5.58e-06, adam=1.64e-02),
    "F5001-cc": dict(adv=0.0, latent=1.99e-07, recon=2.04e-08, grad=3.40e-07, rows=1.22e-07, adam=1.15e-02),
    "F5001-ccm": dict(adv=0.0, latent=1.99e-07, recon=2.04e-08, grad=6.37e-08, grad_rest=3.40e-07, rows=9.71e-08, adam=1.15e-02),
    "F5001-lcm": dict(adv=0.0, latent=2.78e-07, recon=2.01e-08, grad=3.44e-05, grad_rest=3.44e-05, rows=8.71e-08, latent_loss=5.10e-06, adam=3.14e-02),
    "G10001-cc": dict(adv=0.0, latent=1.62e-07, recon=1.78e-08, grad=2.98e-07, rows=7.45e-08, adam=1.67e-02),
    "G10001-lo-ccm": dict(adv=0.0, latent=1.62e-07, recon=1.78e-08, grad=6.41e-08, grad_rest=2.98e-07, rows=1.12e-07, adam=1.67e-02),
    "G10001-hi-ccm": dict(adv=0.0, latent=1.62e-07, recon=1.78e-08, grad=6.54e-08, grad_rest=2.98e-07, rows=9.05e-08, adam=1.67e-02),
    "G15000-cc": dict(adv=0.0, latent=1.96e-07, recon=1.38e-08, grad=6.57e-07, rows=9.39e-08, adam=1.04e-02),
    "H15001-cc": dict(adv=0.0, latent=1.32e-07, recon=1.50e-08, grad=4.32e-07, rows=7.10e-08, adam=1.05e-02),
    "H15001-ccm": dict(adv=0.0, latent=1.32e-07, recon=1.50e-08, grad=6.84e-08, grad_rest=4.32e-07, rows=7.88e-08, adam=1.05e-02),
    "H15001-cp": dict(adv=0.0, latent=1.50e-07, recon=1.37e-08, grad=4.08e-08, rows=8.21e-08, adam=1.15e-02),
    "H15001-lc": dict(adv=0.0, latent=2.18e-07, recon=1.37e-08, grad=1.32e-05, rows=3.46e-08, latent_loss=5.27e-06, adam=1.63e-02),
    "H16385-cc": dict(adv=0.0, latent=1.32e-07, recon=1.44e-08, grad=4.33e-07, rows=4.93e-08, adam=1.02e-02),
}

# b, n, Configuration arguments, what _test_plan() must report (rows: for chamfer / chamfer; H and body: of the fixed-point gradient)
CASES = {
    "A": dict(b=16, n=256, conf={}, screened=False, rtiles=1, rslices=8, rows="packed", loss="fused", body="1pass", H=1),
    "A-ride": dict(b=16, n=256, conf={"loss_in_scan": "always"}, screened=False, rtiles=1, rslices=8, rows="packed", loss="riders",
                   body="1pass", H=1),
    "B": dict(b=33, n=2048, conf={"chamfer_prune": "always"}, scattered=True, screened=False, rtiles=1, rslices=8, rows="packed",
              loss="fused", body="1pass", H=1),
    "C": dict(b=32, n=1025, conf={"chamfer_prune": False}, screened=False, rtiles=1, rslices=5, rows="partials", loss="fused",
              body="1pass", H=1),
    "C-ride": dict(b=32, n=1025, conf={"chamfer_prune": False, "loss_in_scan": "always"}, screened=False, rtiles=1, rslices=5,
                   rows="partials", loss="riders", body="1pass", H=1),
    "D": dict(b=64, n=2048, conf={"chamfer_prune": False}, screened=True, rtiles=1, rslices=2, rows="partials", loss="fused",
              body="1pass", H=1),
    "E": dict(b=3, n=2049, conf={"chamfer_prune": "always"}, screened=False, rtiles=2, rslices=33, rows="merge_launch", loss="fused",
              body="general", H=1),
    "F5000": dict(b=2, n=5000, conf={"chamfer_prune": False}, screened=False, rtiles=3, rslices=40, rows="merge_launch", loss="fused",
                  body="general", H=1),
    "F5001": dict(b=2, n=5001, conf={"chamfer_prune": False}, screened=False, rtiles=3, rslices=40, rows="merge_launch", loss="fused",
                  body="general", H=2, boundary=True),
    "G10001": dict(b=1, n=10001, conf={}, screened=False, rtiles=5, rslices=40, rows="merge_launch", loss="fused", body="general", H=3),
    "G10001-lo": dict(b=1, n=10001, conf={}, screened=False, rtiles=5, rslices=40, rows="merge_launch", loss="fused", body="general", H=3,
                      boundary=-1),
    "G10001-hi": dict(b=1, n=10001, conf={}, screened=False, rtiles=5, rslices=40, rows="merge_launch", loss="fused", body="general", H=3,
                      boundary=0),
    "G15000": dict(b=1, n=15000, conf={}, screened=False, rtiles=8, rslices=59, rows="merge_launch", loss="fused", body="general", H=3),
    "H15001": dict(b=1, n=15001, conf={}, screened=False, rtiles=8, rslices=59, rows="merge_launch", loss="metrics", body="sorted", H=0),
    "H16385": dict(b=1, n=16385, conf={}, screened=True, rtiles=9, rslices=65, rows="merge_launch", loss="metrics", body="sorted", H=0),
}

RUNS = ([("A", v) for v in ALL] + [("A-ride", "cc")] + [("B", v) for v in ("cc", "lc", "ccm")] + [("C", "cc"), ("C", "cp"), ("C-ride", "cc")]
        + [("D", "cc"), ("D", "ccm")] + [("E", v) for v in ALL] + [(c, v) for c in ("F5000", "F5001") for v in ("cc", "ccm", "lcm")]
        + [("G10001", "cc"), ("G10001-lo", "ccm"), ("G10001-hi", "ccm"), ("G15000", "cc")]
        + [("H15001", v) for v in ("cc", "ccm", "cp", "lc")] + [("H16385", "cc")])

_MODEL = {}


def _model(n):
    """Victim, its GPU handle and the float64 model at n points (one size is kept: the large decoders are 100 MB each in float64)."""
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.autoencoder import PointNetAE
    from oracle.attack_model import AEModel
    if n not in _MODEL:
        _MODEL.clear()
        w = W.randomized_weights(n)
        _MODEL[n] = (w, PointNetAE(w, n), AEModel(W.canonical(w, n), n, np.float64))
    return _MODEL[n]


def _sel(b):
    """Clouds are independent: of a large batch the first, one past a multiple of 8 and the last are compared in float64."""
    return list(range(b)) if b <= 3 else [0, 9, b - 1]


def _steer_points(case, H):
    """Per cloud, the point that carries the large perturbation: point 0, point n - 1, and (boundary cases) either side of a part
    boundary of the general gradient body -- parts are ranges of ceil(n / H) receiving points (H from the read-out)."""
    b, n = case["b"], case["n"]
    if "boundary" in case and H > 1:
        edge = -(-n // H)
        pts = [edge - 1, edge] if case["boundary"] is True else [edge + case["boundary"]]
    else:
        pts = [0, n - 1, n // 3]
    at = np.array([pts[c % len(pts)] for c in range(b)])
    sel = _sel(b)
    at[sel] = [pts[i % len(pts)] for i in range(len(sel))]               # the clouds compared in float64 cover every position
    return at


def _inputs(case, jpos, tie=None):
    """Clouds and the starting perturbation.  Scattered (the _inputs of test_gpu_backward_chain.py): duplicated target / source
    columns in the first and the last column slice, cloud 0 perturbed far enough that the paired search hands it back.  tie = (j1, j2):
    source point j1 duplicated at j2 and both given the same large perturbation -- bit-equal distances and norms."""
    from conftest import cloud
    b, n = case["b"], case["n"]
    x, gt = cloud(601, b, n), cloud(602, b, n)
    rng = np.random.default_rng(603)
    p0 = (1e-3 * rng.standard_normal((b, n, 3))).astype(np.float32)
    if case.get("scattered"):
        for a in (x, gt):
            a[:, n // 2] = a[:, 3]
            a[:, n - 1] = a[:, 3]
        p0[0] = (0.3 * (rng.random((n, 3)) - 0.5)).astype(np.float32)
    p0[np.arange(b), jpos, 0] += np.float32(STEER)
    if tie:
        j1, j2 = tie
        x[:, j2] = x[:, j1]
        p0[:, j2] = p0[:, j1]
    return x, gt, p0


class _Run:
    """One handle, its float64 twin on the selected clouds, and the checked iteration."""

    def __init__(self, name, variant, tie=None):
        from geometric_adv_amd.adv_ae import AdvAE, Configuration
        self.name, self.variant = name, variant
        case = self.case = CASES[name]
        self.adv_type, self.dist_type, self.kw = VARIANTS[variant]
        b, n = case["b"], case["n"]
        self.w, self.ae, self.model = _model(n)
        conf = Configuration(batch_size=b, n_points=n, weights=self.w, loss_adv_type=self.adv_type, loss_dist_type=self.dist_type,
                             num_iterations=10, num_iterations_thresh=1, learning_rate=LR, **case["conf"], **self.kw)
        self.at = AdvAE("adversary", conf, ae=self.ae)
        self.tie = tie
        self.jpos = _steer_points(case, case["H"]) if tie is None else np.full(b, tie[0])
        self.x, self.gt, self.p0 = _inputs(case, self.jpos, tie)
        self.sel = _sel(b)
        self.dw = np.resize(np.array([1.0, 150.0, 0.3], np.float32), b)          # per-cloud weights that differ,
        self.dw[self.sel] = self.dw[:len(self.sel)]                              # also among the clouds compared in float64
        self.tz = self.ae.transform(self.gt).astype(np.float32)
        self.at.set_inputs(self.x, self.gt, self.tz, self.dw)
        self.at.init_pert(self.p0, reset_optimizer=True)
        self.am = self.twin()
        self.worst = {}

    def twin(self, dw=None, **over):
        """The float64 model of the selected clouds (sensitivity: with other weights / dist_weight)."""
        from oracle.attack_model import AttackModel
        sel = self.sel
        kw = dict(max_point_pert_weight=self.kw.get("max_point_pert_weight", 0.0), max_point_dist_weight=self.kw.get("max_point_dist_weight", 0.0))
        kw.update(over)
        am = AttackModel(self.model, self.x[sel], self.gt[sel], self.tz[sel].astype(np.float64), (self.dw if dw is None else dw)[sel],
                         self.adv_type, self.dist_type, lr=LR, **kw)
        am.init_pert(self.p0[sel])
        return am

    def assert_form(self):
        """The read-out of the plan: this case runs the form it was written for."""
        case, v = self.case, self.variant
        p = self.at._test_plan()
        got = {k: p[k] for k in ("symmetric", "screened", "rtiles", "rslices", "rows", "loss", "grad", "H")}
        cc = v == "cc"
        one_slice = case["rtiles"] == 1 and case["rslices"] == 1
        fixed = {"1pass": "_1pass", "general": "_general"}.get(case["body"])
        if v == "lp":
            loss, grad = "metrics", "none"
        elif v in ("ccm", "lcm"):
            loss, grad = "metrics", "step_fx" + fixed if fixed else "step_sorted"
        else:
            loss, grad = (case["loss"] if cc or case["loss"] == "metrics" else "fused"), "fused" + fixed if fixed else "step_sorted"
        want = dict(symmetric=True, screened=case["screened"], rtiles=case["rtiles"], rslices=case["rslices"],
                    rows=case["rows"] if cc else "final" if one_slice else "merge_launch", loss=loss, grad=grad,
                    H=case["H"] if grad not in ("none", "step_sorted") else 0)
        assert got == want, "%s/%s runs another form than the one this case was written for" % (self.name, v)
        if "boundary" in case and self.tie is None:
            # _steer_points mirrors cgrad_fx_range; the library's own range says whether the steered points straddle a part boundary
            assert grad.endswith("general") and p["H"] > 1 and p["range"] < case["n"]
            side = self.jpos // p["range"]
            assert set(self.jpos % p["range"]) <= {0, p["range"] - 1} and (side[self.jpos % p["range"] == 0] >= 1).all(), \
                "the steered points do not lie beside a part boundary of the gradient body"
            if case["boundary"] is True:
                assert len(set(side[self.sel])) == 2, "the compared clouds do not straddle the boundary"
        return p

    def note(self, what, err):
        err = float(err)
        assert np.isfinite(err), "%s/%s: the error of %s is %r" % (self.name, self.variant, what, err)      # (max(0.0, nan) is 0.0)
        self.worst[what] = max(self.worst.get(what, 0.0), err)

    def peek(self):
        s = {k: t.cpu().numpy() for k, t in self.at.peek().items()}
        for k, a in s.items():
            assert np.isfinite(a).all(), "%s/%s: the GPU's %s is not finite" % (self.name, self.variant, k)
        return s

    def check_indices(self, s, oracle):
        """exact indices: the pinned oracle on the GPU's own clouds"""
        sel = self.sel
        _, i1, _, i2 = oracle.nn_distance(s["recon"][sel], self.gt[sel])
        assert np.array_equal(s["idx_r1"][sel], i1) and np.array_equal(s["idx_r2"][sel], i2), "indices of (recon, target)"
        _, i1, _, i2 = oracle.nn_distance(s["adv"][sel], self.x[sel])
        assert np.array_equal(s["idx_a1"][sel], i1) and np.array_equal(s["idx_a2"][sel], i2), "indices of (adv, source)"

    @staticmethod
    def pinned(s, sel):
        return tuple(s[k][sel] for k in ("idx_r1", "idx_r2", "idx_a1", "idx_a2"))

    def iteration(self, it, oracle, s=None):
        """One iteration from the GPU's own state; returns what the sensitivity tests need."""
        import torch
        at, am, sel = self.at, self.am, self.sel
        b = self.case["b"]
        s = s if s is not None else self.peek()                           # forward of the current pert
        am.pert = s["pert"][sel].astype(np.float64)                       # re-sync the model to the GPU state
        self.check_indices(s, oracle)
        f = am.forward(idx_override=self.pinned(s, sel))                  # (adv, latent, recon do not depend on the matches)
        for k, mk in (("adv", "adv"), ("latent", "z"), ("recon", "recon")):
            self.note(k, np.abs(s[k][sel] - f[mk]).max())
        g = am.gradient(f)
        jstar = self.assert_form()["jstar"].cpu().numpy()                 # this forward's form; the arg-max points the step will use
        hist = torch.empty((1, 6, b), device=self.ae.device)
        at.run(it, 1, 1, hist)
        s2 = self.peek()
        scale = np.abs(g).reshape(len(sel), -1).max(1)[:, None, None]
        assert (scale > 0).all()
        self.note("grad", np.abs(s2["grad"][sel] / scale - g / scale).max())
        row = 0 if self.kw.get("max_point_dist_weight", 0.0) > 0 else 1 if self.kw.get("max_point_pert_weight", 0.0) > 0 else None
        if row is not None:
            # the max-point term makes its point the cloud's largest component by far (STEER); the same bound for the other
            # points against THEIR largest component, so that the term's size does not hide them
            rest = np.ones(g.shape[:2], bool)
            rest[np.arange(len(sel)), jstar[row][sel]] = False
            rs = np.where(rest[..., None], np.abs(g), 0).reshape(len(sel), -1).max(1)[:, None, None]
            assert (rs > 0).all()
            self.note("grad_rest", (np.abs(s2["grad"][sel] - g) * rest[..., None] / rs).max())
        # Adam from the GPU's own gradient (isolates the update rule)
        am.adam(s2["grad"][sel].astype(np.float64))
        self.note("adam", (np.abs(s2["pert"][sel] - am.pert) / (2e-8 + 2e-6 * np.abs(am.pert))).max())
        # metrics row of this iteration = losses of the UPDATED pert (its indices are checked by the caller's next look)
        am.pert = s2["pert"][sel].astype(np.float64)
        f2 = am.forward(idx_override=self.pinned(s2, sel))
        h = hist.cpu().numpy()[0][:, sel]
        assert np.isfinite(hist.cpu().numpy()).all(), "%s/%s: a history row is not finite" % (self.name, self.variant)
        fourth = f2["loss_max"] if self.dist_type == "pert" else f2["max_dist"]
        for r, (row, want) in enumerate(zip(h, [f2["loss_adv"], f2["loss_dist"], f2["loss_pert"], fourth, f2["input_dist"], f2["loss_ae"]])):
            latent_loss = r == 0 and self.adv_type == "latent"
            self.note("latent_loss" if latent_loss else "rows", (np.abs(row - want) / np.maximum(np.abs(want), 1e-30)).max())
        return dict(s=s, s2=s2, f=f, g=g, scale=scale, jstar=jstar)

    def report(self):
        print("\n%-10s %-4s " % (self.name, self.variant) + "  ".join("%s %.2e" % (k, self.worst[k]) for k in TOL if k in self.worst))

    def assert_within(self, tol=TOL):
        self.report()
        for k, v in self.worst.items():
            assert v <= tol[k], "%s/%s: %s off by %.3e (bound %.1e)" % (self.name, self.variant, k, v, tol[k])


def _assert_steered(run, out, clouds=None):
    """The max-point terms sit where the test put them: the jstar the GPU used is the steered point (and the model's own arg-max)."""
    sel = run.sel
    for row, key, model_arg in ((0, "max_point_dist_weight", out["f"]["A1"].argmax(1)), (1, "max_point_pert_weight", out["f"]["p2"].argmax(1))):
        if run.kw.get(key, 0.0) > 0:
            got = out["jstar"][row][sel]
            assert np.array_equal(got, model_arg), "jstar differs from the float64 model's arg-max"
            keep = [i for i, c in enumerate(sel) if clouds is None or c in clouds]
            assert np.array_equal(got[keep], run.jpos[sel][keep]), "jstar is not the steered point"


@pytest.mark.parametrize("name,variant", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_two_iterations_match_model_in_every_form(oracle, name, variant):
    """Two consecutive iterations in the asserted form, each checked from the GPU's own state."""
    run = _Run(name, variant)
    run.assert_form()
    steered = None if not run.case.get("scattered") else set(range(1, run.case["b"]))      # (cloud 0 of B is scattered: no single large entry)
    for it in range(2):
        out = run.iteration(it, oracle)
        _assert_steered(run, out, steered)
    run.check_indices(out["s2"], oracle)                                  # the last history row's matches
    run.assert_form()                                                     # the last forward's form (iteration() asserts the others')
    run.assert_within()


@pytest.mark.parametrize("name,tie", [("A", (5, 5 + 2 * 64 + 1)), ("B", (5, 5 + 3 * 256 + 64))])
def test_exact_tie_of_the_max_point_goes_to_the_lowest_index(oracle, name, tie):
    """Source point j1 duplicated at j2 -- another thread and another wave of the loss row -- with the same large perturbation:
    bit-equal distances and norms, so both arg-max searches must return j1 (tf.argmax: the first), and the model pinned to j1 matches."""
    run = _Run(name, "ccm", tie=tie)
    run.assert_form()
    out = run.iteration(0, oracle)
    clouds = [c for c in run.sel if not (run.case.get("scattered") and c == 0)]
    for c in clouds:
        a = out["s"]["adv"][c]
        assert np.array_equal(a[tie[0]], a[tie[1]])
    js = out["jstar"]
    assert (js[0][clouds] == tie[0]).all() and (js[1][clouds] == tie[0]).all()
    keep = [i for i, c in enumerate(run.sel) if c in clouds]
    assert (out["f"]["A1"].argmax(1)[keep] == tie[0]).all()               # the model's own first maximum: the gradient compared is pinned to j1
    run.assert_within()


@pytest.mark.parametrize("name,variant", [("A", "cc"), ("A", "ccm"), ("A", "lp"), ("B", "cc"), ("B", "ccm")])
def test_altered_models_fail_the_gradient_tolerance(oracle, name, variant):
    """The comparison can fail: the GPU's gradient lies at least 10 tolerances away from the model without the max-point term, with
    dist_weight all ones (clouds whose weight is not one), and -- ccm -- with the term pinned to the neighbouring point."""
    run = _Run(name, variant)
    run.assert_form()
    out = run.iteration(0, oracle)
    run.assert_within()
    sel, b = run.sel, run.case["b"]
    got = out["s2"]["grad"][sel] / out["scale"]

    def away(am, f_edit=None):
        am.pert = out["s"]["pert"][sel].astype(np.float64)
        f = am.forward(idx_override=run.pinned(out["s"], sel))
        if f_edit:
            f_edit(f)
        return np.abs(got - am.gradient(f) / out["scale"]).reshape(len(sel), -1).max(1)

    alt = {"dist_weight all ones": away(run.twin(dw=np.ones(b, np.float32)))[run.dw[sel] != 1.0]}
    if run.kw:
        alt["max-point term off"] = away(run.twin(max_point_pert_weight=0.0, max_point_dist_weight=0.0))
    if variant == "ccm":
        def neighbour(f):
            j = f["A1"].argmax(1)
            f["A1"] = f["A1"].copy()
            f["A1"][np.arange(len(sel)), (j + 1) % run.case["n"]] = np.inf
        alt["max-point term on the neighbouring point"] = away(run.twin(), neighbour)
    for what, d in alt.items():
        print("%s/%s %s: %s tolerances away" % (name, variant, what, np.round(d / TOL["grad"], 1)))
        assert len(d) and (d >= 10 * TOL["grad"]).all(), what


@pytest.mark.parametrize("name", ["A-ride", "B"])
def test_keep_best_in_the_new_forms(name):
    """Keep-best from iteration 1 on (thresh = 1), one iteration per call: get_best returns, bit for bit, the adv / recon of the
    iteration with the strictly smallest loss_ae per cloud (the first minimum), and that value as the error."""
    import torch
    run = _Run(name, "cc")
    run.assert_form()
    at, b, iters = run.at, run.case["b"], 6
    snaps, errs = [], []
    for it in range(iters):
        hist = torch.empty((1, 6, b), device=run.ae.device)
        at.run(it, 1, 1, hist)
        s = at.peek()
        snaps.append((s["adv"].clone(), s["recon"].clone()))
        errs.append(hist[0, 5].clone())
    run.assert_form()
    ref = torch.ones(b)
    metrics, adv, recon = at.get_best(ref)
    errs = torch.stack(errs).cpu().numpy()
    metrics = metrics.cpu().numpy()
    assert np.isfinite(errs).all() and np.isfinite(metrics).all()
    k = errs.argmin(0)                                                    # np.argmin = first minimum = strict '<'
    print("\n%s: best iteration per cloud %s" % (name, k.tolist()))
    # the strict '<' is exercised: loss_ae is not monotone for every cloud -- the best iteration differs between clouds, and for
    # some cloud it is neither the first nor the last (later, larger values must not replace it)
    assert len(set(k.tolist())) >= 2 and ((k > 0) & (k < iters - 1)).any()
    for j in range(b):
        assert metrics[j, 4] == errs[k[j], j]
        assert torch.equal(adv[j], snaps[k[j]][0][j]) and torch.equal(recon[j], snaps[k[j]][1][j])
