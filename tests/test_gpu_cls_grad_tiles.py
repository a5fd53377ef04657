"""GPU: the classifier's input gradient (csrc/cls_grad.hip) against the float64 model of tests/_cls_grad_model64.py at the
sizes the attacks run at -- 200 ... 900 distinct winner rows per pool, i.e. 4 ... 15 slot tiles of cls_rows_kernel, and 4, 2
and 1 column slices of cls_winner_kernel -- where tests/test_gpu_cls_grad.py stops at n = 130 (3 tiles, 4 slices).

CLOUDS.  Points on a sphere, 0.45 v / |v| with v normal: the most distinct winners per point.  Per (classes, n, b) two compared
clouds (CASE_SEED) at the first and the last position of the batch; the rest of a batch is filler that no model sees.

   n     b    row tiles x clouds   slices (host_util.h: pooled_slices)   distinct winners, pool 0 / 1 / 2   slot tiles
   700    2          22             4                                     450-474 / 280-381 / 228-362        8 / 5-6 / 4-6
  1024   12         192             4                                     538-577 / 329-466 / 261-431        9-10 / 6-8 / 5-7
  1024   16         256             2                                     554-578 / 324-453 / 267-432        9-10 / 6-8 / 5-7
  1024   32         512             1                                     558-581 / 331-454 / 270-429        9-10 / 6-8 / 5-7
  2048    2          64             4                                     707-723 / 422-582 / 360-556        12 / 7-10 / 6-9
  8192    1         128             4                                     916 / 794 / 780                    15 / 13 / 13
(the ranges are over the two classifiers, 13 and 40 classes, and both clouds, from the float64 model.)  pooled_slices doubles
the slices while tiles x clouds x slices < 512: 2 slices need 256 <= tiles x clouds < 512, so the batch of 12 that was meant
to reach them runs with 4 and the batch of 16 is here beside it; 1 slice is what the attacks' 32 x 1024 get.  The last line
is the MOST TILES case (16 row tiles launched): the cloud with the most distinct winners in one pool that
tools/cls_grad_tolerance.py --tiles found among spheres of 8192 points, radius 0.45 and 1, seeds 0 .. 5, both classifiers
(860 ... 921 winners in pool 0; the one with 921 has two fc1 units inside the head window and is left out).  It reaches 916
winners in pool 0 (40 classes, seed 2): slot tile 15 of 16.  None of the 24 searched clouds passes 960 slots, so THE 16TH SLOT
TILE STAYS WITHOUT A REFERENCE; test_one_winner_among_sixteen_row_tiles launches all 16 row tiles, 15 of them through the
early exit.

METHOD.  A ReLU unit whose float64 pre-activation lies within the float32 forward's error of zero may be masked the other
way on the GPU, which moves a path's gradient, not a rounding.  At n >= 512 almost every cloud has such units (a handful to 40
of its 250 000 ... 500 000 units on winner paths), so no cloud could be kept by test_gpu_cls_grad.py's whole-cloud screen.  Here a
unit inside its WINDOW is OPEN (G.open_units) and is resolved instead: per cloud the op's winners are validated against
float64 and handed to the model; the gradient is compared row by row (max-abs error of the row / the cloud's max-abs
gradient); for a row beyond TOL_GRAD the open per-point units ON THAT ROW are tried the other way (G.grad_model's
relu_override), one at a time, then in pairs.  A flip is accepted only if it brings that row within TOL_GRAD; tries are made
on top of the flips accepted so far, the worst row first, and the run with all accepted flips must have every row within
TOL_GRAD.  A failing row without an open unit, or that no allowed flip explains, fails the test.

MEASURED, not chosen (tools/cls_grad_tolerance.py --tiles: the SAME torch graph in float32 on the CPU, winners and ReLU masks
pinned from float64, against float64; the forward errors on seeds 0 .. 7 of every (classes, n), two clouds of 8192 points and
this file's compared clouds, the gradient error on the compared clouds and the most-tiles cloud, all three losses):
  F32_PRE_ERR[layer], max |pre32 - pre64| / max |pre64| over a cloud, worst cloud:   2.2e-7 (tconv1) ... 5.5e-6 (T-Net2 tfc1)
  F32_LOGIT_ERR, max-abs / max |Z|:                                                  7.47e-6
  F32_GRAD_ERR, max-abs over the cloud / the cloud's max-abs gradient, worst:        7.20e-6
  (n <= 130, cube clouds: 2.3e-7 ... 3.7e-5, 3.42e-5 and 2.41e-5 -- the dW sums here run over up to 16 times as many rows,
  yet sphere clouds of this size leave torch's float32 closer to float64 than the small cube clouds did.)
TOL_GRAD = 4 x F32_GRAD_ERR: the factor test_gpu_cls_grad.py gives this kernel (an fp32 chain summed in another order, with
the head kernels' sequential 1024-term chains, earned the forward about 4 x torch's error).
WINDOW = 2 x F32_PRE_ERR for the per-point layers (1 x in the small-n file; an open unit is resolved here, not left out, so
a wider window costs only model runs) and 8 x for the head layers (the small-n file's 4 for the heads' sequential 1024-term
chains, times the same 2).  No window exceeds TOL_FWD (asserted at import).
CAPS that keep the method from hiding a failure, asserted on the model fed with the GPU's winners (the seeds were chosen on
the CPU with the float64 model alone so that they hold): no head unit is open; the CW margins keep 1.25 x 4 x F32_LOGIT_ERR;
a cloud's open per-point units are at most MAX_OPEN = 64 and at most 8 % of its distinct winner rows summed over the three
pools; accepted flips never exceed the open units, and over the whole file stay under 2 % of the winner rows.
test_wrong_models_fail_with_flips_allowed (CPU) feeds the comparison gradients with a slot tile left out of dW3', pool 1 left
out of dW1', and a winner row above 1023 cut to its low 10 bits: each fails although flips are allowed.
Loss and logits: test_gpu_cls_grad.py's TOL_FWD rules.
SEEN on the MI355X: 61 comparisons, 602 open units (6 ... 17 per cloud), 31 accepted flips (0 ... 2 per cloud, 4 on the
most-tiles cloud) on 82 833 winner rows; a flipped unit moved its row by 4e-4 ... 4e-2 of the cloud's largest gradient; the
worst row after the flips 1.41e-5 (1e-6 ... 6e-6 on most clouds) against TOL_GRAD = 2.88e-5.

BIT-EXACT (no margin): batch position, chunking and slices (4 / 4 / 2 / 1, and 1 then 4 inside one call of 70 clouds), a cloud
repeated after itself, one winner among 16 launched row tiles; a permutation moves every row to another slot and tile."""
import functools
import itertools

import numpy as np
import pytest

import _cls_grad_model64 as G

gpu = pytest.mark.gpu

F32_GRAD_ERR = 7.20e-06
F32_LOGIT_ERR = 7.47e-06
F32_PRE_ERR = {"transform_net1/tconv1": 2.24e-07, "transform_net1/tconv2": 7.61e-07, "conv1": 1.83e-06, "conv2": 2.35e-06,
               "transform_net2/tconv1": 3.65e-06, "transform_net2/tconv2": 4.62e-06, "conv3": 3.00e-06, "conv4": 4.13e-06,
               "transform_net1/tfc1": 1.44e-06, "transform_net1/tfc2": 1.42e-06, "transform_net2/tfc1": 5.54e-06,
               "transform_net2/tfc2": 4.37e-06, "fc1": 5.23e-06, "fc2": 5.25e-06}
TOL_GRAD = 4 * F32_GRAD_ERR
TOL_FWD = 1e-4
WINDOW = {s: (8 if s in G.HEADS else 2) * e for s, e in F32_PRE_ERR.items()}
assert all(v <= TOL_FWD for v in WINDOW.values())
MAX_OPEN, MAX_OPEN_FRACTION, MAX_FLIP_FRACTION = 64, 0.08, 0.02
KAPPA = 0.5
RADIUS = 0.45
CASES = ((700, 2), (1024, 12), (1024, 32), (2048, 2), (1024, 16))         # (n, b); the seeds are handed out in this order
CASE_SEED = {(13, 700, 2): (0, 1), (13, 1024, 12): (0, 1), (13, 1024, 32): (2, 3), (13, 2048, 2): (1, 2),
             (13, 1024, 16): (4, 5), (40, 1024, 16): (4, 5),
             (40, 700, 2): (0, 1), (40, 1024, 12): (0, 1), (40, 1024, 32): (2, 3), (40, 2048, 2): (0, 3)}      # (classes, n, b)
MOST_TILES = dict(num_classes=40, n=8192, seed=2, radius=RADIUS, loss="xent", pool=0, winners=916)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights(num_classes):
    from geometric_adv_amd import cls_weights as CW
    return CW.synthetic_weights(num_classes, seed=num_classes)


@functools.lru_cache(maxsize=None)
def _clf(num_classes):
    from geometric_adv_amd.classifier import PointNetClassifier
    return PointNetClassifier(None, num_classes=num_classes, weights=_weights(num_classes))


def sphere(seed, n, radius=RADIUS):
    """(n, 3) float32 on the sphere of that radius."""
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return (radius * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def labels_of(seed, num_classes, logits64):
    """{loss: label} that keeps every loss informative (test_gpu_cls_grad.py: make_case): the cross entropy and the targeted
    CW loss aim at a class the float64 model does not predict, the untargeted CW loss starts from the predicted one."""
    top = int(np.argmax(logits64))
    other = (top + 1 + int(np.random.default_rng([seed, 7]).integers(0, num_classes - 1))) % num_classes
    return {"xent": other, "cw_targeted": other, "cw_untargeted": top}


def fillers(n, count):
    return np.stack([sphere(10_000 + i, n) for i in range(count)]) if count else np.zeros((0, n, 3), np.float32)


def forward64(num_classes, x, margins=False):
    """The float64 model's own forward of one cloud (its winners, columns, pre-activations do not depend on the loss)."""
    return G.grad_model(_weights(num_classes), x[None], np.zeros(1, np.int64), "xent", margins=margins)


def row_err(got, ref_grad):
    """(n,) max-abs error of each row over the cloud's max-abs gradient."""
    scale = np.abs(ref_grad).max()
    return np.abs(np.asarray(got, np.float64) - ref_grad).max(-1) / (scale if scale > 0 else 1.0)


def describe_row(ref, row):
    """Where a row sits in each pool (slot, tile) and the unit closest to zero on its paths."""
    out = []
    for p in range(3):
        rows = G.winner_rows(ref, 0, p)
        k = int(np.searchsorted(rows, row))
        if k == len(rows) or rows[k] != row:
            out.append("pool %d: no winner" % p)
            continue
        near = min((float(np.abs(ref["pres"][s][0][row]).min() / np.abs(ref["pres"][s][0]).max()), s) for s in G.UNDER[p])
        out.append("pool %d: slot %d tile %d of %d, smallest |pre|/scale %.2e (%s, window %.2e)" %
                   (p, k, k // 64, -(-len(rows) // 64), near[0], near[1], WINDOW[near[1]]))
    return "; ".join(out)


def check_caps(ref, loss):
    """The three conditions of the header on a one-cloud result; returns its open per-point units and winner rows."""
    opens = G.open_units(ref, WINDOW)
    heads = [u for u in opens if u[2] is None]
    assert not heads, "head units inside the 8 x window: %s" % heads
    if loss != "xent":
        assert ref["margin_loss"][0] >= 1.25 * 4 * F32_LOGIT_ERR, "CW margin %.2e" % ref["margin_loss"][0]
    nrows = sum(len(G.winner_rows(ref, 0, p)) for p in range(3))
    assert len(opens) <= MAX_OPEN and len(opens) <= MAX_OPEN_FRACTION * nrows, "%d open units, %d winner rows" % (len(opens), nrows)
    return opens, nrows


def resolve(run, got, opens, hints=()):
    """run(flips) -> the model's one-cloud result with those (scope, 0, row, unit) flipped.  Returns (result, accepted flips,
    model runs) with every row of `got` within TOL_GRAD of the result's gradient, or raises AssertionError (see METHOD)."""
    def model(flips):
        ov = {}
        for s, c, row, unit in flips:
            ov.setdefault(s, []).append((c, row, unit, not base["pres"][s][c][row][unit] > 0))
        return run(ov)

    base = run({})
    ref, accepted, runs = base, [], 1
    by_row = {}
    for u in opens:
        by_row.setdefault(u[2], []).append(u)
    rank = {u: i for i, u in enumerate(hints)}
    while True:
        err = row_err(got, ref["grad"][0])
        failing = [int(r) for r in np.argsort(-err) if err[r] > TOL_GRAD]
        if not failing:
            return ref, accepted, runs
        for r in failing:
            cands = sorted((u for u in by_row.get(r, []) if u not in accepted), key=lambda u: rank.get(u, len(rank)))
            hit = None
            for combo in itertools.chain(((u,) for u in cands), itertools.combinations(cands, 2)):
                trial = model(accepted + list(combo))
                runs += 1
                if row_err(got, trial["grad"][0])[r] <= TOL_GRAD:
                    hit = (combo, trial)
                    break
            if hit:
                accepted, ref = accepted + list(hit[0]), hit[1]
                break
        else:
            r = failing[0]
            raise AssertionError("row %d off by %.2e (TOL_GRAD %.2e), %d rows failing, %d flips accepted, open units on the "
                                 "row %s: no allowed flip explains it.  %s" %
                                 (r, err[r], TOL_GRAD, len(failing), len(accepted), by_row.get(r, []), describe_row(ref, r)))


def compare_cloud(num_classes, x, y, loss, got, own, hints=()):
    """One cloud of one call against float64.  got = (loss, grad (n, 3), logits (C,), winners (3, 1024)) as numpy.  Returns a
    record dict; 'fail' holds the first failed assertion's text or None."""
    L, g, Z, win = got
    w = _weights(num_classes)
    rec = dict(fail=None, flips=[], opens=0, rows=0, err=np.inf, runs=0, winners=[0, 0, 0])
    try:
        _validate_winners(win[None], own)
        run = lambda ov, margins=False: G.grad_model(w, x[None], np.array([y]), loss, KAPPA, winners=win[None], relu_override=ov,
                                                     margins=margins)
        ref = run({}, margins=loss != "xent")                              # the CW margins are the only ones used
        rec["winners"] = [len(G.winner_rows(ref, 0, p)) for p in range(3)]
        zmax = max(1.0, np.abs(ref["logits"]).max())
        assert np.abs(Z - ref["logits"][0]).max() <= TOL_FWD * zmax
        assert abs(L - ref["loss"][0]) <= 2 * TOL_FWD * zmax
        assert np.abs(ref["grad"]).max() > 0
        opens, rec["rows"] = check_caps(ref, loss)
        rec["opens"] = len(opens)
        rec["err0"] = float(row_err(g, ref["grad"][0]).max())
        final, rec["flips"], rec["runs"] = resolve(lambda ov: run(ov) if ov else ref, g, opens, hints)
        rec["err"] = float(row_err(g, final["grad"][0]).max())
        assert len(rec["flips"]) <= len(opens) and rec["err"] <= TOL_GRAD
    except AssertionError as e:
        rec["fail"] = str(e) or repr(e)
    return rec


def _validate_winners(win, ref):
    from test_gpu_cls_grad import _validate_winners as validate
    validate(win, ref)


def _run_op(num_classes, x, y, loss):
    out = _clf(num_classes).input_gradient(_dev(x), _dev(np.asarray(y, np.int32)), loss, KAPPA, return_logits=True, return_winners=True)
    return [t.cpu().numpy() for t in out]


@functools.lru_cache(maxsize=None)
def _case(num_classes, n, b):
    """The three losses of one (classes, n, b): {loss: [record of cloud 0, record of cloud 1]} (computed once)."""
    seeds = CASE_SEED[(num_classes, n, b)]
    pos = (0, b - 1)
    x = fillers(n, b)
    y = {loss: np.arange(b) % num_classes for loss in G.LOSSES}
    owns = []
    for s, at in zip(seeds, pos):
        x[at] = sphere(s, n)
        owns.append(forward64(num_classes, x[at]))
        for loss, lab in labels_of(s, num_classes, owns[-1]["logits"][0]).items():
            y[loss][at] = lab
    got = {loss: _run_op(num_classes, x, y[loss], loss) for loss in G.LOSSES}
    out = {loss: [] for loss in G.LOSSES}
    for own, at in zip(owns, pos):
        hints = []
        for loss in G.LOSSES:
            rec = compare_cloud(num_classes, x[at], y[loss][at], loss, [t[at] for t in got[loss]], own, tuple(hints))
            hints += [u for u in rec["flips"] if u not in hints]            # the masks do not depend on the loss
            out[loss].append(rec)
    return out


def _report(tag, rec):
    print("%s: distinct winners %s, open units %d, accepted flips %d %s, model runs %d, worst row error %.2e before / %.2e after "
          "(TOL_GRAD %.2e)" % (tag, rec["winners"], rec["opens"], len(rec["flips"]), rec["flips"], rec["runs"],
                               rec.get("err0", np.inf), rec["err"], TOL_GRAD))


@gpu
@pytest.mark.parametrize("loss", G.LOSSES)
@pytest.mark.parametrize("n,b", CASES)
@pytest.mark.parametrize("num_classes", [13, 40])
def test_gradient_vs_float64_at_many_tiles(num_classes, n, b, loss):
    recs = _case(num_classes, n, b)[loss]
    for i, rec in enumerate(recs):
        _report("classes %d n %d b %d %s cloud %d" % (num_classes, n, b, loss, i), rec)
    for rec in recs:
        assert rec["fail"] is None, rec["fail"]
        assert max(rec["winners"]) > 3 * 64                                # beyond the third slot tile


@functools.lru_cache(maxsize=None)
def _most_tiles():
    m = MOST_TILES
    x = sphere(m["seed"], m["n"], m["radius"])
    own = forward64(m["num_classes"], x)
    y = labels_of(m["seed"], m["num_classes"], own["logits"][0])[m["loss"]]
    got = _run_op(m["num_classes"], x[None], [y], m["loss"])
    return compare_cloud(m["num_classes"], x, y, m["loss"], [t[0] for t in got], own)


@gpu
def test_most_tiles_vs_float64():
    rec = _most_tiles()
    _report("most tiles: classes %(num_classes)d n %(n)d seed %(seed)d %(loss)s" % MOST_TILES, rec)
    assert rec["fail"] is None, rec["fail"]
    assert rec["winners"][MOST_TILES["pool"]] >= MOST_TILES["winners"] - 2      # a near tie may move a winner or two


@gpu
def test_accepted_flips_stay_under_the_cap():
    """Over the whole file at most 2 % of the distinct winner rows took a flip (its cases are computed once)."""
    recs = [rec for C in (13, 40) for n, b in CASES for per in _case(C, n, b).values() for rec in per] + [_most_tiles()]
    flips, rows = sum(len(r["flips"]) for r in recs), sum(r["rows"] for r in recs)
    print("accepted flips %d, open units %d, winner rows %d over %d comparisons" % (flips, sum(r["opens"] for r in recs), rows, len(recs)))
    assert len(recs) == 2 * len(CASES) * 2 * 3 + 1 and all(r["fail"] is None for r in recs)
    assert flips <= MAX_FLIP_FRACTION * rows


# ------------------------------------------------------------------------------------------------ the comparison's own test
MUTATION_N, MUTATION_SEED = 1100, 0


def test_wrong_models_fail_with_flips_allowed():
    """CPU.  The float64 gradient itself passes with 0 flips; three wrong gradients of the same forward fail although
    every open unit may be flipped: one slot tile's rows left out of dW3', pool 1's partials left out of dW1', and a winner
    row above 1023 replaced by its low 10 bits (what a key of `row << 10 | column` cut to 20 bits would give)."""
    w, x = _weights(13), sphere(MUTATION_SEED, MUTATION_N)
    own = forward64(13, x)
    y = labels_of(MUTATION_SEED, 13, own["logits"][0])["cw_targeted"]
    run = lambda ov=None, margins=False, **kw: G.grad_model(w, x[None], np.array([y]), "cw_targeted", KAPPA, relu_override=ov,
                                                            margins=margins, **kw)
    ref = run(margins=True)
    opens, nrows = check_caps(ref, "cw_targeted")
    assert opens, "the case should allow flips"
    final, flips, runs = resolve(run, ref["grad"][0], opens)
    assert not flips and runs == 1
    rows2 = G.winner_rows(ref, 0, 2)
    assert len(rows2) > 128
    high = [r for p in range(3) for r in G.winner_rows(ref, 0, p) if r > 1023]
    r = max(high, key=lambda r: np.abs(ref["grad"][0][r]).max())
    cut = ref["winners"].copy()
    cut[cut == r] = r & 1023
    wrong = {"dW3' without slot tile 1 of pool 2": run(mutate={"dw3_drop_rows": [rows2[64:128]]}),
             "dW1' without pool 1": run(mutate={"dw1_drop_pool1": True}),
             "row %d -> %d" % (r, r & 1023): run(winners=cut)}
    for name, bad in wrong.items():
        assert np.array_equal(bad["logits"], ref["logits"]) or "row" in name
        worst = row_err(bad["grad"][0], ref["grad"][0]).max()
        print("%s: worst row error %.2e = %.1f x TOL_GRAD" % (name, worst, worst / TOL_GRAD))
        with pytest.raises(AssertionError, match="no allowed flip explains it"):
            resolve(run, bad["grad"][0], opens)


# ------------------------------------------------------------------------------------------------ bit-exact checks
def _equal(a, b):
    import torch
    return all(torch.equal(s, t) for s, t in zip(a, b))


def _op(clf, x, y, loss="cw_targeted"):
    return clf.input_gradient(_dev(x), _dev(np.asarray(y, np.int32)), loss, KAPPA, return_logits=True, return_winners=True)


def _live_labels(clf, x):
    """{loss: label} from the op's own logits of one cloud, so that no CW loss sits on its clamp (labels_of's rule)."""
    top = int(clf.forward(_dev(x[None]))[0][0].argmax().item())
    other = (top + 1) % clf.num_classes
    return {"xent": other, "cw_targeted": other, "cw_untargeted": top}


@gpu
def test_batch_position_chunks_and_slices_change_no_bit():
    """One cloud at n = 1024: alone and in a batch of 12 (16 and 192 tiles: 4 slices), of 16 (256 tiles: 2 slices), of 32 (1
    slice), and of 70 (the chunk of 64 with 1 slice, the last 6 clouds with 4): loss, gradient, logits and winners are the
    same bits."""
    clf, n = _clf(13), 1024
    cloud = sphere(77, n)
    others = fillers(n, 70)
    alone = _op(clf, cloud[None], [5])
    assert alone[3].max().item() > 0 and alone[1].abs().max().item() > 0
    for size, places in ((12, (0, 11)), (16, (0, 15)), (32, (0, 31)), (70, (3, 66))):
        batch, yb = others[:size].copy(), np.arange(size) % 13
        for at in places:
            batch[at], yb[at] = cloud, 5
        got = _op(clf, batch, yb)
        for at in places:
            assert _equal([t[at] for t in got], [t[0] for t in alone]), (size, at)


@gpu
def test_a_cloud_repeated_after_itself_changes_no_bit():
    """y = (x, x), n = 2048 against x, n = 1024: the second copy wins nothing (ties go to the lowest row), so the pools, T1,
    T2, the slots and the tile sums are x's, and nothing else may depend on n."""
    import torch
    clf = _clf(40)
    x = sphere(78, 1024)
    assert len(np.unique(x, axis=0)) == 1024
    for loss, y in _live_labels(clf, x).items():
        one = _op(clf, x[None], [y], loss)
        two = _op(clf, np.concatenate([x, x])[None], [y], loss)
        assert two[3].max().item() < 1024 and torch.equal(two[3], one[3])
        assert not two[1][0, 1024:].any().item()
        assert torch.equal(two[1][0, :1024], one[1][0]) and torch.equal(two[0], one[0]) and torch.equal(two[2], one[2])
        assert one[1].abs().max().item() > 0


@gpu
def test_one_winner_among_sixteen_row_tiles():
    """n = 1024 identical points: cnt = 1 in every pool while 16 row tiles are launched (15 leave at slot0 >= cnt)."""
    import torch
    clf = _clf(13)
    point = sphere(79, 1)
    for loss, y in _live_labels(clf, point).items():
        one = _op(clf, point[None], [y], loss)
        many = _op(clf, np.repeat(point, 1024, axis=0)[None], [y], loss)
        assert not many[3].any().item() and not many[1][0, 1:].any().item()
        assert many[1][0, 0].abs().max().item() > 0
        assert torch.equal(many[1][0, 0], one[1][0, 0]) and torch.equal(many[0], one[0]) and torch.equal(many[2], one[2])


@gpu
def test_permutation_moves_rows_to_other_tiles():
    """A compared n = 1024 cloud without tied maxima in float64: its winners permute exactly, the loss is the same bits, and
    the gradient is the permuted gradient within TOL_GRAD -- every row lands in another slot and tile, so only the tile order
    of the dW sums moved."""
    C, n, b = 13, 1024, 12
    seed = CASE_SEED[(C, n, b)][0]
    x = sphere(seed, n)
    own = forward64(C, x, margins=True)
    assert own["margin_pool"][0] > 0
    y = labels_of(seed, C, own["logits"][0])["xent"]
    perm = np.random.default_rng(4).permutation(n)
    L0, g0, Z0, w0 = _run_op(C, x[None], [y], "xent")
    L1, g1, Z1, w1 = _run_op(C, x[perm][None], [y], "xent")
    live = own["pooled"] > 0
    assert np.array_equal(perm[w1][live], w0[live]) and not w1[~live].any() and not w0[~live].any()
    assert L0[0] == L1[0]
    moved = sum(int((np.searchsorted(np.unique(w0[0, p][live[0, p]]), w0[0, p][live[0, p]]) // 64 !=
                     np.searchsorted(np.unique(w1[0, p][live[0, p]]), w1[0, p][live[0, p]]) // 64).any()) for p in range(3))
    assert moved == 3                                                   # in every pool some column's row changed its tile
    err = row_err(g1[0], g0[0][perm].astype(np.float64)).max()
    print("permuted gradient: worst row error %.2e (TOL_GRAD %.2e)" % (err, TOL_GRAD))
    assert err <= TOL_GRAD
