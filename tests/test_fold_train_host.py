"""CPU: the float64 model of the FoldingNet training step (tests/_fold_train_model64.py) and the host side of the trainer.

- the model's gradients against central finite differences in float64 on a tiny batch with every decision held;
- pinning fp64's own decisions reproduces the unpinned step;
- every mistake switch moves the float64 result by at least 10 x the tolerance test_gpu_fold_train.py uses for the quantity
  it moves (gradients: GRAD_TOL; parameters: PARAM_TOL of the update; running statistics: RUNNING_TOL), so those
  tolerances can still tell the mistakes apart;
- checkpoint round trip: fold_weights.save with an optimizer entry -> fold_weights.load / load_training, and
  torch.optim.Adam.load_state_dict on a plain module of the same shapes accepts the entry; the old call signature still
  writes the empty entry;
- the train-mode forward against the reference's own modules (tests/golden/foldingnet_train.npz, written by
  tools/make_golden_foldingnet_train.py from FoldingNet_graph().double().train(), ChamferLoss and build_graph);
- for every input batch of the GPU tests, torch float32 on the CPU takes at most PIN_SHARE of each layer's decisions
  differently from float64: pinning the GPU's decisions can then only absorb what rounding explains;
- initial_weights' bounds and shapes, the CLI's flags, the refusal of one-cloud batches.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _fold_model64 as F64  # noqa: E402
import _fold_train_model64 as M  # noqa: E402
import test_gpu_fold_train as G  # noqa: E402  (the tolerance constants only)
from geometric_adv_amd import fold_weights as FW  # noqa: E402

_CASE = {}


def tiny():
    if not _CASE:
        rng = np.random.default_rng(0)
        w = FW.synthetic_state(0)
        x = rng.random((3, 40, 3)) - 0.5
        cov, rows = F64.graph_from_knn(x, F64.knn(x))
        picks = np.stack([np.stack([np.stack([rng.choice(len(r), 16, replace=False) for r in rc]) for rc in rows]) for _ in range(2)])
        cols = F64.resolve(rows, picks)
        ref = M.step(w, x, cov, cols)
        pins = dict(relu=ref["relu"], win=ref["win"], gmax=ref["gmax"], hidden=ref["hidden"], chamfer=ref["chamfer"])
        _CASE.update(w=w, x=x, cov=cov, cols=cols, ref=ref, pins=pins)
    return _CASE


def test_pinning_its_own_decisions_reproduces_the_step():
    c = tiny()
    again = M.step(c["w"], c["x"], c["cov"], c["cols"], pins=c["pins"])
    assert all(v[0] == 0 for v in again["disagree"].values())
    assert again["loss"] == c["ref"]["loss"]
    for k, g in c["ref"]["grads"].items():
        assert np.array_equal(again["grads"][k], g), k


def test_gradients_match_central_finite_differences():
    c = tiny()
    rng = np.random.default_rng(1)
    h = 1e-6
    for k in ["encoder.conv1.weight", "encoder.bn2.weight", "encoder.conv4.weight", "encoder.bn5.weight", "encoder.conv5.weight",
              "encoder.fc1.weight", "encoder.bn6.bias", "encoder.fc2.bias", "decoder.fold1.conv1.weight", "decoder.fold1.conv3.bias",
              "decoder.fold2.conv1.weight", "decoder.fold2.conv2.weight"]:
        g = c["ref"]["grads"][k]
        d = rng.standard_normal(g.shape)
        d /= np.linalg.norm(d)
        losses = []
        for sign in (1, -1):
            w = dict(c["w"])
            w[k] = np.asarray(w[k], np.float64) + sign * h * d
            losses.append(M.step(w, c["x"], c["cov"], c["cols"], pins=c["pins"])["loss"])
        fd = (losses[0] - losses[1]) / (2 * h)
        an = float((g * d).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), np.linalg.norm(g) * 1e-2), (k, fd, an)


def _moved(ref, res, wd=1e-6):
    g = max(G._rel(res["grads"][k], ref["grads"][k]) for k in ref["grads"] if k not in G.FED_BIASES and np.any(ref["grads"][k]))
    old = tiny()["w"]
    p = max(G.param_error(res["new_state"][k], ref["new_state"][k], np.asarray(old[k], np.float64), ref["grads"][k] + wd * np.asarray(old[k], np.float64))
            for k in M.PARAM_KEYS if k not in G.FED_BIASES)
    r = max(float(np.abs(res["new_state"][k] - ref["new_state"][k]).max() / np.abs(ref["new_state"][k]).max())
            for k in ref["new_state"] if "running" in k)
    return g, p, r


@pytest.mark.parametrize("switch,quantity", [
    ("no_weight_decay", "param"), ("tf_adam_eps", "param"), ("biased_running_var", "running"), ("bn_no_m2", "grad"),
    ("pool_all", "grad"), ("pool_no_self", "grad"), ("chamfer_no_batch_mean", "grad"), ("relu_after_bn5", "grad")])
def test_every_mistake_moves_the_result_by_ten_tolerances(switch, quantity):
    c = tiny()
    # weight decay and Adam's epsilon only show where they are not negligible: sized up here as the GPU test cannot do
    kw = dict(weight_decay=1e-2) if switch == "no_weight_decay" else {}
    ref = M.step(c["w"], c["x"], c["cov"], c["cols"], **kw) if kw else c["ref"]
    res = M.step(c["w"], c["x"], c["cov"], c["cols"], perturb={switch: 2 if switch == "bn_no_m2" else True}, **kw)
    g, p, r = _moved(ref, res, kw.get("weight_decay", 1e-6))
    moved, tol = {"grad": (g, G.GRAD_TOL), "param": (p, G.PARAM_TOL), "running": (r, G.RUNNING_TOL)}[quantity]
    assert moved >= 10 * tol, (switch, moved, tol)


def test_checkpoint_round_trip_and_torch_accepts_the_optimizer_entry(tmp_path):
    w = FW.initial_weights(3)
    names = FW.parameter_names()
    rng = np.random.default_rng(0)
    opt = {"step": 5, "lr": 1e-4, "weight_decay": 1e-6,
           "exp_avg": {k: rng.standard_normal(w[k].shape).astype(np.float32) for k in names},
           "exp_avg_sq": {k: rng.random(w[k].shape).astype(np.float32) for k in names}}
    FW.save(str(tmp_path), 4, w, optimizer=opt, extra={"graph_ordinal": 40})
    state, got, ck = FW.load_training(str(tmp_path), 4)
    assert ck["epoch"] == 4 and ck["graph_ordinal"] == 40 and got["step"] == 5
    assert int(ck["model"]["encoder.bn3.num_batches_tracked"]) == 5
    for k in w:
        assert np.array_equal(state[k], w[k]), k
    for k in names:
        assert np.array_equal(got["exp_avg"][k], opt["exp_avg"][k]) and np.array_equal(got["exp_avg_sq"][k], opt["exp_avg_sq"][k])
    assert np.array_equal(FW.load(str(tmp_path), 4)["decoder.fold2.conv3.weight"], w["decoder.fold2.conv3.weight"])
    shapes = FW.key_shapes()
    params = [torch.nn.Parameter(torch.zeros(shapes[k])) for k in names]
    adam = torch.optim.Adam(params, lr=1e-4, weight_decay=1e-6)
    adam.load_state_dict(ck["optimizer"])
    assert float(adam.state[params[0]]["step"]) == 5
    assert np.array_equal(adam.state[params[-1]]["exp_avg"].numpy(), opt["exp_avg"][names[-1]])
    assert adam.param_groups[0]["lr"] == 1e-4 and adam.param_groups[0]["weight_decay"] == 1e-6
    FW.save(str(tmp_path), 9, w)                       # the old signature: an empty optimizer entry, as before
    assert FW.load_training(str(tmp_path), 9)[1] is None


def test_parameter_order_is_the_state_dict_order_without_buffers():
    names = FW.parameter_names()
    assert len(names) == 38 and names[0] == "encoder.conv1.weight" and names[14] == "encoder.bn1.weight"
    assert names[26] == "decoder.fold1.conv1.weight" and not any("running" in k or "tracked" in k for k in names)
    assert names == M.PARAM_KEYS


def test_initial_weights_follow_torchs_default_initialisation():
    w = FW.initial_weights(0)
    FW.validate(w)
    for k, shape in FW.key_shapes().items():
        assert w[k].shape == shape and w[k].dtype == np.float32
    for name, fi in (("encoder.conv1", 12), ("encoder.fc1", 1024), ("decoder.fold1.conv1", 514), ("decoder.fold2.conv3", 512)):
        bound = 1 / np.sqrt(fi)
        for f in ("weight", "bias"):
            a = w["%s.%s" % (name, f)]
            assert np.abs(a).max() <= bound
        assert np.abs(w[name + ".weight"]).max() > 0.9 * bound
        assert abs(w[name + ".weight"].std() - bound / np.sqrt(3)) < 0.1 * bound
    for i in range(1, 7):
        assert np.all(w["encoder.bn%d.weight" % i] == 1) and np.all(w["encoder.bn%d.bias" % i] == 0)
        assert np.all(w["encoder.bn%d.running_mean" % i] == 0) and np.all(w["encoder.bn%d.running_var" % i] == 1)
    assert not np.array_equal(FW.initial_weights(1)["encoder.conv1.weight"], w["encoder.conv1.weight"])


def test_cli_flags_and_the_refusal_of_one_cloud():
    from geometric_adv_amd import train_foldingnet
    from geometric_adv_amd.fold_trainer import FoldingNetTrainer, check_batch
    f = train_foldingnet.build_parser().parse_args([])
    assert (f.batchSize, f.num_points, f.nepoch, f.outf, f.checkpoint_num) == (8, 2048, 25, "log/foldingnet", 0)
    assert f.sampling == "device" and f.top_dir == "."
    f = train_foldingnet.build_parser().parse_args(["--batchSize", "4", "--graph_seed", "9", "--sampling", "reference"])
    assert (f.batchSize, f.graph_seed, f.sampling) == (4, 9, "reference")
    assert "dropped" in train_foldingnet.build_parser().format_help()
    with pytest.raises(ValueError, match="bn6"):
        check_batch(1)
    with pytest.raises(ValueError, match="bn6"):
        FoldingNetTrainer(num_points=64, batch_size=1)
    with pytest.raises(ValueError, match="bn6"):
        train_foldingnet.main(["--batchSize", "1"])


GOLDEN = os.path.join(os.path.dirname(HERE), "tests", "golden", "foldingnet_train.npz")


def test_train_mode_forward_equals_the_references_own_modules():
    import hashlib
    g = np.load(GOLDEN)
    w = FW.synthetic_state(int(g["weight_seed"]))
    h = hashlib.sha256()
    for k in FW.key_names():
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(w[k], np.float32).tobytes())
    assert h.hexdigest() == str(g["sha256"])
    x = g["clouds"]
    cov, rows = F64.graph_from_knn(x, F64.knn(x))
    assert np.array_equal(F64.degrees(rows), g["degree"].astype(np.int64))
    assert np.abs(cov - g["cov"]).max() <= 1e-6 * np.abs(g["cov"]).max()          # ours is rounded to float32
    cols = F64.resolve(rows, g["positions"].astype(np.int64))
    P = {k: M._t(w[k]) for k in M.PARAM_KEYS}
    run = {i: [M._t(w["encoder.bn%d.running_mean" % i]).clone(), M._t(w["encoder.bn%d.running_var" % i]).clone()] for i in range(1, 7)}
    with torch.no_grad():
        loss, mid_loss, ex = M.forward(P, run, x.astype(np.float64), g["cov"], cols)
    assert abs(float(loss) - float(g["loss"])) <= 1e-10 * float(g["loss"])
    assert abs(mid_loss - float(g["mid_loss"])) <= 1e-10 * float(g["mid_loss"])
    n = g["recon"].shape[1]
    for got, want in ((ex["code"], g["code"]), (ex["recon"][:, :n], g["recon"]), (ex["mid"][:, :n], g["mid"])):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    for i in range(1, 7):
        for j, f in enumerate(("running_mean", "running_var")):
            want = g["encoder.bn%d.%s" % (i, f)]
            assert np.abs(run[i][j].numpy() - want).max() <= 1e-10 * np.abs(want).max(), (i, f)
        assert int(g["encoder.bn%d.num_batches_tracked" % i]) == 1


# the input batches of test_gpu_fold_train.py: (weights seed, B, n, batch seed, sampler seed or None = given picks, ordinal,
# every third batch-norm gamma negated)
GPU_BATCHES = [(0, 8, 2048, 1, 5, 0, False), (1, 2, 256, -2, None, 0, False), (2, 3, 1001, 4, 5, 11, False), (0, 32, 2048, 6, 5, 0, False),
               (0, 4, 512, 7, 9, 3, False), (0, 4, 512, 8, 9, 0, False), (0, 4, 512, 13, 5, 0, False), (0, 3, 128, 15, 5, 0, False),
               (0, 4, 512, 31, 5, 0, True), (0, 3, 17, 32, 5, 0, False)]


@pytest.mark.parametrize("wseed,B,n,seed,sampler,ordinal,signed", GPU_BATCHES,
                         ids=["-".join(str(v) for v in c[:6]) + ("-signed" if c[6] else "") for c in GPU_BATCHES])
def test_float32_and_float64_decide_alike_on_the_gpu_tests_batches(wseed, B, n, seed, sampler, ordinal, signed):
    w, x = FW.synthetic_state(wseed), (G._batch(B, n, seed) if seed >= 0 else G._two_shapes(n, -seed))      # seed < 0: the two-shape batch
    if signed:
        w = G.signed_gammas(w)
    cov, rows = F64.graph_from_knn(x, F64.knn(x))
    picks = G._given_picks(x, 3) if sampler is None else F64.device_picks(sampler, np.arange(ordinal, ordinal + B), F64.degrees(rows))
    cols = F64.resolve(rows, picks)
    d64 = M.decisions(w, x, cov, cols)
    d32 = M.decisions(w, x, cov, cols, torch.float32)
    share = {k: float(np.mean(np.asarray(d64[k]) != np.asarray(d32[k]))) for k in d64}
    print(share)
    assert max(share.values()) <= G.PIN_SHARE, share
