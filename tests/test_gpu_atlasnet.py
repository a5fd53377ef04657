"""GPU: the AtlasNet auto-encoder (csrc/atlasnet.hip through geoadv_atlas_* and atlasnet.AtlasNetAE) against the reference
modules' golden and the float64 model of tests/_atlas_model64.py, its invariances, isolation, refusals, streams, the Chamfer
loss and the run_transfer CLI."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import _atlas_model64 as M

pytestmark = pytest.mark.gpu

# TOLERANCE, on max |got - ref| / max(1, max |ref|).  Every layer is an fp32 dot product -- MFMA fp32 accumulation or an
# fmaf chain -- whose rounding is about sqrt(K) * 2^-24 of the magnitudes summed: 32 * 6e-8 = 2e-6 for K = 1024.  A
# coordinate sits at the end of up to eleven of them (conv1..conv3, lin1, lin2, decoder conv1, conv2 with K = 1024, up to
# four 512-wide hidden layers, last_conv), and every batch norm of the calibrated synthetic model divides by its layer's
# standard deviation, which sits well below the summed magnitudes where terms cancel -- most of all lin1 / lin2, whose
# statistics are taken across clouds that differ little.  Measured on the MI355X: latents within 1.1e-5 of float64,
# reconstructions within 1.0e-5 ... 3.5e-5 with decoder batch norm and up to 5.3e-5 without it at num_layers 4 (its
# bias-centred layers amplify more), about what the classifier's 17-layer chain reaches (7.5e-5).  The bound is therefore
# the 1e-4 ceiling; every "told apart" mistake below moves the output by more than 0.6, i.e. 6000 x TOL.
TOL = 1e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atlasnet.npz")


def _clouds(seed, b, n):
    return (np.random.default_rng(seed).random((b, n, 3)) - 0.5).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model(nb, nl, dbn, seed=0):
    from geometric_adv_amd import atlas_weights as AW
    g = AW.grain(2500, nb)
    opt, state = AW.synthetic_state(nb, nl, dbn, seed=seed)
    return opt, state, AW.template(nb, g)


@functools.lru_cache(maxsize=None)
def _ae(nb, nl, dbn, seed=0):
    from geometric_adv_amd.atlasnet import AtlasNetAE
    opt, state, _ = _model(nb, nl, dbn, seed)
    return AtlasNetAE(options=opt, state=state)


@functools.lru_cache(maxsize=None)
def _ref(nb, nl, dbn, n):
    _, state, tmpl = _model(nb, nl, dbn)
    x = _clouds(100 + n, 32, n)
    return (x,) + M.model(state, x, tmpl, nl)


def _err(got, ref):
    return np.abs(np.asarray(got, np.float64) - ref).max() / max(1.0, np.abs(ref).max())


def _run(ae, x):
    z, r = ae.forward(x)
    return z.cpu().numpy(), r.cpu().numpy()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_against_the_reference_modules(tag):
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlasnet import AtlasNetAE
    with np.load(GOLDEN) as g:
        nb, nl, dbn = (int(v) for v in g["config_" + tag])
        opt, state = AW.synthetic_state(nb, nl, bool(dbn), seed=int(g["seed_" + tag]))
        z, r = _run(AtlasNetAE(options=opt, state=state), g["clouds"])
        ez, er = _err(z, g["latent_" + tag]), _err(r, g["recon_" + tag])
        print("golden %s: latent %.2e recon %.2e" % (tag, ez, er))
        assert r.shape == g["recon_" + tag].shape
        assert ez <= TOL and er <= TOL


@pytest.mark.parametrize("dbn", [True, False])
@pytest.mark.parametrize("nl", [0, 2, 4])
@pytest.mark.parametrize("nb", [1, 25])
@pytest.mark.parametrize("b,n", [(1, 2048), (3, 1000), (32, 2048)])
def test_against_float64(b, n, nb, nl, dbn):
    x, z64, r64 = _ref(nb, nl, dbn, n)
    z, r = _run(_ae(nb, nl, dbn), x[:b])
    ez, er = _err(z, z64[:b]), _err(r, r64[:b])
    print("b %d n %d nb %d nl %d bn %d: latent %.2e recon %.2e" % (b, n, nb, nl, dbn, ez, er))
    assert r.shape == (b, 2500, 3) and z.shape == (b, 1024)
    assert ez <= TOL and er <= TOL


def test_negative_pooled_channels_are_exact():
    """conv3's BN output is negative for every point in 100 channels: the signed max must pick the largest negative value
    (an integer max on the raw float bits, with +0 as identity, would return 0 there)."""
    from geometric_adv_amd.atlasnet import AtlasNetAE
    opt, state, tmpl = _model(1, 2, True)
    state = dict(state)
    beta = state["encoder.bn3.bias"].copy()
    beta[:100] = -12.0
    state["encoder.bn3.bias"] = beta
    x = _clouds(7, 4, 2048)
    # the pooled values of those channels are negative (float64, straight from the layers)
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        s = {k: torch.as_tensor(v, dtype=torch.float64) for k, v in state.items()}
        h = torch.as_tensor(x, dtype=torch.float64).transpose(1, 2)
        for i, c in enumerate(("conv1", "conv2", "conv3")):
            h = F.batch_norm(F.conv1d(h, s["encoder.%s.weight" % c], s["encoder.%s.bias" % c]),
                             s["encoder.bn%d.running_mean" % (i + 1)], s["encoder.bn%d.running_var" % (i + 1)],
                             s["encoder.bn%d.weight" % (i + 1)], s["encoder.bn%d.bias" % (i + 1)], False, 0, 1e-5)
            if i < 2:
                h = F.relu(h)
        pooled = h.max(2)[0].numpy()
    assert (pooled[:, :100] < -1).all()
    z64, r64 = M.model(state, x, tmpl, 2)
    z, r = _run(AtlasNetAE(options=opt, state=state), x)
    assert _err(z, z64) <= TOL and _err(r, r64) <= TOL


def test_mistakes_are_told_apart():
    """Each of these mistakes moves the output by more than 100 x TOL: the comparisons above would catch it."""
    x = _clouds(9, 2, 2048)
    _, state, tmpl = _model(25, 2, True)
    z, r = _run(_ae(25, 2, True), x)
    _, want = M.model(state, x, tmpl, 2)
    assert _err(r, want) <= TOL
    for kw in ({"swap_template_axes": True}, {"reverse_primitives": True}):
        _, wrong = M.model(state, x, tmpl, 2, **kw)
        assert _err(wrong, want) > 100 * TOL, kw
    # a remove_all_batchNorms model: only the decoder lost its batch norms; dropping the encoder's as well is a mistake
    opt, state, tmpl = _model(1, 0, False)
    z, r = _run(_ae(1, 0, False), x)
    zw, want = M.model(state, x, tmpl, 0)
    zb, wrong = M.model(state, x, tmpl, 0, drop_encoder_bn=True)
    assert _err(r, want) <= TOL and _err(z, zw) <= TOL
    assert _err(wrong, want) > 100 * TOL and _err(zb, zw) > 100 * TOL


def test_bit_exact_invariances():
    ae = _ae(25, 2, True)
    x = _clouds(21, 32, 2048)
    z, r = _run(ae, x)
    perm = np.random.default_rng(3).permutation(2048)
    zp, rp = _run(ae, x[:, perm])
    assert np.array_equal(z, zp) and np.array_equal(r, rp)
    for k in (0, 13, 31):
        z1, r1 = _run(ae, x[k:k + 1])
        assert np.array_equal(z1[0], z[k]) and np.array_equal(r1[0], r[k])


def test_non_default_stream_same_bits():
    """The delayed-call protocol of tests/_stream_order.py: behind a pending delay on a side stream, over scratch that holds
    another batch's values, the forward gives the default stream's bits and does not block the host."""
    import torch
    import _stream_order as SO
    ae = _ae(25, 2, True)
    a, b = (torch.from_numpy(_clouds(s, 10, 1500)).to("cuda:0") for s in (30, 31))
    SO.check_call("atlasnet.forward", ae.forward, [a], [b], keep=ae)


def test_nonfinite_cloud_is_isolated():
    ae = _ae(25, 2, True)
    x = _clouds(41, 5, 700)
    z, r = _run(ae, x)
    for bad in (np.nan, np.inf):
        y = x.copy()
        y[2, 17, 1] = bad
        zb, rb = _run(ae, y)
        keep = [0, 1, 3, 4]
        assert np.array_equal(zb[keep], z[keep]) and np.array_equal(rb[keep], r[keep])


def test_refusals():
    import torch
    from geometric_adv_amd import _lib
    from geometric_adv_amd.atlasnet import _AtlasConfig, _AtlasWeights
    ae = _ae(1, 0, False)
    lib = _lib.lib()
    good = dict(nb_primitives=1, points_per_primitive=2500, dim_template=2, bottleneck_size=1024, hidden_neurons=512,
                num_layers=0, activation=0, decoder_bn=0)
    bad = [("nb_primitives", 0), ("nb_primitives", 129), ("dim_template", 4), ("bottleneck_size", 512),
           ("hidden_neurons", 256), ("num_layers", 5), ("activation", 1), ("decoder_bn", 2), ("points_per_primitive", 0)]
    hw = _AtlasWeights()
    for key, arrays in ae._canon.items():
        for i, a in enumerate(arrays):
            getattr(hw, key)[i] = a.ctypes.data if a is not None else None
    tmpl = np.zeros((1, 2500, 2), np.float32)
    for f, v in bad:
        cfg = _AtlasConfig(**dict(good, **{f: v}))
        h = ctypes.c_void_p()
        assert lib.geoadv_atlas_create(ctypes.byref(h), ctypes.byref(cfg), ctypes.byref(hw),
                                       tmpl.ctypes.data_as(ctypes.c_void_p)) == 1, f
    # BN pointers given although decoder_bn = 0
    hw.dec_gamma[0] = hw.enc_gamma[0]
    h = ctypes.c_void_p()
    assert lib.geoadv_atlas_create(ctypes.byref(h), ctypes.byref(_AtlasConfig(**good)), ctypes.byref(hw),
                                   tmpl.ctypes.data_as(ctypes.c_void_p)) == 1
    ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda:0")
    x = torch.zeros((1, 16385, 3), device="cuda:0")
    rec = torch.empty((1, ae.num_points, 3), device="cuda:0")
    for b, n in ((1, 0), (1, 16385), (0, 16), (-1, 16)):
        assert lib.geoadv_atlas_forward(ae.handle, b, n, _lib.ptr(x), None, _lib.ptr(rec), _lib.ptr(ws), None) == 1
    with pytest.raises(ValueError):
        ae.forward(torch.zeros((1, 16, 2), device="cuda:0"))


def test_loss_per_pc_equals_the_oracle_chamfer():
    from oracle.cpu_oracle import Oracle
    ae = _ae(25, 2, True)
    recon = ae.get_reconstructions(_clouds(51, 5, 2048))
    target = _clouds(52, 5, 2048)
    got = ae.get_loss_per_pc(recon, target)
    d1, _, d2, _ = Oracle().nn_distance(recon, target)
    want = d1.astype(np.float64).mean(1) + d2.astype(np.float64).mean(1)
    assert got.shape == (5,) and np.allclose(got, want, rtol=1e-5, atol=0)
    # any number of clouds, chunked by batch_size: the same bits as one forward
    assert np.array_equal(recon, _run(ae, _clouds(51, 5, 2048))[1])


# ------------------------------------------------------------------------------------------------ run_transfer
def _eval_folder(root, n):
    """A victim eval folder whose point clouds, reconstructions and AE losses come from the victim PointNetAE itself, plus an
    attack folder whose adversarial outputs are consistent with it (what run_attack would have written)."""
    from geometric_adv_amd import weights as W
    from geometric_adv_amd.attack_data import prepare_data_for_attack
    from geometric_adv_amd.autoencoder import PointNetAE
    classes, sizes = ["chair", "table", "car"], [4, 5, 4]
    ae_dir = root / "log" / "ae"
    ev = ae_dir / "eval"
    os.makedirs(ev)
    w = W.synthetic_weights(n)
    W.save_npz(str(ae_dir / "weights.npz"), w)
    victim = PointNetAE(w, n)
    slice_idx = np.concatenate([[0], np.cumsum(sizes)])
    pcs = _clouds(61, int(slice_idx[-1]), n)
    rec = victim.get_reconstructions(pcs)
    loss = victim.get_loss_per_pc(pcs)
    rng = np.random.default_rng(0)
    nn_idx = np.zeros((len(pcs), len(pcs)), np.int16)
    for s in range(len(pcs)):
        for t in range(len(sizes)):
            nn_idx[s, slice_idx[t]:slice_idx[t + 1]] = rng.permutation(sizes[t])
    attack_idx = np.stack([rng.permutation(4)[:2] for _ in sizes])
    np.save(ev / "point_clouds_test_set_3l.npy", pcs); np.save(ev / "reconstructions_test_set_3l.npy", rec)
    np.save(ev / "ae_loss_test_set_3l.npy", loss)
    np.save(ev / "pc_classes_3l.npy", np.array(classes)); np.save(ev / "slice_idx_test_set_3l.npy", slice_idx)
    np.save(ev / "chamfer_nn_idx_complete_test_set_3l.npy", nn_idx)
    np.save(ev / "sel_idx.npy", attack_idx)
    att = ev / "attack_res"
    os.makedirs(att)
    with open(att / "attack_configuration.json", "w") as f:
        json.dump({"class_names": ["chair", "car"], "target_pc_idx_type": "chamfer_nn_complete", "num_pc_for_attack": 2,
                   "num_pc_for_target": 1, "correct_pred_only": 0, "dist_weight_list": [0.5, 2.0], "restore_epoch": 500}, f)
    adv = {}
    for k, name in enumerate(("chair", "car")):
        os.makedirs(att / name / "analysis_results")
        prep = lambda d: prepare_data_for_attack(np.array(classes), [name], ["chair", "car"], d, slice_idx, attack_idx, 1,
                                                 nn_idx, None)
        _, tgt = prep(pcs)
        _, tloss = prep(loss)
        m = len(tgt)
        pc_in = _clouds(70 + k, 2 * m, n).reshape(2, m, n, 3)
        pc_rec = np.stack([victim.get_reconstructions(pc_in[j]) for j in range(2)])
        metrics = np.zeros((2, m, 7), np.float32)
        for j in range(2):
            err = victim.get_loss_per_pc(pc_in[j], tgt)
            metrics[j, :, 4] = err
            metrics[j, :, 3] = err / tloss.reshape(-1)
            metrics[j, :, 0] = rng.random(m)
        np.save(att / name / "adversarial_pc_input.npy", pc_in)
        np.save(att / name / "adversarial_pc_recon.npy", pc_rec)
        np.save(att / name / "adversarial_metrics.npy", metrics)
        sel = np.arange(m) % 2
        np.save(att / name / "analysis_results" / "source_target_norm_min_idx.npy", sel)
        adv[name] = (pc_in[sel, np.arange(m)], metrics[sel, np.arange(m)], tgt, tloss.reshape(-1))
    return adv


def _check_outputs(folder, adv, ae, P):
    for name, (pc_in, metrics, tgt, tloss) in adv.items():
        rec = np.load(folder / name / "transferred_pc_recon.npy")
        tm = np.load(folder / name / "transfer_metrics.npy")
        m = len(pc_in)
        assert rec.shape == (1, m, P, 3) and tm.shape == (1, m, 4)
        assert np.array_equal(tm[0, :, 2], metrics[:, 4]) and np.array_equal(tm[0, :, 3], metrics[:, 3])
        assert np.array_equal(tm[0, :, 1], tm[0, :, 0] / tloss)
        assert np.array_equal(rec[0], ae.get_reconstructions(pc_in))


def test_run_transfer_end_to_end(tmp_path):
    from geometric_adv_amd import atlas_weights as AW, run_transfer, weights as W
    from geometric_adv_amd.atlasnet import AtlasNetAE
    from geometric_adv_amd.autoencoder import PointNetAE
    n = 256
    adv = _eval_folder(tmp_path, n)
    base = ["--top_dir", str(tmp_path), "--ae_folder", "log/ae", "--attack_pc_idx", "log/ae/eval/sel_idx.npy"]
    # AtlasNet: 4 primitives x 10 x 10 = 400 points (the reference's buffer would only take 2500)
    opt, state = AW.synthetic_state(4, 1, True, seed=5, number_points_eval=400)
    AW.save(str(tmp_path / "log" / "atlas"), opt, state)
    run_transfer.main(base + ["--transfer_ae_type", "AtlasNet", "--transfer_ae_folder", "log/atlas"])
    out = tmp_path / "log" / "atlas" / "eval" / "attack_res_transfer"
    ae = AtlasNetAE(str(tmp_path / "log" / "atlas"))
    _check_outputs(out, adv, ae, 400)
    for name, (_, _, tgt, _) in adv.items():
        tm = np.load(out / name / "transfer_metrics.npy")
        rec = np.load(out / name / "transferred_pc_recon.npy")
        assert np.array_equal(tm[0, :, 0], ae.get_loss_per_pc(rec[0], tgt))
    assert os.path.exists(out / "transfer_configuration.json")
    # PointNet with other weights
    os.makedirs(tmp_path / "log" / "ae2")
    w2 = W.randomized_weights(n, seed=9)
    W.save_npz(str(tmp_path / "log" / "ae2" / "weights.npz"), w2)
    run_transfer.main(base + ["--transfer_ae_type", "PointNet", "--transfer_ae_folder", "log/ae2"])
    _check_outputs(tmp_path / "log" / "ae2" / "eval" / "attack_res_transfer", adv, PointNetAE(w2, n), n)
    # PointNet with the victim's own folder: the sanity checks pass and nothing is written (run_transfer.py:220-222)
    run_transfer.main(base + ["--transfer_ae_type", "PointNet", "--transfer_ae_folder", "log/ae", "--do_sanity_checks", "1"])
    own = tmp_path / "log" / "ae" / "eval" / "attack_res_transfer"
    for name in adv:
        assert os.path.isdir(own / name) and not os.listdir(own / name)
