"""CPU: the AtlasNet auto-encoder's weights contract (key names, network.pth + options.json loading, refusals), the SQUARE
template, the float64 models against the reference modules' golden, and the ctypes mirrors of geoadv_atlas_* (no GPU)."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import _atlas_model64 as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "atlasnet.npz")


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _cfg(tag):
    nb, nl, dbn = (int(v) for v in _golden()["config_" + tag])
    return nb, nl, bool(dbn)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_key_names_equal_the_reference_modules(tag):
    from geometric_adv_amd import atlas_weights as AW
    nb, nl, dbn = _cfg(tag)
    assert AW.key_names(nb, nl, dbn) == [str(k) for k in _golden()["keys_" + tag]]


def test_remove_all_batchnorms_keeps_the_encoder_bns():
    keys = [str(k) for k in _golden()["keys_b"]]
    assert "module.encoder.bn3.running_mean" in keys and "module.encoder.bn5.weight" in keys
    assert not any(".bn" in k for k in keys if k.startswith("module.decoder."))


@pytest.mark.parametrize("nb", [1, 3, 4, 25])
def test_square_template_equals_the_reference(nb):
    from geometric_adv_amd import atlas_weights as AW
    g = AW.grain(2500, nb)
    want = _golden()["template_%d" % nb]
    assert want.shape == (g * g, 2) and want.dtype == np.float32
    assert np.array_equal(AW.square_template(g), want)
    t = AW.template(nb, g)
    assert t.shape == (nb, g * g, 2) and all(np.array_equal(t[p], want) for p in range(nb))
    if nb == 3:
        assert g == 28                                  # 833 points asked for, 28 x 28 given


@pytest.mark.parametrize("tag", ["a", "b"])
def test_synthetic_weights_are_the_goldens(tag):
    import hashlib
    from geometric_adv_amd import atlas_weights as AW
    nb, nl, dbn = _cfg(tag)
    _, state = AW.synthetic_state(nb, nl, dbn, seed=int(_golden()["seed_" + tag]))
    h = hashlib.sha256()
    for k in AW.key_names(nb, nl, dbn, prefix=""):
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(state[k], np.float32).tobytes())
    assert h.hexdigest() == str(_golden()["sha256_" + tag])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_float64_models_equal_the_reference_modules(tag):
    """Both float64 models (tests/_atlas_model64.py, atlas_weights.forward64) against the reference's modules run in float64
    (golden stored as float32: 2^-24 relative)."""
    from geometric_adv_amd import atlas_weights as AW
    nb, nl, dbn = _cfg(tag)
    _, state = AW.synthetic_state(nb, nl, dbn, seed=int(_golden()["seed_" + tag]))
    g = _golden()
    tmpl = AW.template(nb, AW.grain(2500, nb))
    for z, rec in (M.model(state, g["clouds"], tmpl, nl), AW.forward64(state, g["clouds"], tmpl, nl)):
        assert rec.shape == g["recon_" + tag].shape == (2, 2500, 3)
        assert np.abs(z - g["latent_" + tag]).max() <= 1e-6 * max(1.0, np.abs(z).max())
        assert np.abs(rec - g["recon_" + tag]).max() <= 1e-6 * max(1.0, np.abs(rec).max())


def test_synthetic_model_is_calibrated():
    from geometric_adv_amd import atlas_weights as AW
    _, s = AW.synthetic_state(25, 2, True, seed=11)
    x = AW.calibration_batch()[:2]
    tmpl = AW.template(25, 10)
    z, rec = AW.forward64(s, x, tmpl, 2)
    assert 0.1 < (z > 0).mean() < 0.9
    assert 0.1 < np.abs(rec).mean() < 10


def _write_folder(path, nb=2, nl=1, dbn=True, opt_over=None, drop=(), reshape=None, extra=None):
    from geometric_adv_amd import atlas_weights as AW
    opt, state = AW.synthetic_state(nb, nl, dbn, seed=3, number_points_eval=nb * 16)
    opt.update(opt_over or {})
    AW.save(str(path), opt, state)
    if drop or reshape or extra:
        import torch
        sd = torch.load(str(path / "network.pth"), weights_only=True)
        for k in drop:
            del sd[k]
        for k, shape in (reshape or {}).items():
            sd[k] = torch.zeros(shape)
        sd.update(extra or {})
        torch.save(sd, str(path / "network.pth"))
    return opt, state


def test_loader_reads_network_pth_and_options(tmp_path):
    import torch
    from geometric_adv_amd import atlas_weights as AW
    opt, state = _write_folder(tmp_path, nb=2, nl=1, dbn=True)
    sd = torch.load(str(tmp_path / "network.pth"), weights_only=True)
    assert all(k.startswith("module.") for k in sd) and "module.encoder.bn1.num_batches_tracked" in sd
    got_opt, got = AW.load(str(tmp_path))
    assert got_opt["nb_primitives"] == 2 and got_opt["template_type"] == "SQUARE"
    assert set(got) == set(AW.key_shapes(2, 1, True))
    for k, v in got.items():
        assert np.array_equal(v, state[k])
    c = AW.canonical(got, 2, 1)
    assert c["enc_w"][0].shape == (3, 64) and c["enc_w"][3].shape == (1024, 1024)
    assert c["dec_w"][0].shape == (2, 2, 1024) and c["dec_w"][1].shape == (2, 1024, 512) and c["dec_w"][3].shape == (2, 512, 3)
    assert np.array_equal(c["dec_w"][1][1], state["decoder.decoder.1.conv2.weight"][:, :, 0].T)
    assert c["dec_gamma"][3] is None and c["dec_gamma"][2] is not None


def test_loader_handles_a_model_without_decoder_bn(tmp_path):
    from geometric_adv_amd import atlas_weights as AW
    _write_folder(tmp_path, nb=3, nl=0, dbn=False)
    _, got = AW.load(str(tmp_path))
    assert AW.has_decoder_bn(got) is False and "encoder.bn2.running_var" in got
    c = AW.canonical(got, 3, 0)
    assert all(c[k][i] is None for k in ("dec_gamma", "dec_beta", "dec_mean", "dec_var") for i in range(3))
    assert all(c["enc_gamma"][i] is not None for i in range(5))


def test_loader_reports_every_bad_key_at_once(tmp_path):
    import torch
    from geometric_adv_amd import atlas_weights as AW
    _write_folder(tmp_path, nb=2, nl=1, drop=["module.encoder.lin1.bias", "module.decoder.decoder.1.bn_list.0.running_var"],
                  reshape={"module.decoder.decoder.0.conv2.weight": (512, 1000, 1)},
                  extra={"module.decoder.decoder.2.conv1.weight": torch.zeros(1024, 2, 1)})
    with pytest.raises(KeyError) as e:
        AW.load(str(tmp_path))
    msg = str(e.value)
    for s in ("encoder.lin1.bias", "decoder.decoder.1.bn_list.0.running_var", "decoder.decoder.0.conv2.weight",
              "decoder.decoder.2.conv1.weight", "2 missing", "1 unexpected", "1 of the wrong shape"):
        assert s in msg


@pytest.mark.parametrize("over,match", [
    ({"template_type": "SPHERE"}, "SPHERE.*2500"),
    ({"activation": "tanh"}, "activation"),
    ({"hidden_neurons": 256}, "hidden_neurons"),
    ({"bottleneck_size": 512}, "bottleneck_size"),
    ({"num_layers": 5}, "num_layers"),
    ({"SVR": True}, "SVR"),
    ({"nb_primitives": 129}, "nb_primitives"),
])
def test_refusals(tmp_path, over, match):
    from geometric_adv_amd import atlas_weights as AW
    _write_folder(tmp_path)
    with open(tmp_path / "options.json") as f:
        opt = json.load(f)
    opt.update(over)
    with open(tmp_path / "options.json", "w") as f:
        json.dump(opt, f)
    with pytest.raises(ValueError, match=match):
        AW.load(str(tmp_path))


def test_reference_default_template_is_refused():
    from geometric_adv_amd import atlas_weights as AW
    with pytest.raises(ValueError, match="SPHERE"):
        AW.check_options(AW.options())          # parser_transfer's default template_type is SPHERE


def test_run_transfer_refuses_foldingnet():
    from geometric_adv_amd import run_transfer
    with pytest.raises(SystemExit, match="np.random.choice"):
        run_transfer.main(["--transfer_ae_type", "FoldingNet"])
    with pytest.raises(AssertionError):
        run_transfer.main(["--transfer_ae_type", "Other"])


def test_library_exports_the_atlas_entry_points():
    from geometric_adv_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("geoadv_atlas_create", "geoadv_atlas_destroy", "geoadv_atlas_workspace_bytes", "geoadv_atlas_forward"):
        assert hasattr(lib, name), name


def test_python_mirrors_match_the_header():
    from test_classifier_host import _header_struct
    from geometric_adv_amd.atlasnet import _AtlasConfig, _AtlasWeights
    assert [(f, "int", 1) for f, _ in _AtlasConfig._fields_] == _header_struct("geoadv_atlas_config")
    got = [(f, "ptr", t._length_) for f, t in _AtlasWeights._fields_]
    assert all(t._type_ is ctypes.c_void_p for _, t in _AtlasWeights._fields_)
    assert got == _header_struct("geoadv_atlas_weights")
    assert ctypes.sizeof(_AtlasConfig) == 8 * 4 and ctypes.sizeof(_AtlasWeights) == (6 * 5 + 6 * 7) * ctypes.sizeof(ctypes.c_void_p)
