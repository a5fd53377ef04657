"""CPU: the kNN outlier term of the auto-encoder attack on the host side -- Configuration carries knn_weight / knn_k / knn_alpha
with their defaults, refuses what geoadv_attack_create refuses (include/geoadv.h at geoadv_attack_config) before any device is
touched, refuses none of it while the term is off, and run_attack has the three flags."""
import ctypes

import pytest

N = 256


def _conf(**kw):
    from geometric_adv_amd.adv_ae import Configuration
    args = dict(batch_size=4, n_points=N, weights=None)
    args.update(kw)
    return Configuration(**args)


def test_configuration_carries_the_three_values_and_their_defaults():
    c = _conf()
    assert (c.knn_weight, c.knn_k, c.knn_alpha) == (0.0, 5, 1.05)
    assert isinstance(c.knn_weight, float) and isinstance(c.knn_k, int) and isinstance(c.knn_alpha, float)
    c = _conf(knn_weight=3, knn_k=7, knn_alpha=2)
    assert (c.knn_weight, c.knn_k, c.knn_alpha) == (3.0, 7, 2.0)
    c = _conf(knn_weight=-2.5, batch_slots=2)            # a negative weight is a weight; batch_slots is untouched by the term
    assert c.knn_weight == -2.5 and c.batch_slots == 2


REFUSED = {
    "n = knn_k + 1": dict(n_points=6, knn_k=5),
    "n = 16385": dict(n_points=16385),
    "knn_k = 0": dict(knn_k=0),
    "knn_k = 16": dict(knn_k=16),
    "knn_alpha = -1": dict(knn_alpha=-1.0),
    "knn_alpha = nan": dict(knn_alpha=float("nan")),
    "knn_alpha = inf": dict(knn_alpha=float("inf")),
    "knn_weight = nan": dict(knn_weight=float("nan")),
    "knn_weight = inf": dict(knn_weight=float("inf")),
    "loss_dist_type = pert": dict(loss_dist_type="pert"),
    "batch = 65536": dict(batch_size=65536),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_configuration_refuses(name):
    kw = dict(knn_weight=3.0)
    kw.update(REFUSED[name])
    with pytest.raises(ValueError):
        _conf(**kw)


@pytest.mark.parametrize("name", [k for k in REFUSED if "knn_weight" not in k])
def test_nothing_is_refused_while_the_term_is_off(name):
    c = _conf(knn_weight=0.0, **REFUSED[name])
    assert c.knn_weight == 0.0


def test_the_smallest_and_largest_accepted_shapes():
    assert _conf(knn_weight=1.0, knn_k=5, n_points=7).knn_k == 5
    assert _conf(knn_weight=1.0, knn_k=15, n_points=17).knn_k == 15
    assert _conf(knn_weight=1.0, n_points=16384, batch_size=65535, knn_alpha=0.0).knn_alpha == 0.0


def test_pert_refusal_says_why():
    with pytest.raises(ValueError, match="pert"):
        _conf(knn_weight=1.0, loss_dist_type="pert")


def test_run_attack_has_the_three_flags():
    from geometric_adv_amd import run_attack
    p = run_attack.build_parser()
    d = p.parse_args([])
    assert (d.knn_weight, d.knn_k, d.knn_alpha) == (0.0, 5, 1.05)
    f = p.parse_args(["--knn_weight", "5", "--knn_k", "7", "--knn_alpha", "1.5"])
    assert (f.knn_weight, f.knn_k, f.knn_alpha) == (5.0, 7, 1.5)
    assert isinstance(f.knn_k, int)


def test_the_mirror_has_the_three_members_before_loss_in_scan():
    """loss_in_scan stays the struct's last member (tests/test_abi.py holds it there); the three members stand before it, all
    int / float, and a zeroed structure has the term off."""
    from geometric_adv_amd import _abi
    assert _abi.AttackConfig._fields_[-4:] == [("knn_weight", ctypes.c_float), ("knn_k", ctypes.c_int), ("knn_alpha", ctypes.c_float),
                                               ("loss_in_scan", ctypes.c_int)]
    c = _abi.AttackConfig()
    assert (c.knn_weight, c.knn_k, c.knn_alpha) == (0.0, 0, 0.0)


def test_an_alpha_beyond_float32_is_refused():
    with pytest.raises(ValueError):
        _conf(knn_weight=1.0, knn_alpha=1e39)
