"""What the golden training steps (test_gpu_train_step_bits.py) do not reach in the three layer-by-layer trainers: _flatten,
set_slots, the layout export and the restore path.  Each trainer, at its smallest golden shape, takes one train_step; a second
trainer is built from the first one's exported weights, slots and counters, and its flat parameter buffer, both optimizer
slots and running (moving) statistics must be the first's bit for bit -- they are copies, so there is no tolerance.  And
_flatten(_unflatten(flat)) must give back every word that geoadv_*_trainer_layout names (zeros elsewhere).

The weights are the initial ones with a seeded offset on every vector (biases, gamma, beta, running statistics): the initial
gamma = 1, beta = 0, mean = 0, var = 1 could be exchanged between layers without a trace."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ABSENT = (1 << 64) - 1          # (size_t)-1: what the layout export writes for an entry a layer does not have


def _clouds(seed, b, n):
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)


def _distinct(state, seed):
    rng = np.random.default_rng(seed)
    return {k: np.asarray(v, np.float32) + rng.uniform(0.05, 0.25, np.shape(v)).astype(np.float32) if np.ndim(v) == 1 else v
            for k, v in state.items()}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _flat(tr, ptr):
    import torch
    from geometric_adv_amd import _lib
    torch.cuda.synchronize(tr.device)
    return _lib.device_view(ptr, tr._count, "<f4", tr.device).cpu().numpy().copy()


def _named_mask(tr, layers, max_layers):
    """True at every word of the flat layout that geoadv_*_trainer_layout names.  layers: (groups, fan_in, fan_out, has a
    batch norm) per layer, from the Python side's tables; the offsets are the handle's."""
    offs, moving = tr._offsets, tr._moving_offsets
    assert len(offs) == 4 * max_layers and len(moving) == max_layers
    mask = np.zeros(tr._count, bool)
    for l, (g, fi, fo, bn) in enumerate(layers):
        o = offs[4 * l: 4 * l + 4]
        spans = [(o[0], g * fi * fo), (o[1], g * fo)] + ([(o[2], g * fo), (o[3], g * fo)] if bn else [])
        assert (o[2] != ABSENT) == (o[3] != ABSENT) == (moving[l] != ABSENT) == bool(bn), (l, o, moving[l])
        for start, count in spans:
            assert start % 16 == 0 and start + count <= tr._count and not mask[start:start + count].any(), (l, start, count)
            mask[start:start + count] = True
    assert all(v == ABSENT for v in offs[4 * len(layers):] + moving[len(layers):])
    return mask


def _check_round_trip(tr, mask, flats):
    assert mask.any()
    for name, flat in flats.items():
        back = tr._flatten(tr._unflatten(flat))
        assert back.dtype == np.float32 and back.shape == flat.shape, name
        assert (_bits(back)[mask] == _bits(flat)[mask]).all(), "%s: _flatten(_unflatten(flat)) differs at a named offset" % name
        assert not _bits(back)[~mask].any(), "%s: _flatten wrote outside the named offsets" % name


def _check_same(one, two, bn_layers, mean, var):
    assert two.counters() == one.counters()
    for name in ("parameters", "slot1", "slot2"):               # the whole flat buffers, padding words included
        a, b = (_flat(t, t._params_ptr) if name == "parameters" else t.state(name) for t in (one, two))
        assert a.shape == b.shape == (one._count,)
        same = _bits(a) == _bits(b)
        assert same.all(), "%s: %d words differ, first at %d" % (name, same.size - int(same.sum()), int(np.argmin(same)))
    assert bn_layers
    for l in bn_layers:
        for what in (mean, var):
            assert np.array_equal(_bits(one.state(what, l)), _bits(two.state(what, l))), (what, l)


def test_foldingnet_restore_and_round_trip():
    from geometric_adv_amd import fold_weights as FW
    from geometric_adv_amd.fold_trainer import LAYERS, FoldingNetTrainer
    B, n = 2, 17
    one = FoldingNetTrainer(weights=_distinct(FW.initial_weights(0), 1), num_points=n, batch_size=B, seed=11)
    loss, mid = one.train_step(_clouds(5, B, n))
    assert np.isfinite([loss, mid]).all()
    step, ordinal = one.counters()
    assert (step, ordinal) == (1, B)
    two = FoldingNetTrainer(weights=one.export_state_dict(), num_points=n, batch_size=B, seed=11, step=step, slots=one.slots(),
                            ordinal=ordinal)
    _check_same(one, two, range(6), "running_mean", "running_var")
    mask = _named_mask(one, [(1, fi, fo, bn) for pre, fi, fo, conv, bn in LAYERS], len(LAYERS))
    _check_round_trip(one, mask, {"params": _flat(one, one._params_ptr), "grads": _flat(one, one._grads_ptr),
                                  "slot1": one.state("slot1"), "slot2": one.state("slot2")})


@pytest.mark.parametrize("decoder_bn", [True, False])
def test_atlasnet_restore_and_round_trip(decoder_bn):
    from geometric_adv_amd import atlas_weights as AW
    from geometric_adv_amd.atlas_trainer import MAX_TRAIN_LAYERS, AtlasNetTrainer
    B, n, nb, p, nl = 3, 33, 2, 7, 1
    opt, state = AW.initial_weights(0, nb, nl, decoder_bn, p * nb)
    opt["number_points"] = nb * p
    one = AtlasNetTrainer(weights=_distinct(state, 2), options=opt, num_points=n, batch_size=B, seed=13)
    assert one.decoder_bn == decoder_bn and one.points_per_primitive == p
    assert np.isfinite(one.train_step(_clouds(6, B, n)))
    step, tracked = one.counters()
    assert (step, tracked) == (1, 1)
    two = AtlasNetTrainer(weights=one.export_state_dict(), options=one.options, num_points=n, batch_size=B, seed=13, step=step,
                          slots=one.slots(), tracked=tracked)
    bn_layers = [l for l, layer in enumerate(one.layers) if layer[4]]
    assert len(bn_layers) == (5 + 2 + nl if decoder_bn else 5)
    _check_same(one, two, bn_layers, "running_mean", "running_var")
    mask = _named_mask(one, [(nb if dec else 1, fi, fo, bn) for pre, fi, fo, conv, bn, dec in one.layers], MAX_TRAIN_LAYERS)
    _check_round_trip(one, mask, {"params": _flat(one, one._params_ptr), "grads": _flat(one, one._grads_ptr),
                                  "slot1": one.state("slot1"), "slot2": one.state("slot2")})


@pytest.mark.parametrize("optimizer", ["adam", "momentum"])
def test_classifier_restore_and_round_trip(optimizer):
    from geometric_adv_amd import _abi, cls_weights as CW
    from geometric_adv_amd.cls_trainer import PointNetClassifierTrainer
    B, n, nc = 3, 70, 5
    one = PointNetClassifierTrainer(weights=_distinct(CW.initial_weights(nc, 0), 3), num_points=n, batch_size=B, num_classes=nc,
                                    optimizer=optimizer, seed=17)
    loss, _ = one.train_step(_clouds(7, B, n), np.array([4, 0, 2]))
    assert np.isfinite(loss)
    saved = one.export_weights(slots=True)
    assert int(saved[CW.STEP_NAME]) == one.counters()[0] == 1
    two = PointNetClassifierTrainer(weights=saved, num_points=n, batch_size=B, num_classes=nc, optimizer=optimizer, seed=17,
                                    step=int(saved[CW.STEP_NAME]), slots=saved)
    bn_layers = [l for l, layer in enumerate(one._shapes()) if layer[3]]
    assert len(bn_layers) == 17
    _check_same(one, two, bn_layers, "moving_mean", "moving_var")
    assert np.array_equal(_bits(one.parameters()), _bits(_flat(one, one._params_ptr)))        # parameters(): the flat buffer
    mask = _named_mask(one, [(1, fi, fo, bn) for scope, fi, fo, bn, shape in one._shapes()], _abi.GEOADV_CLS_LAYERS)
    _check_round_trip(one, mask, {"params": one.parameters(), "grads": _flat(one, one._grads_ptr), "slot1": one.state("slot1"),
                                  "slot2": one.state("slot2")})
