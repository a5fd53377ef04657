"""GPU: the f16x2 split the encoder kernels use (h2_split_pair: v_cvt_pk_f16_f32, then one v_fma_mix per value) gives, word for
word, what its reference form (convert, subtract in fp32, convert) gives on the same card and what the numpy model gives
(h2_split_cases.model), through the test entry geoadv_debug_h2_split -- on the 4.1 M inputs of the host test plus the zeros, the
fp16 subnormal range, 65504, the first fp32 values that round to the fp16 infinity and +inf.  Every non-NaN input is compared;
NaN inputs need only give NaN pieces."""
import ctypes

import numpy as np
import pytest

import h2_split_cases as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def run():
    import torch
    from geometric_adv_amd import _lib
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    nans = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7fffffff], np.uint32).view(np.float32)
    a = np.concatenate([H.inputs(), H.edge_inputs(), nans])
    if a.size % 2:
        a = np.concatenate([a, np.zeros(1, np.float32)])
    # a second copy with the halves of every pair swapped: each value is split in the low AND the high half of a word
    a = np.concatenate([a, a.reshape(-1, 2)[:, ::-1].reshape(-1)])
    n = a.size // 2
    with torch.cuda.device(dev):
        src = torch.from_numpy(a).to(dev)
        out = torch.zeros((3, n), dtype=torch.int32, device=dev)
        fn = _lib.lib().geoadv_debug_h2_split
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib.check(fn(_lib.ptr(src), n, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_handle()), "debug_h2_split")
        torch.cuda.synchronize()
        w = out.cpu().numpy().view(np.uint32)
    # little-endian halves: element k of the uint16 view belongs to input k
    return a, w[0].view(np.uint16), w[1].view(np.uint16), w[2].view(np.uint16)


def _is_nan16(h):
    return (h & 0x7fff) > 0x7c00


def test_every_input_is_there(run):
    a = run[0]
    for v in (0.0, 65504.0, 65520.0, np.inf, 2.0 ** -24, 2.0 ** -14):
        assert (a == np.float32(v)).any()
    assert (np.signbit(a) & (a == 0)).any() and np.isnan(a).sum() == 8


def test_mix_form_equals_reference_form_and_model_word_for_word(run):
    a, w0, w1, w1_ref = run
    ok = ~np.isnan(a)
    hi, lo = H.model(a)
    assert not _is_nan16(hi[ok]).any() and (_is_nan16(lo) & ok == np.isposinf(a)).all()
    # (the one NaN piece of a non-NaN input is +inf's inf - inf, whose sign IEEE 754 leaves open -- x86 and this GPU give 0xfe00,
    # other hosts 0x7e00: against the MODEL a NaN piece must be a NaN piece; between the two device forms every word is compared)
    for name, got, want in (("w0 vs model", w0, hi), ("w1 vs w1_ref", w1, w1_ref), ("w1 vs model", w1, lo), ("w1_ref vs model", w1_ref, lo)):
        bad = ok & (got != want)
        if "model" in name:
            bad &= ~(_is_nan16(got) & _is_nan16(want))
        assert not bad.any(), "%s: %d of %d differ, first input %r (bits 0x%08x): 0x%04x against 0x%04x" % (
            name, int(bad.sum()), int(ok.sum()), a[bad][0], int(a[bad][:1].view(np.uint32)[0]), int(got[bad][0]), int(want[bad][0]))


def test_nan_inputs_give_nan_pieces(run):
    a, w0, w1, w1_ref = run
    nan = np.isnan(a)
    assert _is_nan16(w0[nan]).all() and _is_nan16(w1[nan]).all() and _is_nan16(w1_ref[nan]).all()
