"""GPU: the two fp32 MFMA GEMM kernels of the training steps on their own (geoadv_train_gemm, ops.train_gemm), through the
launches the trainers use: kernel 0 = ct_gemm_kernel + ct_splitk_reduce (csrc/train_tile.h, 64 x 64 tiles, K chunks of 32, a
split of the K range chosen from the shape), kernel 1 = at_gemm_kernel (csrc/atlas_train.hip, 128 x 128 tiles, K slices of 16,
double-buffered, batched, a bias per group).  Reference: C64 = A64 @ B64 (+ bias) in numpy float64 on the fp32 inputs.

THE BOUND, per element, derived and not measured:  |C - C64| <= (K + 4) * 2^-24 * (|A| @ |B| + |bias|).
With u = 2^-24 (fp32, round to nearest): every product a b is rounded at most once (u) and the K products of an element are
added by K fp32 additions in some order (the MFMA's two-wide steps, the K slices, the accumulator that starts at 0), each of
which rounds its partial sum once: the standard inner-product bound gives |sum - exact| <= ((1 + u)^K - 1) * sum |a| |b| =
(K u + O(K^2 u^2)) * (|A| @ |B|) whatever the order.  The bias is added in fp32: one more rounding of (sum + bias), at most
u * (|A| @ |B| + |bias|) to first order.  With a split K range each partial sum has the bound of its own part of K (together
K u), the partials are added in double (2^-53: nothing) and the double is rounded to fp32 once: one more u.  That is
(K + 2) u; the remaining 2 u cover every second-order term: K^2 u^2 <= 1.2e-9 << 2 u = 1.2e-7 for K <= 1024, the largest K
here.  The multiplication by alpha = 1 is exact.  The largest error / bound of every launch is printed (-s).

EVERY SHAPE CAN FAIL: before the launch the test forms on the CPU two wrong results -- C64 with the last k index dropped (a
K tail that is not read) and C64 with the rows of A shifted by one (row i takes row i - 1, row 0 zeros: a row index off by
one) -- and requires the largest change of either to exceed 100 x the largest bound of the shape.  Values are normal, signed
and O(1); the generator's seed is part of the shape's entry (0 everywhere: the lists pair a long K with results of at least
127 columns, so some product |a b| of the last k index is large; a shape that misses the factor gets another seed).

GUARDS: A, B and the bias live in buffers full of NaN, at an odd offset, with a leading dimension 3 above the extent and a
group stride 5 above a group: a read outside the operand puts a NaN into C, and no NaN may appear.  C lives in a buffer
prefilled with a bit pattern: two guard rows before, 3 guard columns (ldc = N + 3), 2 guard rows between groups and a guard
group of at least 128 rows after; every element outside the M x N results is bit-equal afterwards.  Nothing reads or writes
out of bounds on purpose: the buffers hold every address a correct kernel touches, and their tails (a row of NaN after the
last operand group, a full tile of rows after the last group of C) also hold what a row or k mask that is off by one, or a
missing row mask in the epilogue, would touch, so that such a kernel fails the test instead of leaving the buffers.

KERNEL 0's SPLIT (ct_ksplit, restated in ksplit_rule and asserted against what the launch reports): with blocks =
ceil(M / 64) * ceil(N / 64) * batch, ks = 1 if blocks >= 512 or K < 128, else min(ceil(K / 128), 512 // blocks), lowered
while ks * batch * M * N floats exceed the 2^24 floats of partials.  Split s covers k in [s * kc, min(K, (s + 1) * kc)) with
kc = ceil(K / ks) rounded up to 32.  No K of the list leaves a split empty (k_ranges checks it for every kernel 0 shape; an
empty one would have to write a zero partial and the result would still have to meet the bound).

Measured on the MI355X: largest error / bound 0.373 (kernel 0), 0.406 (kernel 1).
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FACTOR = 100.0
PATTERN = 0x5CA1AB1E
PAD, LD_GAP, Z_GAP = 7, 3, 5
SIZES = [1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257, 393]
KS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 127, 128, 129, 393, 515]
LAYOUTS = [("k", "j"), ("i", "j"), ("k", "k"), ("i", "k")]        # (A's fast index, B's fast index)


def _grid():
    """Every M, N and K of the lists with every layout pair: row r of layout pair c takes M, N, K at rotations of the lists
    that differ per pair, batch and bias alternate.  (M, N, K, A fast, B fast, batch, bias, seed)."""
    out = []
    for c, (la, lb) in enumerate(LAYOUTS):
        for r in range(len(KS)):
            out.append((SIZES[(r + 3 * c) % 12], SIZES[(5 * r + c + 7) % 12], KS[r], la, lb, (1, 3)[(r + c) % 2], (r // 2 + c) % 2 == 0, 0))
    return out


GRID = _grid()
# the AtlasNet step's own products in the cases of test_gpu_atlas_train.py (393 rows per primitive, 32805 encoder rows)
STEP_TILE = [(512, 512, 393, "i", "j", 16, False, 0),        # ragged16: weight gradient 512 -> 512
             (1024, 512, 393, "i", "j", 3, False, 0),        # weight gradient 1024 -> 512
             (393, 1024, 512, "k", "k", 3, False, 0),        # input gradient of 1024 -> 512
             (393, 512, 512, "k", "k", 3, False, 0),         # input gradient of 512 -> 512
             (393, 512, 3, "k", "k", 3, False, 0),           # last_conv's input gradient: K = 3
             (393, 512, 1024, "k", "j", 3, True, 0),         # the biased forward 1024 -> 512
             (32805, 64, 3, "k", "j", 1, True, 0),           # encoder_tiles: conv1 forward, K = 3, N = 64, 257 row tiles
             (8248, 512, 512, "k", "k", 1, False, 0)]        # one_primitive_tiles: input gradient, 65 row tiles, batch 1
STEP_SPLIT = [(512, 512, 393, "i", "j", 15, False, 0),       # ragged15: 240 tiles of 128 -> 960 blocks of 64, split 1
              (512, 3, 393, "i", "j", 16, False, 0),         # last_conv's weight gradient: N = 3, split 4
              (1200, 512, 1024, "k", "j", 1, True, 0),       # one_primitive: the biased forward with one group, split 3
              (1024, 1024, 4, "i", "j", 1, False, 0)]        # lin1's weight gradient over a batch of 4
# kernel 0: splits of 1, 2, 3, 4 and 5 with K off the chunk of 32
SPLITS = [(64, 65, 129, "k", "j", 1, True, 0), (33, 129, 385, "i", "k", 3, False, 0), (129, 31, 513, "k", "k", 1, True, 0),
          (257, 64, 515, "i", "j", 1, False, 0), (393, 393, 515, "k", "j", 3, True, 0), (63, 127, 127, "i", "j", 3, True, 0)]
SHAPES = [(0,) + s for s in GRID + STEP_SPLIT + SPLITS] + [(1,) + s for s in GRID + STEP_TILE]
REPEAT = [(0,) + SPLITS[0], (0,) + SPLITS[4], (0,) + GRID[9], (0,) + STEP_SPLIT[1], (1,) + GRID[13], (1,) + GRID[30], (1,) + STEP_TILE[4],
          (1,) + STEP_TILE[0]]
WORST = {0: 0.0, 1: 0.0}


def _id(s):
    return "k%d-%dx%dx%d-A%s-B%s-b%d-%s" % (s[0], s[1], s[2], s[3], s[4], s[5], s[6], "bias" if s[7] else "nobias") + ("-s%d" % s[8] if s[8] else "")


def cdiv(a, b):
    return -(-a // b)


def ksplit_rule(M, N, K, batch):
    """ct_ksplit of csrc/train_tile.h, restated."""
    blocks = cdiv(M, 64) * cdiv(N, 64) * batch
    ks = 1
    if blocks < 512 and K >= 128:
        ks = min(cdiv(K, 128), 512 // blocks)
        while ks > 1 and ks * batch * M * N > 1 << 24:
            ks -= 1
    return ks


def k_ranges(K, ks):
    kc = cdiv(cdiv(K, ks), 32) * 32
    return [(s * kc, min(K, (s + 1) * kc)) for s in range(ks)]


@functools.lru_cache(maxsize=4)
def host_case(shape):
    """The operands in their guarded host buffers, the float64 reference and bound, and the proof that the shape can fail."""
    kernel, M, N, K, la, lb, batch, with_bias, seed = shape
    rng = np.random.default_rng([seed, M, N, K, batch])
    A = rng.standard_normal((batch, M, K)).astype(np.float32)
    B = rng.standard_normal((batch, K, N)).astype(np.float32)
    bias = rng.standard_normal((batch, N)).astype(np.float32) if with_bias else None
    if with_bias and kernel == 0:
        bias[:] = bias[0]                                   # one bias for all groups
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    b64 = bias.astype(np.float64)[:, None, :] if with_bias else 0.0
    C64 = A64 @ B64 + b64
    bound = (K + 4) * U * (np.abs(A64) @ np.abs(B64) + np.abs(b64))
    drop_k = np.abs(A64[:, :, K - 1:] @ B64[:, K - 1:, :]).max()
    shifted = np.concatenate([np.zeros((batch, 1, K)), A64[:, :-1]], axis=1)
    shift_rows = np.abs(C64 - (shifted @ B64 + b64)).max()
    can_fail = (float(drop_k), float(shift_rows), float(bound.max()))

    def operand(X, fast_last):
        """X [batch][r][c] into a NaN buffer: element (z, i, j) at PAD + z * sz + i * ld + j (fast_last) or PAD + z * sz + j * ld + i."""
        _, r, c = X.shape
        rows, cols = (r, c) if fast_last else (c, r)
        ld = cols + LD_GAP
        sz = rows * ld + Z_GAP
        buf = np.full(PAD + batch * sz + ld + PAD, np.nan, np.float32)      # a row or k index one too far still reads a NaN of the buffer
        for z in range(batch):
            view = buf[PAD + z * sz: PAD + z * sz + rows * ld].reshape(rows, ld)[:, :cols]
            view[:] = X[z] if fast_last else X[z].T
        return buf, ld, sz

    bufA, lda, sAz = operand(A, la == "k")
    bufB, ldb, sBz = operand(B, lb == "j")
    a_strides = (lda, 1, sAz) if la == "k" else (1, lda, sAz)
    b_strides = (ldb, 1, sBz) if lb == "j" else (1, ldb, sBz)
    bufbias, bias_stride = None, 0
    if with_bias:
        per = N + 2
        groups = batch if kernel == 1 else 1
        bufbias = np.full(3 + groups * per + 3, np.nan, np.float32)
        for z in range(groups):
            bufbias[3 + z * per: 3 + z * per + N] = bias[z]
        bias_stride = per if kernel == 1 else 0
    ldc = N + LD_GAP
    sCz = (M + 2) * ldc
    c_off = 2 * ldc + 5
    c_len = c_off + batch * sCz + max(M + 2, 128) * ldc        # the guard after the last group holds every row of the last tile
    written = np.zeros(c_len, bool)
    for z in range(batch):
        written[c_off + z * sCz: c_off + z * sCz + M * ldc].reshape(M, ldc)[:, :N] = True
    return dict(bufA=bufA, a_strides=a_strides, bufB=bufB, b_strides=b_strides, bufbias=bufbias, bias_stride=bias_stride, ldc=ldc, sCz=sCz,
                c_off=c_off, c_len=c_len, written=written, C64=C64, bound=bound, can_fail=can_fail)


def launch(shape, h):
    """One launch on fresh device buffers -> (the whole C buffer as int32 bits, the split taken)."""
    import torch
    from geometric_adv_amd import ops
    kernel, M, N, K, _, _, batch, _, _ = shape
    dev = torch.device("cuda:0")
    dA, dB = torch.from_numpy(h["bufA"]).to(dev), torch.from_numpy(h["bufB"]).to(dev)
    dbias = torch.from_numpy(h["bufbias"]).to(dev) if h["bufbias"] is not None else None
    dC = torch.full((h["c_len"],), PATTERN, dtype=torch.int32, device=dev).view(torch.float32)
    ks = ops.train_gemm(kernel, dA[PAD:], h["a_strides"], dB[PAD:], h["b_strides"], dC[h["c_off"]:], (h["ldc"], h["sCz"]),
                        dbias[3:] if dbias is not None else None, h["bias_stride"], M, N, K, batch)
    torch.cuda.synchronize()
    return dC.view(torch.int32).cpu().numpy(), ks


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_gemm_against_the_float64_product(shape):
    kernel, M, N, K, _, _, batch, _, _ = shape
    h = host_case(shape)
    drop_k, shift_rows, worst_bound = h["can_fail"]
    assert drop_k > FACTOR * worst_bound and shift_rows > FACTOR * worst_bound, h["can_fail"]
    bits, ks = launch(shape, h)
    if kernel == 0:
        assert ks == ksplit_rule(M, N, K, batch), (ks, ksplit_rule(M, N, K, batch))
        assert all(b > a for a, b in k_ranges(K, ks)), k_ranges(K, ks)
    else:
        assert ks == 1
    assert np.all(bits[~h["written"]] == PATTERN), "%d guard elements of C changed" % int(np.sum(bits[~h["written"]] != PATTERN))
    C = bits.view(np.float32)[h["written"]].reshape(batch, M, N)
    assert not np.isnan(C).any(), "%d NaN in C: the kernel read outside an operand" % int(np.isnan(C).sum())
    ratio = float((np.abs(C.astype(np.float64) - h["C64"]) / h["bound"]).max())
    WORST[kernel] = max(WORST[kernel], ratio)
    print("\n%s: split %d, error / bound %.3g (worst of kernel %d so far %.3g); can fail: drop k %.3g, shift rows %.3g against 100 x %.3g"
          % (_id(shape), ks, ratio, kernel, WORST[kernel], drop_k, shift_rows, worst_bound))
    assert ratio <= 1.0, ratio


def test_the_shape_lists_cover_what_they_promise():
    """Every M, N, K of the lists meets each layout pair on both kernels; kernel 0 takes splits of 1, 2 and at least 5 at a K
    off the chunk of 32; both batch sizes and both bias settings occur with every layout pair."""
    for kernel in (0, 1):
        mine = [s for s in SHAPES if s[0] == kernel]
        for la, lb in LAYOUTS:
            sub = [s for s in mine if (s[4], s[5]) == (la, lb)]
            assert {s[1] for s in sub} >= set(SIZES) and {s[2] for s in sub} >= set(SIZES) and {s[3] for s in sub} >= set(KS)
            assert {s[6] for s in sub} >= {1, 3} and {s[7] for s in sub} == {True, False}
    splits = {ksplit_rule(s[1], s[2], s[3], s[6]) for s in SHAPES if s[0] == 0 and s[3] % 32}
    assert {1, 2} <= splits and max(splits) >= 5, splits


@pytest.mark.parametrize("shape", REPEAT, ids=_id)
def test_the_same_launch_twice_is_bitwise_equal(shape):
    h = host_case(shape)
    first, ks = launch(shape, h)
    second, _ = launch(shape, h)
    if shape == REPEAT[1]:
        assert ks > 1
    assert np.array_equal(first, second)


def test_split_k_refuses_a_bias_per_group():
    import torch
    from geometric_adv_amd import ops
    dev = torch.device("cuda:0")
    a, b, c, bias = (torch.zeros(n, device=dev) for n in (3 * 8 * 8, 3 * 8 * 8, 3 * 8 * 8, 3 * 8))
    with pytest.raises(ValueError, match="one bias"):
        ops.train_gemm(ops.TRAIN_GEMM_SPLITK, a, (8, 1, 64), b, (8, 1, 64), c, (8, 64), bias, 8, 8, 8, 8, batch=3)
    assert ops.train_gemm(ops.TRAIN_GEMM_SPLITK, a, (8, 1, 64), b, (8, 1, 64), c, (8, 64), bias, 0, 8, 8, 8, batch=3) == 1
    with pytest.raises(ValueError, match="kernel"):
        ops.train_gemm(2, a, (8, 1, 64), b, (8, 1, 64), c, (8, 64), None, 0, 8, 8, 8, batch=3)
