// Per-point / per-row tile code shared by the three inference models (classifier.hip, atlasnet.hip, foldingnet.hip), on
// top of mfma_tile.h: the point loader with the 3 -> 64 VALU layer, the pooled 128 -> 1024 layer, the batched FC kernel
// and the pieces of the 512-wide decoders.  A workgroup is 512 threads (8 waves) on a tile of 64 rows.  Every sum order is
// written out here once: a change reaches all three models.
#pragma once
#include "mfma_tile.h"

namespace geoadv {

constexpr int PT_ROWS = 64, PT_THREADS = 512;
constexpr int PT_SA = 68, PT_SB = 132;            // LDS row strides of 64- and 128-wide activations
constexpr int PT_POOL = 1024;                     // width of the pooled layer
constexpr int PT_HID = 512, PT_SH = PT_HID + 4;   // decoder width and the LDS row stride of its activations
constexpr int FC_CLOUDS = 8, FC_THREADS = 256;

// Order-preserving key of a float for an unsigned atomicMax (positive: the sign bit set; negative: every bit flipped).  The
// key of every real float is > 0, so 0 (a memset) is the identity of the max.
__device__ __forceinline__ unsigned float_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The tile's points x[0 .. live) (rows past `live` zero) into pts[64 * 3], then the 3 -> 64 layer on the VALU:
// bufA[r][c] = relu((x_r . w0[:, c]) * sc0[c] + sh0[c]) at row stride PT_SA, w0 [3][64] row-major.  Ends on a barrier.
__device__ __forceinline__ void load_points_conv1(const float *x, int live, const float *w0, const float *sc0, const float *sh0,
                                                  float *pts, float *bufA) {
    if (threadIdx.x < PT_ROWS * 3) {
        const int r = threadIdx.x / 3;
        pts[threadIdx.x] = r < live ? x[threadIdx.x] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PT_ROWS * 64; e += PT_THREADS) {
        const int r = e >> 6, c = e & 63;
        const float a = pts[3 * r] * w0[c] + pts[3 * r + 1] * w0[64 + c] + pts[3 * r + 2] * w0[128 + c];
        bufA[r * PT_SA + c] = fmaxf(a * sc0[c] + sh0[c], 0.f);
    }
    __syncthreads();
}

// The pooled 128 -> 1024 layer of a tile in buf[64][stride]: the 32-column blocks of this workgroup's slice dealt to the 8
// waves, both row blocks per wave; out[col] = max(out[col], key(acc * scale + shift)) over the tile's live rows -- in
// registers, then across the wave's halves, then across tiles by the atomic.  `key` maps a value to an unsigned that orders
// like it and is > 0 for whatever should count; `out` [1024] is zeroed before the launch.
template <class Key>
__device__ __forceinline__ void pooled_wide_layer(const float *buf, int stride, const PackedLayer &L, const float *scale,
                                                  const float *shift, int slice, int slices, int live, unsigned *out, Key key) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, i = lane & 31;
    const int nblk = (PT_POOL / 32) / slices;
    for (int j = wave; j < nblk; j += PT_THREADS / 64) {
        const int cb = slice * nblk + j;
        f32x16 acc[2] = {};
        gemm_chain<2>(buf, stride, 0, L, cb, 0, 128 / 8, acc);
        const int col = cb * 32 + i;
        const float sc = scale[col], sh = shift[col];
        unsigned m = 0;
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rm * 32 + acc_row(r, h);
                const unsigned v = key(acc[rm][r] * sc + sh);
                if (row < live) m = max(m, v);
            }
        m = max(m, (unsigned)__shfl_xor((int)m, 32));
        if (h == 0 && m != 0) atomicMax(out + col, m);
    }
}

// load_points_conv1 for a tile of GATHERED rows: row s of the tile is point rows[s] of the cloud x[n][3] (s < live; rows
// past `live` zero).  The same products and sums per row, so a gathered row's activations carry the bits its own tile gave it.
__device__ __forceinline__ void gather_points_conv1(const float *x, const int *rows, int live, const float *w0, const float *sc0,
                                                    const float *sh0, float *pts, float *bufA) {
    if (threadIdx.x < PT_ROWS * 3) {
        const int r = threadIdx.x / 3;
        pts[threadIdx.x] = r < live ? x[(size_t)rows[r] * 3 + (threadIdx.x - 3 * r)] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PT_ROWS * 64; e += PT_THREADS) {
        const int r = e >> 6, c = e & 63;
        const float a = pts[3 * r] * w0[c] + pts[3 * r + 1] * w0[64 + c] + pts[3 * r + 2] * w0[128 + c];
        bufA[r * PT_SA + c] = fmaxf(a * sc0[c] + sh0[c], 0.f);
    }
    __syncthreads();
}

// The recomputing pass behind pooled_wide_layer: the same blocks, chains and keys, compared with the finished pool
// `pooled` [1024]; win[col] = min(win[col], row0 + row) over the tile's live rows whose key equals pooled[col] != 0 -- the
// lowest row among equal maxima, whatever the order of tiles.  `win` is preset to a value above every row.
template <class Key>
__device__ __forceinline__ void pooled_wide_winners(const float *buf, int stride, const PackedLayer &L, const float *scale,
                                                    const float *shift, int slice, int slices, int live, int row0,
                                                    const unsigned *pooled, int *win, Key key) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, i = lane & 31;
    const int nblk = (PT_POOL / 32) / slices;
    for (int j = wave; j < nblk; j += PT_THREADS / 64) {
        const int cb = slice * nblk + j;
        f32x16 acc[2] = {};
        gemm_chain<2>(buf, stride, 0, L, cb, 0, 128 / 8, acc);
        const int col = cb * 32 + i;
        const float sc = scale[col], sh = shift[col];
        const unsigned want = pooled[col];
        int best = 0x7fffffff;
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rm * 32 + acc_row(r, h);
                const unsigned v = key(acc[rm][r] * sc + sh);
                if (row < live && v == want) best = min(best, row0 + row);
            }
        best = min(best, __shfl_xor(best, 32));
        if (h == 0 && want != 0 && best != 0x7fffffff) atomicMin(win + col, best);
    }
}

// ------------------------------------------------------------------------------------------------ FC head (M = clouds)
// One workgroup: 64 output columns (a lane each) x 8 clouds, the K inputs split in four quarters over the 4 waves and summed
// in a fixed order -- the same for every cloud, whatever the batch size.  Grid (N / 64, ceil(b / 8)).
struct FcBatchedArgs {
    const unsigned *keys;                           // input as pooled keys [b][K], or
    const float *in;                                // as floats [b][K]
    const float *w, *sc, *sh;                       // [K][N] row-major; sc null: scale 1
    float *out;                                     // [b][N]
    int N, b, relu;
    const float *s1, *t1;                           // c non-null: c[cloud][p][:] = s1[p] * out + t1[p] for p < nb, s1 / t1 [nb][N]
    float *c;
    int nb;
};

template <int K>
__global__ __launch_bounds__(FC_THREADS) void fc_batched_kernel(FcBatchedArgs F) {
    __shared__ float xin[FC_CLOUDS][K];
    __shared__ float part[4][FC_CLOUDS][64];
    const int c0 = blockIdx.y * FC_CLOUDS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, N = F.N;
    for (int e = threadIdx.x; e < FC_CLOUDS * K; e += FC_THREADS) {
        const int j = e / K, k = e - j * K, c = c0 + j;
        float v = 0.f;
        if (c < F.b) v = F.keys ? float_unkey(F.keys[(size_t)c * K + k]) : F.in[(size_t)c * K + k];
        xin[j][k] = v;
    }
    __syncthreads();
    float acc[FC_CLOUDS] = {};
    const int k0 = wave * (K / 4);
    const float *w = F.w + (size_t)k0 * N + col;
#pragma unroll 8
    for (int k = 0; k < K / 4; ++k) {
        const float wv = w[(size_t)k * N];
#pragma unroll
        for (int j = 0; j < FC_CLOUDS; ++j) acc[j] = fmaf(xin[j][k0 + k], wv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < FC_CLOUDS; ++j) part[wave][j][lane] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < FC_CLOUDS * 64; e += FC_THREADS) {
        const int j = e >> 6, l = e & 63, c = c0 + j;
        if (c >= F.b) continue;
        const int o = blockIdx.x * 64 + l;
        const float s = (part[0][j][l] + part[1][j][l]) + (part[2][j][l] + part[3][j][l]);
        float y = F.sc ? s * F.sc[o] + F.sh[o] : s + F.sh[o];
        if (F.relu) y = fmaxf(y, 0.f);
        F.out[(size_t)c * N + o] = y;
        if (F.c)
            for (int p = 0; p < F.nb; ++p)
                F.c[((size_t)c * F.nb + p) * N + o] = fmaf(F.s1[(size_t)p * N + o], y, F.t1[(size_t)p * N + o]);
    }
}

// ------------------------------------------------------------------------------------------------ 512-wide decoder tile
// The activations of a tile's 64 rows live in H[64][PT_SH]; wave w owns the 32-column blocks 2w and 2w + 1 of a layer's 512
// outputs, both row blocks each: a 2 x 2 set of accumulators.

// relu(acc * scale + shift) (SCALE) or relu(acc + shift) of a wave's accumulators into H
template <bool SCALE>
__device__ __forceinline__ void dec512_epilogue(float *H, const f32x16 (&acc)[2][2], int cb0, const float *sc, const float *sh) {
    const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = (cb0 + q) * 32 + i;
        const float s = SCALE ? sc[col] : 1.f, t = sh[col];
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                H[(rm * 32 + acc_row(r, h)) * PT_SH + col] = fmaxf(SCALE ? acc[q][rm][r] * s + t : acc[q][rm][r] + t, 0.f);
    }
}

// 512 -> 512 layer of the tile in H, back into H (every wave has read all of H before the barrier that precedes the
// epilogue).  Ends on a barrier.
template <bool SCALE>
__device__ __forceinline__ void dec512_hidden(float *H, const PackedLayer &L, const float *sc, const float *sh) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cb0 = 2 * wave;
    f32x16 acc[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        acc[q][0] = acc[q][1] = f32x16{};
        gemm_chain<2>(H, PT_SH, 0, L, cb0 + q, 0, PT_HID / 8, acc[q]);
    }
    __syncthreads();
    dec512_epilogue<SCALE>(H, acc, cb0, sc, sh);
    __syncthreads();
}

// 512 -> 3 on the VALU: 192 (row, coordinate) outputs x two halves of K through part[2][192]; thread o < 192 hands
// y = (half 0 + half 1) + b3[o % 3] of row o / 3 to put(o, y).  w3 [512][3] row-major.  No barrier after put.
template <class Put>
__device__ __forceinline__ void dec512_last(const float *H, const float *w3, const float *b3, float *part, Put put) {
    if (threadIdx.x < 2 * 3 * PT_ROWS) {
        const int half = threadIdx.x / (3 * PT_ROWS), o = threadIdx.x - half * 3 * PT_ROWS;
        const int r = o / 3, d = o - 3 * r;
        const float *hr = H + r * PT_SH + half * (PT_HID / 2);
        const float *wk = w3 + half * (PT_HID / 2) * 3 + d;
        float a = 0.f;
#pragma unroll 8
        for (int k = 0; k < PT_HID / 2; ++k) a = fmaf(hr[k], wk[3 * k], a);
        part[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x < 3 * PT_ROWS) put((int)threadIdx.x, (part[threadIdx.x] + part[threadIdx.x + 3 * PT_ROWS]) + b3[threadIdx.x % 3]);
}

}  // namespace geoadv
