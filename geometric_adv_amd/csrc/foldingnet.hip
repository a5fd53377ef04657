// geoadv_fold: the FoldingNet auto-encoder of the transfer experiment (transfer/foldingnet/foldingnet.py:14-189 with the
// graph of prepare_graph.py:24-73), inference only, fp32 throughout.
//
// Graph (per chunk of clouds; forward rebuilds it, geoadv_fold_graph returns it):
//   geoadv_knn_point_ws       k = 17 nearest neighbours of every point (grouping.hip), column 0 dropped as prepare_graph.py:61-66
//   fold_graph_count_kernel   in-degree of every point (atomics), the 3x3 covariance (ddof 1, float64, rounded to float)
//   fold_graph_scan_kernel    row capacities 16 + in-degree, exclusive scan per cloud (a cloud's rows hold 32 n entries)
//   fold_graph_fill_kernel    own 16 neighbours, then every j with i in L(j) appended to row i (atomic slot)
//   fold_graph_sort_kernel    one wave per row: stable rank sort and de-duplication -> the sorted, unique CSR row, degree
//   fold_pick_kernel          per (pool layer, cloud, point): 16 positions in [0, deg) -- given by the caller, or drawn on the
//                             device (below) -- resolved to neighbour columns
// Encoder:
//   fold_enc1_kernel          cat(xyz, cov) 12 -> 64 (VALU), conv2, conv3 64 -> 64 (MFMA), BN + ReLU   -> f1 [n][64]
//   fold_pool_conv4_kernel    graph pool 1 (max of 16 gathered rows and the point's own), ReLU, conv4 64 -> 128, BN, ReLU
//   fold_pool_conv5_kernel    graph pool 2, ReLU, conv5 128 -> 1024, BN (NO ReLU), max over points (order-preserving keys)
//   fc_batched_kernel x 3     fc1 1024 -> 512 + bn6 + ReLU; fc2 512 -> 512 (the code); the folds' per-cloud layer-1 shifts
//                             [W1_code | W2_code] . code + [b1 | b2]  (512 -> 1024)
// Decoder:
//   fold_dec_kernel           per 64-row tile of (cloud, grid point) rows: fold1 layer 1 = relu(shift1 + W1_grid . grid) built
//                             as the A operand of the 512 x 512 GEMM, ReLU, 512 -> 3 = p1 (kept in LDS); fold2 layer 1 =
//                             relu(shift2 + W2_p1 . p1), 512 x 512 GEMM, ReLU, 512 -> 3 = the reconstruction
//
// Device sampling (GEOADV_FOLD_PICKS_DEVICE).  mix(z) is splitmix64's finaliser:
//     z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9;  z = (z ^ (z >> 27)) * 0x94d049bb133111eb;  return z ^ (z >> 31)
// (all arithmetic modulo 2^64), G = 0x9e3779b97f4a7c15.  For cloud ordinal o (cloud_offset + index in the batch), pool layer
// l (0 or 1) and point i:  key = mix(mix(mix(seed + G) ^ o) ^ (l << 32 | i)).  Floyd's algorithm then draws the uniform
// 16-subset of [0, deg): for t = 0 .. 15, j = deg - 16 + t, r = mix(key + (t + 1) G), x = ((r >> 32) * (j + 1)) >> 32 (in
// [0, j]); pick x, or j if x was picked already.  The 16 picks are stored in that order.  Nothing depends on the batch, the
// chunking or the launch shape.
//
// Batch norm is folded at create time (eps 1e-5, eval mode): y = (x @ W) * scale + shift.  Per-point work does not depend
// on the point's position in its tile, no sum is split by batch size, so a cloud's results depend only on its points, its
// picks and (device sampling) its ordinal.  Every index read from the graph is clamped into its cloud, so a cloud with
// non-finite coordinates reads and writes only its own rows.
#include "point_tile.h"
#include "host_util.h"
#include "fold_graph.h"
#include <math.h>
#include <string.h>

namespace geoadv {

constexpr int FN_K = 17, FN_NB = 16, FN_LAT = PT_POOL, FN_CODE = 512;
constexpr int FN_GRID = 45, FN_G2 = FN_GRID * FN_GRID;
constexpr int FN_SCAN_THREADS = 1024;
constexpr size_t FN_DEC_LDS = sizeof(float) * (PT_ROWS * PT_SH + 2 * 3 * PT_ROWS + 3 * PT_ROWS + 2 * PT_ROWS) +
                              sizeof(int) * PT_ROWS;

__device__ __forceinline__ int fold_clamp(int j, int n) { return (unsigned)j < (unsigned)n ? j : 0; }

// ------------------------------------------------------------------------------------------------ graph
struct FoldGraph {                                  // one chunk of bc clouds; the CSR rows of cloud c start at c * 32 n
    const float *pc;                                // [bc][n][3]
    const int *knn;                                 // [bc][n][17]
    int *cnt, *fill, *off, *deg;                    // [bc][n]
    int *raw, *col;                                 // [bc][32 n]
    float *cov;                                     // [bc][n][9]
    float *cov_out;                                 // user, may be null
    int *knn_out, *deg_out;                         // user, may be null
    int n;
};

__global__ __launch_bounds__(256) void fold_graph_count_kernel(FoldGraph G) {
    const int c = blockIdx.y, n = G.n, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int *nb = G.knn + ((size_t)c * n + i) * FN_K + 1;
    const float *x = G.pc + (size_t)c * n * 3;
    double s[3] = {0, 0, 0}, p[3][3] = {};
    int L[FN_NB];
#pragma unroll
    for (int t = 0; t < FN_NB; ++t) {
        const int j = fold_clamp(nb[t], n);
        L[t] = j;
        atomicAdd(G.cnt + (size_t)c * n + j, 1);
        s[0] += x[3 * j]; s[1] += x[3 * j + 1]; s[2] += x[3 * j + 2];
    }
    const double m[3] = {s[0] / FN_NB, s[1] / FN_NB, s[2] / FN_NB};
#pragma unroll
    for (int t = 0; t < FN_NB; ++t) {
        const double d[3] = {x[3 * L[t]] - m[0], x[3 * L[t] + 1] - m[1], x[3 * L[t] + 2] - m[2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) p[a][b] += d[a] * d[b];
    }
    float *cv = G.cov + ((size_t)c * n + i) * 9;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float v = (float)(p[a][b] / (FN_NB - 1));
            cv[3 * a + b] = v;
            if (G.cov_out) G.cov_out[((size_t)c * n + i) * 9 + 3 * a + b] = v;
        }
    if (G.knn_out)
        for (int t = 0; t < FN_NB; ++t) G.knn_out[((size_t)c * n + i) * FN_NB + t] = L[t];
}

// one workgroup per cloud: off[i] = sum over r < i of (16 + cnt[r]); fill[] zeroed
__global__ __launch_bounds__(FN_SCAN_THREADS) void fold_graph_scan_kernel(FoldGraph G) {
    __shared__ int part[FN_SCAN_THREADS];
    const int c = blockIdx.x, n = G.n, t = threadIdx.x;
    const int per = (n + FN_SCAN_THREADS - 1) / FN_SCAN_THREADS, r0 = t * per, r1 = min(n, r0 + per);
    const int *cnt = G.cnt + (size_t)c * n;
    int s = 0;
    for (int r = r0; r < r1; ++r) s += FN_NB + cnt[r];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < FN_SCAN_THREADS; d <<= 1) {          // inclusive Hillis-Steele scan of the thread sums
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int o = part[t] - s;
    for (int r = r0; r < r1; ++r) {
        G.off[(size_t)c * n + r] = o;
        G.fill[(size_t)c * n + r] = 0;
        o += FN_NB + cnt[r];
    }
}

__global__ __launch_bounds__(256) void fold_graph_fill_kernel(FoldGraph G) {
    const int c = blockIdx.y, n = G.n, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int *nb = G.knn + ((size_t)c * n + j) * FN_K + 1;
    int *raw = G.raw + (size_t)c * 32 * n;
    const int *off = G.off + (size_t)c * n, *cnt = G.cnt + (size_t)c * n;
    int *fill = G.fill + (size_t)c * n;
    const int oj = off[j];
    for (int t = 0; t < FN_NB; ++t) {
        const int i = fold_clamp(nb[t], n);
        raw[oj + t] = i;
        const int slot = atomicAdd(fill + i, 1);
        if (slot < cnt[i]) raw[off[i] + FN_NB + slot] = j;
    }
}

// one wave per row: the row's 16 + cnt entries -> sorted unique columns at the same offset of `col`, and the degree
__global__ __launch_bounds__(256) void fold_graph_sort_kernel(FoldGraph G) {
    const int c = blockIdx.y, n = G.n, lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const size_t base = (size_t)c * 32 * n + G.off[(size_t)c * n + i];
    const int len = FN_NB + G.cnt[(size_t)c * n + i];
    const int *src = G.raw + base;
    int *dst = G.col + base;
    // stable rank: position of entry p = #{q : v_q < v_p} + #{q < p : v_q == v_p}
    for (int p0 = 0; p0 < len; p0 += 64) {
        const int p = p0 + lane;
        const int v = p < len ? src[p] : 0x7fffffff;
        int rank = 0;
        for (int q = 0; q < len; ++q) {
            const int u = src[q];
            rank += (u < v) | ((u == v) & (q < p));
        }
        if (p < len) dst[rank] = v;
    }
    __threadfence_block();
    // compaction in place: keep sorted entry r if r == 0 or it differs from entry r - 1
    int kept = 0, prev = -1;
    for (int p0 = 0; p0 < len; p0 += 64) {
        const int p = p0 + lane;
        const int v = p < len ? dst[p] : 0x7fffffff;
        int before = __shfl_up(v, 1);
        if (lane == 0) before = prev;
        const bool keep = p < len && v != before;
        const unsigned long long m = __ballot(keep);
        prev = __shfl(v, 63);
        const int pos = kept + __popcll(m & ((1ull << lane) - 1ull));
        if (keep) dst[pos] = v;
        kept += __popcll(m);
    }
    if (lane == 0) {
        G.deg[(size_t)c * n + i] = kept;
        if (G.deg_out) G.deg_out[(size_t)c * n + i] = kept;
    }
}

struct FoldPick {
    const int *deg, *off, *col;                     // chunk graph
    const int *given;                               // given mode: [2][b][n][16] of the whole call, else null
    int *picks_out, *cols_out;                      // user [2][b][n][16], may be null
    int *cols;                                      // [2][bc][n][16] the chunk's resolved columns
    unsigned long long seed;
    long long ordinal0;                             // cloud ordinal of the chunk's first cloud
    int n, bc, b, c0;                               // chunk size, call's batch, the chunk's first cloud in the call
};

__global__ __launch_bounds__(256) void fold_pick_kernel(FoldPick P) {
    const int n = P.n, i = blockIdx.x * 256 + threadIdx.x, c = blockIdx.y, l = blockIdx.z;
    if (i >= n) return;
    const int deg = P.deg[(size_t)c * n + i];
    const int *row = P.col + (size_t)c * 32 * n + P.off[(size_t)c * n + i];
    const size_t u = (((size_t)l * P.b + P.c0 + c) * n + i) * FN_NB;        // the call's layout
    const size_t w = (((size_t)l * P.bc + c) * n + i) * FN_NB;               // the chunk's layout
    int pk[FN_NB];
    if (P.given) {
#pragma unroll
        for (int t = 0; t < FN_NB; ++t) {
            const int q = P.given[u + t];
            pk[t] = (unsigned)q < (unsigned)deg ? q : deg - 1;               // never outside the row (Python refuses these)
        }
    } else {
        const unsigned long long o = (unsigned long long)(P.ordinal0 + c);
        const unsigned long long key =
            mix64(mix64(mix64(P.seed + kGolden64) ^ o) ^ (((unsigned long long)l << 32) | (unsigned)i));
#pragma unroll
        for (int t = 0; t < FN_NB; ++t) {
            const unsigned j = (unsigned)(deg - FN_NB + t);
            const unsigned long long r = mix64(key + (unsigned long long)(t + 1) * kGolden64);
            const unsigned x = (unsigned)(((r >> 32) * ((unsigned long long)j + 1)) >> 32);
            bool seen = false;
#pragma unroll
            for (int s = 0; s < t; ++s) seen |= pk[s] == (int)x;
            pk[t] = seen ? (int)j : (int)x;
        }
    }
#pragma unroll
    for (int t = 0; t < FN_NB; ++t) {
        const int colj = fold_clamp(row[(unsigned)pk[t] < (unsigned)deg ? pk[t] : 0], n);
        P.cols[w + t] = colj;
        if (P.cols_out) P.cols_out[u + t] = colj;
        if (P.picks_out && !P.given) P.picks_out[u + t] = pk[t];
    }
}

// ------------------------------------------------------------------------------------------------ encoder
struct FoldEncArgs {
    const float *pc, *cov;                          // [bc][n][3], [bc][n][9]
    const float *w0, *sc0, *sh0;                    // conv1 [12][64]
    PackedLayer l1, l2, l3, l4;                     // conv2, conv3 64 -> 64; conv4 64 -> 128; conv5 128 -> 1024
    const float *sc[5], *sh[5];
    const int *cols;                                // [2][bc][n][16]
    float *f1, *f2;                                 // [bc][n][64], [bc][n][128]
    unsigned *keys;                                 // [bc][1024], zeroed before the launch
    int n, bc, slices;
};

__global__ __launch_bounds__(PT_THREADS, 2) void fold_enc1_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[PT_ROWS * PT_SA];
    __shared__ __attribute__((aligned(16))) float bufB[PT_ROWS * PT_SA];
    __shared__ float in[PT_ROWS * 12];
    const int tile = blockIdx.x, c = blockIdx.y, n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    for (int e = threadIdx.x; e < PT_ROWS * 12; e += PT_THREADS) {
        const int r = e / 12, k = e - 12 * r;
        const size_t p = (size_t)c * n + n0 + r;
        in[e] = r < live ? (k < 3 ? A.pc[p * 3 + k] : A.cov[p * 9 + k - 3]) : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < PT_ROWS * 64; e += PT_THREADS) {      // conv1 12 -> 64 on the VALU
        const int r = e >> 6, o = e & 63;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) a = fmaf(in[12 * r + k], A.w0[64 * k + o], a);
        bufA[r * PT_SA + o] = fmaxf(a * A.sc0[o] + A.sh0[o], 0.f);
    }
    __syncthreads();
    layer_gemm<PT_ROWS, 64, 1>(bufA, PT_SA, A.l1, nullptr, [&](int row, int col, float a) {
        bufB[row * PT_SA + col] = fmaxf(a * A.sc[1][col] + A.sh[1][col], 0.f);
    });
    __syncthreads();
    float *f1 = A.f1 + ((size_t)c * n + n0) * 64;
    layer_gemm<PT_ROWS, 64, 1>(bufB, PT_SA, A.l2, nullptr, [&](int row, int col, float a) {
        if (row < live) f1[(size_t)row * 64 + col] = fmaxf(a * A.sc[2][col] + A.sh[2][col], 0.f);
    });
}

// Graph pooling of a tile: out[r][:] = relu(max(x_i, max over the 16 picked neighbours)), W channels, rows past n zero
template <int W>
__device__ __forceinline__ void fold_pool(const float *f, const int *cols, int n0, int live, float *out, int s_out) {
    constexpr int Q = W / 4;
    for (int e = threadIdx.x; e < PT_ROWS * Q; e += PT_THREADS) {
        const int r = e / Q, q = e - Q * r;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < live) {
            const int i = n0 + r;
            v = *reinterpret_cast<const float4 *>(f + (size_t)i * W + 4 * q);
            const int *cl = cols + (size_t)i * FN_NB;
#pragma unroll 4
            for (int t = 0; t < FN_NB; ++t) {
                const float4 g = *reinterpret_cast<const float4 *>(f + (size_t)cl[t] * W + 4 * q);
                v.x = fmaxf(v.x, g.x); v.y = fmaxf(v.y, g.y); v.z = fmaxf(v.z, g.z); v.w = fmaxf(v.w, g.w);
            }
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        }
        *reinterpret_cast<float4 *>(out + r * s_out + 4 * q) = v;
    }
}

__global__ __launch_bounds__(PT_THREADS, 2) void fold_pool_conv4_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[PT_ROWS * PT_SA];
    const int tile = blockIdx.x, c = blockIdx.y, n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    fold_pool<64>(A.f1 + (size_t)c * n * 64, A.cols + (size_t)c * n * FN_NB, n0, live, bufA, PT_SA);
    __syncthreads();
    float *f2 = A.f2 + ((size_t)c * n + n0) * 128;
    layer_gemm<PT_ROWS, 128, 1>(bufA, PT_SA, A.l3, nullptr, [&](int row, int col, float a) {
        if (row < live) f2[(size_t)row * 128 + col] = fmaxf(a * A.sc[3][col] + A.sh[3][col], 0.f);
    });
}

__global__ __launch_bounds__(PT_THREADS, 2) void fold_pool_conv5_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufB[PT_ROWS * PT_SB];
    const int tile = blockIdx.x, c = blockIdx.y, slice = blockIdx.z, n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    fold_pool<128>(A.f2 + (size_t)c * n * 128, A.cols + ((size_t)A.bc + c) * n * FN_NB, n0, live, bufB, PT_SB);
    __syncthreads();
    pooled_wide_layer(bufB, PT_SB, A.l4, A.sc[4], A.sh[4], slice, A.slices, live, A.keys + (size_t)c * FN_LAT,
                      [](float v) { return float_key(v); });
}

// ------------------------------------------------------------------------------------------------ decoder
struct FoldDecArgs {
    const float *lin;                               // [45] np.linspace(-0.3, 0.3, 45) as float
    const float *shift;                             // [bc][1024]: fold1's layer-1 shift | fold2's
    const float *wg;                                // [2][512] fold1.conv1's grid rows
    const float *wp;                                // [3][512] fold2.conv1's p1 rows
    PackedLayer l2a, l2b;                           // fold1.conv2, fold2.conv2
    const float *b2a, *b2b;                         // [512]
    const float *w3a, *b3a, *w3b, *b3b;             // conv3 [512][3], [3]
    float *p1, *recon;                              // [bc][2025][3]; p1 may be null
    int bc;
};

__global__ __launch_bounds__(PT_THREADS) void fold_dec_kernel(FoldDecArgs A) {
    extern __shared__ __attribute__((aligned(16))) float fn_lds[];
    float *H = fn_lds;                                          // [64][PT_SH]
    float *part = H + PT_ROWS * PT_SH;                          // [2][64 * 3]
    float *pt = part + 2 * 3 * PT_ROWS;                         // [64][3] p1, then the output
    float *gxy = pt + 3 * PT_ROWS;                              // [64][2] grid coordinates
    int *rcloud = reinterpret_cast<int *>(gxy + 2 * PT_ROWS);   // [64]
    const int rows = A.bc * FN_G2, r0 = blockIdx.x * PT_ROWS;
    const int live = rows - r0 < PT_ROWS ? rows - r0 : PT_ROWS;
    if (threadIdx.x < PT_ROWS) {
        const int r = r0 + (threadIdx.x < live ? threadIdx.x : 0);     // padding rows repeat the tile's first row
        const int c = r / FN_G2, p = r - c * FN_G2;
        rcloud[threadIdx.x] = c;
        gxy[2 * threadIdx.x] = A.lin[p % FN_GRID];                      // point p = row * 45 + column is (x_column, y_row)
        gxy[2 * threadIdx.x + 1] = A.lin[p / FN_GRID];
    }
    __syncthreads();
    // fold1 layer 1: relu(shift1 + W_grid . (x, y))
    for (int e = threadIdx.x; e < PT_ROWS * (PT_HID / 4); e += PT_THREADS) {
        const int r = e >> 7, k = 4 * (e & 127);
        const float4 s = *reinterpret_cast<const float4 *>(A.shift + (size_t)rcloud[r] * 2 * PT_HID + k);
        const float4 w0 = *reinterpret_cast<const float4 *>(A.wg + k), w1 = *reinterpret_cast<const float4 *>(A.wg + PT_HID + k);
        const float x = gxy[2 * r], y = gxy[2 * r + 1];
        *reinterpret_cast<float4 *>(H + r * PT_SH + k) =
            make_float4(fmaxf(fmaf(w1.x, y, fmaf(w0.x, x, s.x)), 0.f), fmaxf(fmaf(w1.y, y, fmaf(w0.y, x, s.y)), 0.f),
                        fmaxf(fmaf(w1.z, y, fmaf(w0.z, x, s.z)), 0.f), fmaxf(fmaf(w1.w, y, fmaf(w0.w, x, s.w)), 0.f));
    }
    __syncthreads();
    dec512_hidden<false>(H, A.l2a, nullptr, A.b2a);
    dec512_last(H, A.w3a, A.b3a, part, [&](int o, float y) { pt[o] = y; });
    __syncthreads();
    if (A.p1 && threadIdx.x < 3 * PT_ROWS && threadIdx.x / 3 < live) A.p1[(size_t)r0 * 3 + threadIdx.x] = pt[threadIdx.x];
    // fold2 layer 1: relu(shift2 + W_p1 . p1)
    for (int e = threadIdx.x; e < PT_ROWS * (PT_HID / 4); e += PT_THREADS) {
        const int r = e >> 7, k = 4 * (e & 127);
        const float4 s = *reinterpret_cast<const float4 *>(A.shift + (size_t)rcloud[r] * 2 * PT_HID + PT_HID + k);
        const float4 w0 = *reinterpret_cast<const float4 *>(A.wp + k), w1 = *reinterpret_cast<const float4 *>(A.wp + PT_HID + k),
                     w2 = *reinterpret_cast<const float4 *>(A.wp + 2 * PT_HID + k);
        const float x = pt[3 * r], y = pt[3 * r + 1], z = pt[3 * r + 2];
        *reinterpret_cast<float4 *>(H + r * PT_SH + k) =
            make_float4(fmaxf(fmaf(w2.x, z, fmaf(w1.x, y, fmaf(w0.x, x, s.x))), 0.f),
                        fmaxf(fmaf(w2.y, z, fmaf(w1.y, y, fmaf(w0.y, x, s.y))), 0.f),
                        fmaxf(fmaf(w2.z, z, fmaf(w1.z, y, fmaf(w0.z, x, s.z))), 0.f),
                        fmaxf(fmaf(w2.w, z, fmaf(w1.w, y, fmaf(w0.w, x, s.w))), 0.f));
    }
    __syncthreads();
    dec512_hidden<false>(H, A.l2b, nullptr, A.b2b);
    dec512_last(H, A.w3b, A.b3b, part, [&](int o, float y) { pt[o] = y; });
    __syncthreads();
    if (A.recon && threadIdx.x < 3 * PT_ROWS && threadIdx.x / 3 < live) A.recon[(size_t)r0 * 3 + threadIdx.x] = pt[threadIdx.x];
}

}  // namespace geoadv

using namespace geoadv;

struct geoadv_fold {
    void *arena;
    const float *w0, *sc[6], *sh[6];                // conv1 [12][64]; folded BN of conv1..conv5, fc1
    const float *pk[4];                             // conv2, conv3, conv4, conv5 packed
    const float *fc1, *fc2, *fc2b, *shw, *shb;      // fc1 [1024][512], fc2 [512][512] + bias, shift [512][1024] + bias
    const float *lin, *wg, *wp;                     // grid linspace, fold1 grid rows, fold2 p1 rows
    const float *pk2a, *pk2b, *b2a, *b2b, *w3a, *b3a, *w3b, *b3b;
};

extern "C" int geoadv_fold_create(geoadv_fold **out, const geoadv_fold_weights *hw) {
    GA_REQUIRE(out && hw, "fold_create: null argument");
    for (int l = 0; l < GEOADV_FOLD_ENC_LAYERS; ++l) {
        GA_REQUIRE(hw->enc_w[l] && hw->enc_b[l], "fold_create: null encoder weight pointer at layer %d", l);
        const bool bn = l < GEOADV_FOLD_ENC_LAYERS - 1;
        if (bn)
            GA_REQUIRE(hw->enc_gamma[l] && hw->enc_beta[l] && hw->enc_mean[l] && hw->enc_var[l],
                       "fold_create: null batch-norm pointer at encoder layer %d", l);
        else
            GA_REQUIRE(!hw->enc_gamma[l] && !hw->enc_beta[l] && !hw->enc_mean[l] && !hw->enc_var[l],
                       "fold_create: fc2 has no batch norm: its batch-norm pointers must be NULL");
    }
    for (int l = 0; l < GEOADV_FOLD_DEC_LAYERS; ++l)
        GA_REQUIRE(hw->dec_w[l] && hw->dec_b[l], "fold_create: null decoder pointer at layer %d", l);
    static const int ein[6] = {12, 64, 64, 64, 128, FN_LAT}, eout[6] = {64, 64, 64, 128, FN_LAT, FN_CODE};
    HostArena arena;
    std::vector<float> &host = arena.host;
    size_t o_w0, o_sc[6], o_sh[6], o_pk[4], o_fc1, o_fc2, o_fc2b, o_shw, o_shb, o_lin, o_wg, o_wp;
    size_t o_pk2a, o_pk2b, o_b2a, o_b2b, o_w3a, o_b3a, o_w3b, o_b3b;
    o_w0 = arena.reserve(12 * 64);
    memcpy(&host[o_w0], hw->enc_w[0], sizeof(float) * 12 * 64);
    for (int l = 1; l <= 4; ++l) {
        o_pk[l - 1] = arena.reserve((size_t)ein[l] * eout[l]);
        pack_fragments(&host[o_pk[l - 1]], hw->enc_w[l], ein[l], eout[l]);
    }
    for (int l = 0; l < 6; ++l) {
        o_sc[l] = arena.reserve(eout[l]);
        o_sh[l] = arena.reserve(eout[l]);
        fold_bn_torch(&host[o_sc[l]], &host[o_sh[l]], eout[l], hw->enc_b[l], hw->enc_gamma[l], hw->enc_beta[l], hw->enc_mean[l],
                hw->enc_var[l]);
    }
    o_fc1 = arena.reserve((size_t)FN_LAT * FN_CODE);
    memcpy(&host[o_fc1], hw->enc_w[5], sizeof(float) * FN_LAT * FN_CODE);
    o_fc2 = arena.reserve((size_t)FN_CODE * FN_CODE);
    memcpy(&host[o_fc2], hw->enc_w[6], sizeof(float) * FN_CODE * FN_CODE);
    o_fc2b = arena.reserve(FN_CODE);
    memcpy(&host[o_fc2b], hw->enc_b[6], sizeof(float) * FN_CODE);
    // the folds' code rows side by side: shift[c][0:512] = code . W1[0:512] + b1, shift[c][512:1024] = code . W2[0:512] + b2
    o_shw = arena.reserve((size_t)FN_CODE * 2 * PT_HID);
    o_shb = arena.reserve(2 * PT_HID);
    for (int f = 0; f < 2; ++f) {
        const float *w = hw->dec_w[3 * f];
        for (int k = 0; k < FN_CODE; ++k)
            memcpy(&host[o_shw + (size_t)k * 2 * PT_HID + f * PT_HID], w + (size_t)k * PT_HID, sizeof(float) * PT_HID);
        memcpy(&host[o_shb + f * PT_HID], hw->dec_b[3 * f], sizeof(float) * PT_HID);
    }
    o_lin = arena.reserve(FN_GRID);
    for (int i = 0; i < FN_GRID; ++i) {     // np.linspace(-0.3, 0.3, 45): start + i * step, the last point exactly the stop
        const double step = 0.6 / (FN_GRID - 1);
        host[o_lin + i] = (float)(i == FN_GRID - 1 ? 0.3 : -0.3 + i * step);
    }
    o_wg = arena.reserve(2 * PT_HID);
    memcpy(&host[o_wg], hw->dec_w[0] + (size_t)FN_CODE * PT_HID, sizeof(float) * 2 * PT_HID);
    o_wp = arena.reserve(3 * PT_HID);
    memcpy(&host[o_wp], hw->dec_w[3] + (size_t)FN_CODE * PT_HID, sizeof(float) * 3 * PT_HID);
    o_pk2a = arena.reserve((size_t)PT_HID * PT_HID);
    pack_fragments(&host[o_pk2a], hw->dec_w[1], PT_HID, PT_HID);
    o_pk2b = arena.reserve((size_t)PT_HID * PT_HID);
    pack_fragments(&host[o_pk2b], hw->dec_w[4], PT_HID, PT_HID);
    o_b2a = arena.reserve(PT_HID); memcpy(&host[o_b2a], hw->dec_b[1], sizeof(float) * PT_HID);
    o_b2b = arena.reserve(PT_HID); memcpy(&host[o_b2b], hw->dec_b[4], sizeof(float) * PT_HID);
    o_w3a = arena.reserve(PT_HID * 3); memcpy(&host[o_w3a], hw->dec_w[2], sizeof(float) * PT_HID * 3);
    o_w3b = arena.reserve(PT_HID * 3); memcpy(&host[o_w3b], hw->dec_w[5], sizeof(float) * PT_HID * 3);
    o_b3a = arena.reserve(3); memcpy(&host[o_b3a], hw->dec_b[2], sizeof(float) * 3);
    o_b3b = arena.reserve(3); memcpy(&host[o_b3b], hw->dec_b[5], sizeof(float) * 3);

    geoadv_fold *m = new geoadv_fold();
    if (int rc = arena.upload("fold_create", &m->arena)) {
        delete m;
        return rc;
    }
    const float *base = static_cast<const float *>(m->arena);
    m->w0 = base + o_w0;
    for (int l = 0; l < 6; ++l) { m->sc[l] = base + o_sc[l]; m->sh[l] = base + o_sh[l]; }
    for (int l = 0; l < 4; ++l) m->pk[l] = base + o_pk[l];
    m->fc1 = base + o_fc1; m->fc2 = base + o_fc2; m->fc2b = base + o_fc2b; m->shw = base + o_shw; m->shb = base + o_shb;
    m->lin = base + o_lin; m->wg = base + o_wg; m->wp = base + o_wp;
    m->pk2a = base + o_pk2a; m->pk2b = base + o_pk2b; m->b2a = base + o_b2a; m->b2b = base + o_b2b;
    m->w3a = base + o_w3a; m->b3a = base + o_b3a; m->w3b = base + o_w3b; m->b3b = base + o_b3b;
    *out = m;
    return GEOADV_OK;
}

extern "C" void geoadv_fold_destroy(geoadv_fold *fold) {
    if (!fold) return;
    (void)hipFree(fold->arena);
    delete fold;
}

namespace {
struct FoldScratch {
    float *kval; int *kidx;                          // [bc][n][17]
    char *knn_ws; size_t knn_bytes;
    int *cnt, *fill, *off, *deg;                     // [bc][n]
    int *raw, *col;                                  // [bc][32 n]
    float *cov;                                      // [bc][n][9]
    int *cols;                                       // [2][bc][n][16]
    float *f1, *f2;                                  // [bc][n][64], [bc][n][128]
    unsigned *keys;                                  // [bc][1024]
    float *h, *code, *shift;                         // [bc][512], [bc][512], [bc][1024]
    size_t bytes;
};
FoldScratch carve_fold(void *workspace, int bc, int n) {
    FoldScratch s;
    Carver cv(workspace);
    const size_t bn = (size_t)bc * n;
    s.kval = cv.take<float>(bn * FN_K);
    s.kidx = cv.take<int>(bn * FN_K);
    s.knn_bytes = geoadv_knn_workspace_bytes(bc, n, n, FN_K);
    s.knn_ws = cv.take<char>(s.knn_bytes);
    s.cnt = cv.take<int>(bn);
    s.fill = cv.take<int>(bn);
    s.off = cv.take<int>(bn);
    s.deg = cv.take<int>(bn);
    s.raw = cv.take<int>(bn * 32);
    s.col = cv.take<int>(bn * 32);
    s.cov = cv.take<float>(bn * 9);
    s.cols = cv.take<int>(2 * bn * FN_NB);
    s.f1 = cv.take<float>(bn * 64);
    s.f2 = cv.take<float>(bn * 128);
    s.keys = cv.take<unsigned>((size_t)bc * FN_LAT);
    s.h = cv.take<float>((size_t)bc * FN_CODE);
    s.code = cv.take<float>((size_t)bc * FN_CODE);
    s.shift = cv.take<float>((size_t)bc * 2 * PT_HID);
    s.bytes = cv.bytes();
    return s;
}
// clouds per chunk: about 2^17 points of graph and features at a time (2.6 KB per point), at most 1024 clouds
int fold_chunk(int b, int n) { return std::max(1, std::min(b, std::min(1024, (1 << 17) / n))); }

int fold_check(const char *who, int b, int n) {
    GA_REQUIRE(b >= 1, "%s: batch %d must be >= 1", who, b);
    GA_REQUIRE(n >= FN_K && n <= 16384, "%s: n %d out of range [17, 16384]", who, n);
    return GEOADV_OK;
}

// the graph of clouds [c0, c0 + bc): kNN, covariance, CSR rows, degrees (user copies offset to the call's cloud c0)
int fold_build_graph(const FoldScratch &s, int bc, int n, const float *pc, int *deg_out, int *knn_out, float *cov_out,
                     hipStream_t st) {
    if (int rc = geoadv_knn_point_ws(GEOADV_KNN_AUTO, bc, n, n, FN_K, pc, pc, s.kval, s.kidx, s.knn_ws, s.knn_bytes, st)) return rc;
    GA_HIP(hipMemsetAsync(s.cnt, 0, sizeof(int) * (size_t)bc * n, st));
    FoldGraph G{};
    G.pc = pc; G.knn = s.kidx; G.cnt = s.cnt; G.fill = s.fill; G.off = s.off; G.deg = s.deg; G.raw = s.raw; G.col = s.col;
    G.cov = s.cov; G.cov_out = cov_out; G.knn_out = knn_out; G.deg_out = deg_out; G.n = n;
    const dim3 g256(cdiv(n, 256), bc);
    hipLaunchKernelGGL(fold_graph_count_kernel, g256, dim3(256), 0, st, G);
    GA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fold_graph_scan_kernel, dim3(bc), dim3(FN_SCAN_THREADS), 0, st, G);
    GA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fold_graph_fill_kernel, g256, dim3(256), 0, st, G);
    GA_LAUNCH_CHECK();
    hipLaunchKernelGGL(fold_graph_sort_kernel, dim3(cdiv(n, 4), bc), dim3(256), 0, st, G);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
}  // namespace

// ---- the training step's graph (fold_graph.h): the same kernels over the whole batch as one chunk ----
size_t geoadv::fold_train_graph_bytes(int b, int n) { return carve_fold(nullptr, b, n).bytes + 256; }

int geoadv::fold_train_graph(int b, int n, const float *pc, int sampling, unsigned long long seed, long long ordinal0, int *picks,
                             void *workspace, hipStream_t st, FoldTrainGraph *out) {
    if (int rc = fold_check("fold_train_graph", b, n)) return rc;
    GA_REQUIRE((long long)b * n <= FOLD_TRAIN_MAX_ROWS, "fold_train_graph: batch * n exceeds 2^17 rows");
    GA_REQUIRE(pc && picks && workspace && out, "fold_train_graph: null argument");
    const FoldScratch s = carve_fold(workspace, b, n);
    if (int rc = fold_build_graph(s, b, n, pc, nullptr, nullptr, nullptr, st)) return rc;
    FoldPick P{};
    P.deg = s.deg; P.off = s.off; P.col = s.col;
    P.given = sampling == GEOADV_FOLD_PICKS_GIVEN ? picks : nullptr;
    P.picks_out = sampling == GEOADV_FOLD_PICKS_DEVICE ? picks : nullptr;
    P.cols_out = nullptr; P.cols = s.cols; P.seed = seed; P.ordinal0 = ordinal0;
    P.n = n; P.bc = b; P.b = b; P.c0 = 0;
    hipLaunchKernelGGL(fold_pick_kernel, dim3(cdiv(n, 256), b, 2), dim3(256), 0, st, P);
    GA_LAUNCH_CHECK();
    out->cov = s.cov; out->cols = s.cols; out->off = s.off; out->deg = s.deg; out->col = s.col;
    return GEOADV_OK;
}

extern "C" size_t geoadv_fold_workspace_bytes(const geoadv_fold *fold, int b, int n) {
    if (!fold || b <= 0 || n < FN_K || n > 16384) return 256;
    return carve_fold(nullptr, fold_chunk(b, n), n).bytes + 256;
}

extern "C" int geoadv_fold_graph(const geoadv_fold *fold, int b, int n, const float *pc, int *degree, int *knn, float *cov,
                                 void *workspace, void *stream) {
    GA_REQUIRE(fold, "fold_graph: null handle");
    if (int rc = fold_check("fold_graph", b, n)) return rc;
    GA_REQUIRE(pc && workspace, "fold_graph: null point cloud or workspace");
    hipStream_t st = as_stream(stream);
    const int bc = fold_chunk(b, n);
    const FoldScratch s = carve_fold(workspace, bc, n);
    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nbc = std::min(bc, b - c0);
        const size_t o = (size_t)c0 * n;
        if (int rc = fold_build_graph(s, nbc, n, pc + o * 3, degree ? degree + o : nullptr, knn ? knn + o * FN_NB : nullptr,
                                      cov ? cov + o * 9 : nullptr, st)) return rc;
    }
    return GEOADV_OK;
}

extern "C" int geoadv_fold_forward(const geoadv_fold *fold, int b, int n, const float *pc, int sampling,
                                   unsigned long long seed, long long cloud_offset, int *picks, int *cols, float *code,
                                   float *p1, float *recon, void *workspace, void *stream) {
    GA_REQUIRE(fold, "fold_forward: null handle");
    if (int rc = fold_check("fold_forward", b, n)) return rc;
    GA_REQUIRE(sampling == GEOADV_FOLD_PICKS_GIVEN || sampling == GEOADV_FOLD_PICKS_DEVICE,
               "fold_forward: sampling %d is not 0 (given) or 1 (device)", sampling);
    GA_REQUIRE(sampling == GEOADV_FOLD_PICKS_DEVICE || picks, "fold_forward: given sampling needs the picks");
    GA_REQUIRE(cloud_offset >= 0, "fold_forward: cloud_offset %lld must be >= 0", cloud_offset);
    GA_REQUIRE(pc && workspace, "fold_forward: null point cloud or workspace");
    static DeviceOnce attr;
    if (int rc = attr.run([]() -> int {
            GA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(fold_dec_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)FN_DEC_LDS));
            return GEOADV_OK;
        })) return rc;
    hipStream_t st = as_stream(stream);
    const int bc = fold_chunk(b, n);
    const FoldScratch s = carve_fold(workspace, bc, n);
    const int tiles = cdiv(n, PT_ROWS);
    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nbc = std::min(bc, b - c0);
        const size_t o = (size_t)c0 * n;
        const float *x = pc + o * 3;
        if (int rc = fold_build_graph(s, nbc, n, x, nullptr, nullptr, nullptr, st)) return rc;
        FoldPick P{};
        P.deg = s.deg; P.off = s.off; P.col = s.col;
        P.given = sampling == GEOADV_FOLD_PICKS_GIVEN ? picks : nullptr;
        P.picks_out = sampling == GEOADV_FOLD_PICKS_DEVICE ? picks : nullptr;
        P.cols_out = cols; P.cols = s.cols; P.seed = seed; P.ordinal0 = cloud_offset + c0;
        P.n = n; P.bc = nbc; P.b = b; P.c0 = c0;
        hipLaunchKernelGGL(fold_pick_kernel, dim3(cdiv(n, 256), nbc, 2), dim3(256), 0, st, P);
        GA_LAUNCH_CHECK();

        const int slices = pooled_slices(tiles, nbc);
        FoldEncArgs ea{};
        ea.pc = x; ea.cov = s.cov; ea.w0 = fold->w0; ea.sc0 = fold->sc[0]; ea.sh0 = fold->sh[0];
        ea.l1 = PackedLayer{fold->pk[0], 64, 64}; ea.l2 = PackedLayer{fold->pk[1], 64, 64};
        ea.l3 = PackedLayer{fold->pk[2], 64, 128}; ea.l4 = PackedLayer{fold->pk[3], 128, FN_LAT};
        for (int l = 0; l < 5; ++l) { ea.sc[l] = fold->sc[l]; ea.sh[l] = fold->sh[l]; }
        ea.cols = s.cols; ea.f1 = s.f1; ea.f2 = s.f2; ea.keys = s.keys; ea.n = n; ea.bc = nbc; ea.slices = slices;
        hipLaunchKernelGGL(fold_enc1_kernel, dim3(tiles, nbc), dim3(PT_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(fold_pool_conv4_kernel, dim3(tiles, nbc), dim3(PT_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        GA_HIP(hipMemsetAsync(s.keys, 0, sizeof(unsigned) * (size_t)nbc * FN_LAT, st));
        hipLaunchKernelGGL(fold_pool_conv5_kernel, dim3(tiles, nbc, slices), dim3(PT_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();

        const int fy = cdiv(nbc, FC_CLOUDS);
        float *cd = code ? code + (size_t)c0 * FN_CODE : s.code;
        FcBatchedArgs fa{};
        fa.keys = s.keys; fa.w = fold->fc1; fa.sc = fold->sc[5]; fa.sh = fold->sh[5]; fa.out = s.h; fa.N = FN_CODE;
        fa.b = nbc; fa.relu = 1;
        hipLaunchKernelGGL(fc_batched_kernel<FN_LAT>, dim3(FN_CODE / 64, fy), dim3(FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        fa.keys = nullptr; fa.in = s.h; fa.w = fold->fc2; fa.sc = nullptr; fa.sh = fold->fc2b; fa.out = cd; fa.relu = 0;
        hipLaunchKernelGGL(fc_batched_kernel<FN_CODE>, dim3(FN_CODE / 64, fy), dim3(FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        fa.in = cd; fa.w = fold->shw; fa.sh = fold->shb; fa.out = s.shift; fa.N = 2 * PT_HID;
        hipLaunchKernelGGL(fc_batched_kernel<FN_CODE>, dim3(2 * PT_HID / 64, fy), dim3(FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();

        FoldDecArgs da{};
        da.lin = fold->lin; da.shift = s.shift; da.wg = fold->wg; da.wp = fold->wp;
        da.l2a = PackedLayer{fold->pk2a, PT_HID, PT_HID}; da.l2b = PackedLayer{fold->pk2b, PT_HID, PT_HID};
        da.b2a = fold->b2a; da.b2b = fold->b2b; da.w3a = fold->w3a; da.b3a = fold->b3a; da.w3b = fold->w3b; da.b3b = fold->b3b;
        da.p1 = p1 ? p1 + (size_t)c0 * FN_G2 * 3 : nullptr;
        da.recon = recon ? recon + (size_t)c0 * FN_G2 * 3 : nullptr;
        da.bc = nbc;
        if (recon || p1) {
            hipLaunchKernelGGL(fold_dec_kernel, dim3(cdiv(nbc * FN_G2, PT_ROWS)), dim3(PT_THREADS), FN_DEC_LDS, st, da);
            GA_LAUNCH_CHECK();
        }
    }
    return GEOADV_OK;
}
