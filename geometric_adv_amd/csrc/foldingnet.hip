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
//   fold_fc_kernel x 3        fc1 1024 -> 512 + bn6 + ReLU; fc2 512 -> 512 (the code); the folds' per-cloud layer-1 shifts
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
#include "mfma_tile.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace geoadv {

constexpr int FN_ROWS = 64, FN_THREADS = 512, FN_K = 17, FN_NB = 16, FN_LAT = 1024, FN_CODE = 512, FN_HID = 512;
constexpr int FN_GRID = 45, FN_G2 = FN_GRID * FN_GRID;
constexpr int FN_SA = 68, FN_SB = 132;             // encoder LDS row strides (64- and 128-wide activations)
constexpr int FN_SH = FN_HID + 4;                  // decoder LDS row stride
constexpr int FN_FC_CLOUDS = 8, FN_FC_THREADS = 256;
constexpr int FN_SCAN_THREADS = 1024;
constexpr size_t FN_DEC_LDS = sizeof(float) * (FN_ROWS * FN_SH + 2 * 3 * FN_ROWS + 3 * FN_ROWS + 2 * FN_ROWS) +
                              sizeof(int) * FN_ROWS;

__device__ __forceinline__ unsigned fold_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fold_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ int fold_clamp(int j, int n) { return (unsigned)j < (unsigned)n ? j : 0; }

__device__ __forceinline__ unsigned long long fold_mix(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
constexpr unsigned long long FN_GOLDEN = 0x9e3779b97f4a7c15ull;

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
            fold_mix(fold_mix(fold_mix(P.seed + FN_GOLDEN) ^ o) ^ (((unsigned long long)l << 32) | (unsigned)i));
#pragma unroll
        for (int t = 0; t < FN_NB; ++t) {
            const unsigned j = (unsigned)(deg - FN_NB + t);
            const unsigned long long r = fold_mix(key + (unsigned long long)(t + 1) * FN_GOLDEN);
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

__global__ __launch_bounds__(FN_THREADS, 2) void fold_enc1_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[FN_ROWS * FN_SA];
    __shared__ __attribute__((aligned(16))) float bufB[FN_ROWS * FN_SA];
    __shared__ float in[FN_ROWS * 12];
    const int tile = blockIdx.x, c = blockIdx.y, n = A.n, n0 = tile * FN_ROWS;
    const int live = n - n0 < FN_ROWS ? n - n0 : FN_ROWS;
    for (int e = threadIdx.x; e < FN_ROWS * 12; e += FN_THREADS) {
        const int r = e / 12, k = e - 12 * r;
        const size_t p = (size_t)c * n + n0 + r;
        in[e] = r < live ? (k < 3 ? A.pc[p * 3 + k] : A.cov[p * 9 + k - 3]) : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < FN_ROWS * 64; e += FN_THREADS) {      // conv1 12 -> 64 on the VALU
        const int r = e >> 6, o = e & 63;
        float a = 0.f;
#pragma unroll
        for (int k = 0; k < 12; ++k) a = fmaf(in[12 * r + k], A.w0[64 * k + o], a);
        bufA[r * FN_SA + o] = fmaxf(a * A.sc0[o] + A.sh0[o], 0.f);
    }
    __syncthreads();
    layer_gemm<FN_ROWS, 64, 1>(bufA, FN_SA, A.l1, nullptr, [&](int row, int col, float a) {
        bufB[row * FN_SA + col] = fmaxf(a * A.sc[1][col] + A.sh[1][col], 0.f);
    });
    __syncthreads();
    float *f1 = A.f1 + ((size_t)c * n + n0) * 64;
    layer_gemm<FN_ROWS, 64, 1>(bufB, FN_SA, A.l2, nullptr, [&](int row, int col, float a) {
        if (row < live) f1[(size_t)row * 64 + col] = fmaxf(a * A.sc[2][col] + A.sh[2][col], 0.f);
    });
}

// Graph pooling of a tile: out[r][:] = relu(max(x_i, max over the 16 picked neighbours)), W channels, rows past n zero
template <int W>
__device__ __forceinline__ void fold_pool(const float *f, const int *cols, int n0, int live, float *out, int s_out) {
    constexpr int Q = W / 4;
    for (int e = threadIdx.x; e < FN_ROWS * Q; e += FN_THREADS) {
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

__global__ __launch_bounds__(FN_THREADS, 2) void fold_pool_conv4_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[FN_ROWS * FN_SA];
    const int tile = blockIdx.x, c = blockIdx.y, n = A.n, n0 = tile * FN_ROWS;
    const int live = n - n0 < FN_ROWS ? n - n0 : FN_ROWS;
    fold_pool<64>(A.f1 + (size_t)c * n * 64, A.cols + (size_t)c * n * FN_NB, n0, live, bufA, FN_SA);
    __syncthreads();
    float *f2 = A.f2 + ((size_t)c * n + n0) * 128;
    layer_gemm<FN_ROWS, 128, 1>(bufA, FN_SA, A.l3, nullptr, [&](int row, int col, float a) {
        if (row < live) f2[(size_t)row * 128 + col] = fmaxf(a * A.sc[3][col] + A.sh[3][col], 0.f);
    });
}

__global__ __launch_bounds__(FN_THREADS, 2) void fold_pool_conv5_kernel(FoldEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufB[FN_ROWS * FN_SB];
    const int tile = blockIdx.x, c = blockIdx.y, slice = blockIdx.z, n = A.n, n0 = tile * FN_ROWS;
    const int live = n - n0 < FN_ROWS ? n - n0 : FN_ROWS;
    fold_pool<128>(A.f2 + (size_t)c * n * 128, A.cols + ((size_t)A.bc + c) * n * FN_NB, n0, live, bufB, FN_SB);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, i = lane & 31;
    const int nblk = (FN_LAT / 32) / A.slices;
    unsigned *keys = A.keys + (size_t)c * FN_LAT;
    for (int j = wave; j < nblk; j += FN_THREADS / 64) {
        const int cb = slice * nblk + j;
        f32x16 acc[2] = {};
        gemm_chain<2>(bufB, FN_SB, 0, A.l4, cb, 0, 128 / 8, acc);
        const int col = cb * 32 + i;
        const float sc = A.sc[4][col], sh = A.sh[4][col];
        unsigned m = 0;                              // below the key of every float
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rm * 32 + acc_row(r, h);
                const unsigned v = fold_key(acc[rm][r] * sc + sh);
                if (row < live) m = max(m, v);
            }
        m = max(m, (unsigned)__shfl_xor((int)m, 32));
        if (h == 0 && m != 0) atomicMax(keys + col, m);
    }
}

// ------------------------------------------------------------------------------------------------ FC head (M = clouds)
// One workgroup: 64 output columns (a lane each) x 8 clouds, the K inputs split in four quarters over the 4 waves and summed
// in a fixed order -- the same for every cloud, whatever the batch size.
struct FoldFcArgs {
    const unsigned *keys;                           // input as pooled keys [bc][K], or
    const float *in;                                // as floats [bc][K]
    const float *w, *sc, *sh;                       // [K][N] row-major; sc null: scale 1
    float *out;                                     // [bc][N]
    int N, bc, relu;
};

template <int K>
__global__ __launch_bounds__(FN_FC_THREADS) void fold_fc_kernel(FoldFcArgs F) {
    __shared__ float xin[FN_FC_CLOUDS][K];
    __shared__ float part[4][FN_FC_CLOUDS][64];
    const int c0 = blockIdx.y * FN_FC_CLOUDS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane, N = F.N;
    for (int e = threadIdx.x; e < FN_FC_CLOUDS * K; e += FN_FC_THREADS) {
        const int j = e / K, k = e - j * K, c = c0 + j;
        float v = 0.f;
        if (c < F.bc) v = F.keys ? fold_unkey(F.keys[(size_t)c * K + k]) : F.in[(size_t)c * K + k];
        xin[j][k] = v;
    }
    __syncthreads();
    float acc[FN_FC_CLOUDS] = {};
    const int k0 = wave * (K / 4);
    const float *w = F.w + (size_t)k0 * N + col;
#pragma unroll 8
    for (int k = 0; k < K / 4; ++k) {
        const float wv = w[(size_t)k * N];
#pragma unroll
        for (int j = 0; j < FN_FC_CLOUDS; ++j) acc[j] = fmaf(xin[j][k0 + k], wv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < FN_FC_CLOUDS; ++j) part[wave][j][lane] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < FN_FC_CLOUDS * 64; e += FN_FC_THREADS) {
        const int j = e >> 6, l = e & 63, c = c0 + j;
        if (c >= F.bc) continue;
        const int o = blockIdx.x * 64 + l;
        const float s = (part[0][j][l] + part[1][j][l]) + (part[2][j][l] + part[3][j][l]);
        float y = F.sc ? s * F.sc[o] + F.sh[o] : s + F.sh[o];
        if (F.relu) y = fmaxf(y, 0.f);
        F.out[(size_t)c * N + o] = y;
    }
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

// relu(acc + bias) of a wave's 2 x 2 (column block, row block) accumulators into the LDS activation tile
__device__ __forceinline__ void fold_dec_epilogue(float *H, const f32x16 (&acc)[2][2], int cb0, const float *bias) {
    const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = (cb0 + q) * 32 + i;
        const float t = bias[col];
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) H[(rm * 32 + acc_row(r, h)) * FN_SH + col] = fmaxf(acc[q][rm][r] + t, 0.f);
    }
}

// 512 -> 512 GEMM of the tile in H, bias, ReLU, back into H (every wave reads all of H before the barrier)
__device__ __forceinline__ void fold_dec_hidden(float *H, const PackedLayer &L, const float *bias) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cb0 = 2 * wave;
    f32x16 acc[2][2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        acc[q][0] = acc[q][1] = f32x16{};
        gemm_chain<2>(H, FN_SH, 0, L, cb0 + q, 0, FN_HID / 8, acc[q]);
    }
    __syncthreads();
    fold_dec_epilogue(H, acc, cb0, bias);
    __syncthreads();
}

// 512 -> 3 on the VALU: 192 (row, coordinate) outputs x two halves of K; result in out[64][3]
__device__ __forceinline__ void fold_dec_last(const float *H, const float *w3, const float *b3, float *part, float *out) {
    if (threadIdx.x < 2 * 3 * FN_ROWS) {
        const int half = threadIdx.x / (3 * FN_ROWS), o = threadIdx.x - half * 3 * FN_ROWS;
        const int r = o / 3, d = o - 3 * r;
        const float *hr = H + r * FN_SH + half * (FN_HID / 2);
        const float *wk = w3 + half * (FN_HID / 2) * 3 + d;
        float a = 0.f;
#pragma unroll 8
        for (int k = 0; k < FN_HID / 2; ++k) a = fmaf(hr[k], wk[3 * k], a);
        part[threadIdx.x] = a;
    }
    __syncthreads();
    if (threadIdx.x < 3 * FN_ROWS) {
        const int d = threadIdx.x % 3;
        out[threadIdx.x] = (part[threadIdx.x] + part[threadIdx.x + 3 * FN_ROWS]) + b3[d];
    }
    __syncthreads();
}

__global__ __launch_bounds__(FN_THREADS) void fold_dec_kernel(FoldDecArgs A) {
    extern __shared__ __attribute__((aligned(16))) float fn_lds[];
    float *H = fn_lds;                                          // [64][FN_SH]
    float *part = H + FN_ROWS * FN_SH;                          // [2][64 * 3]
    float *pt = part + 2 * 3 * FN_ROWS;                         // [64][3] p1, then the output
    float *gxy = pt + 3 * FN_ROWS;                              // [64][2] grid coordinates
    int *rcloud = reinterpret_cast<int *>(gxy + 2 * FN_ROWS);   // [64]
    const int rows = A.bc * FN_G2, r0 = blockIdx.x * FN_ROWS;
    const int live = rows - r0 < FN_ROWS ? rows - r0 : FN_ROWS;
    if (threadIdx.x < FN_ROWS) {
        const int r = r0 + (threadIdx.x < live ? threadIdx.x : 0);     // padding rows repeat the tile's first row
        const int c = r / FN_G2, p = r - c * FN_G2;
        rcloud[threadIdx.x] = c;
        gxy[2 * threadIdx.x] = A.lin[p % FN_GRID];                      // point p = row * 45 + column is (x_column, y_row)
        gxy[2 * threadIdx.x + 1] = A.lin[p / FN_GRID];
    }
    __syncthreads();
    // fold1 layer 1: relu(shift1 + W_grid . (x, y))
    for (int e = threadIdx.x; e < FN_ROWS * (FN_HID / 4); e += FN_THREADS) {
        const int r = e >> 7, k = 4 * (e & 127);
        const float4 s = *reinterpret_cast<const float4 *>(A.shift + (size_t)rcloud[r] * 2 * FN_HID + k);
        const float4 w0 = *reinterpret_cast<const float4 *>(A.wg + k), w1 = *reinterpret_cast<const float4 *>(A.wg + FN_HID + k);
        const float x = gxy[2 * r], y = gxy[2 * r + 1];
        *reinterpret_cast<float4 *>(H + r * FN_SH + k) =
            make_float4(fmaxf(fmaf(w1.x, y, fmaf(w0.x, x, s.x)), 0.f), fmaxf(fmaf(w1.y, y, fmaf(w0.y, x, s.y)), 0.f),
                        fmaxf(fmaf(w1.z, y, fmaf(w0.z, x, s.z)), 0.f), fmaxf(fmaf(w1.w, y, fmaf(w0.w, x, s.w)), 0.f));
    }
    __syncthreads();
    fold_dec_hidden(H, A.l2a, A.b2a);
    fold_dec_last(H, A.w3a, A.b3a, part, pt);
    if (A.p1 && threadIdx.x < 3 * FN_ROWS && threadIdx.x / 3 < live) A.p1[(size_t)r0 * 3 + threadIdx.x] = pt[threadIdx.x];
    // fold2 layer 1: relu(shift2 + W_p1 . p1)
    for (int e = threadIdx.x; e < FN_ROWS * (FN_HID / 4); e += FN_THREADS) {
        const int r = e >> 7, k = 4 * (e & 127);
        const float4 s = *reinterpret_cast<const float4 *>(A.shift + (size_t)rcloud[r] * 2 * FN_HID + FN_HID + k);
        const float4 w0 = *reinterpret_cast<const float4 *>(A.wp + k), w1 = *reinterpret_cast<const float4 *>(A.wp + FN_HID + k),
                     w2 = *reinterpret_cast<const float4 *>(A.wp + 2 * FN_HID + k);
        const float x = pt[3 * r], y = pt[3 * r + 1], z = pt[3 * r + 2];
        *reinterpret_cast<float4 *>(H + r * FN_SH + k) =
            make_float4(fmaxf(fmaf(w2.x, z, fmaf(w1.x, y, fmaf(w0.x, x, s.x))), 0.f),
                        fmaxf(fmaf(w2.y, z, fmaf(w1.y, y, fmaf(w0.y, x, s.y))), 0.f),
                        fmaxf(fmaf(w2.z, z, fmaf(w1.z, y, fmaf(w0.z, x, s.z))), 0.f),
                        fmaxf(fmaf(w2.w, z, fmaf(w1.w, y, fmaf(w0.w, x, s.w))), 0.f));
    }
    __syncthreads();
    fold_dec_hidden(H, A.l2b, A.b2b);
    fold_dec_last(H, A.w3b, A.b3b, part, pt);
    if (A.recon && threadIdx.x < 3 * FN_ROWS && threadIdx.x / 3 < live) A.recon[(size_t)r0 * 3 + threadIdx.x] = pt[threadIdx.x];
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

namespace {
inline size_t fn_rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// W [K][N] row-major -> 32x32x2 fragments (ae.h): dst[((cb * K/8 + t) * 64 + lane) * 4 + u] = W[8t + 4(lane>>5) + u][32cb + (lane&31)]
void fn_pack(float *dst, const float *W, int K, int N) {
    const int kg = K / 8;
    for (int cb = 0; cb < N / 32; ++cb)
        for (int t = 0; t < kg; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u) {
                    const int k = 8 * t + 4 * (lane >> 5) + u, n = 32 * cb + (lane & 31);
                    dst[(((size_t)cb * kg + t) * 64 + lane) * 4 + u] = W[(size_t)k * N + n];
                }
}
void fn_fold(float *sc, float *sh, int N, const float *b, const float *g, const float *be, const float *m, const float *v) {
    for (int c = 0; c < N; ++c) {
        const float inv = g[c] * (1.0f / sqrtf(v[c] + 1e-5f));
        sc[c] = inv;
        sh[c] = (b[c] - m[c]) * inv + be[c];
    }
}
}  // namespace

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
    std::vector<float> host;
    auto reserve = [&](size_t count) { size_t off = fn_rup(host.size(), 64); host.resize(off + count, 0.f); return off; };
    size_t o_w0, o_sc[6], o_sh[6], o_pk[4], o_fc1, o_fc2, o_fc2b, o_shw, o_shb, o_lin, o_wg, o_wp;
    size_t o_pk2a, o_pk2b, o_b2a, o_b2b, o_w3a, o_b3a, o_w3b, o_b3b;
    o_w0 = reserve(12 * 64);
    memcpy(&host[o_w0], hw->enc_w[0], sizeof(float) * 12 * 64);
    for (int l = 1; l <= 4; ++l) {
        o_pk[l - 1] = reserve((size_t)ein[l] * eout[l]);
        fn_pack(&host[o_pk[l - 1]], hw->enc_w[l], ein[l], eout[l]);
    }
    for (int l = 0; l < 6; ++l) {
        o_sc[l] = reserve(eout[l]);
        o_sh[l] = reserve(eout[l]);
        fn_fold(&host[o_sc[l]], &host[o_sh[l]], eout[l], hw->enc_b[l], hw->enc_gamma[l], hw->enc_beta[l], hw->enc_mean[l],
                hw->enc_var[l]);
    }
    o_fc1 = reserve((size_t)FN_LAT * FN_CODE);
    memcpy(&host[o_fc1], hw->enc_w[5], sizeof(float) * FN_LAT * FN_CODE);
    o_fc2 = reserve((size_t)FN_CODE * FN_CODE);
    memcpy(&host[o_fc2], hw->enc_w[6], sizeof(float) * FN_CODE * FN_CODE);
    o_fc2b = reserve(FN_CODE);
    memcpy(&host[o_fc2b], hw->enc_b[6], sizeof(float) * FN_CODE);
    // the folds' code rows side by side: shift[c][0:512] = code . W1[0:512] + b1, shift[c][512:1024] = code . W2[0:512] + b2
    o_shw = reserve((size_t)FN_CODE * 2 * FN_HID);
    o_shb = reserve(2 * FN_HID);
    for (int f = 0; f < 2; ++f) {
        const float *w = hw->dec_w[3 * f];
        for (int k = 0; k < FN_CODE; ++k)
            memcpy(&host[o_shw + (size_t)k * 2 * FN_HID + f * FN_HID], w + (size_t)k * FN_HID, sizeof(float) * FN_HID);
        memcpy(&host[o_shb + f * FN_HID], hw->dec_b[3 * f], sizeof(float) * FN_HID);
    }
    o_lin = reserve(FN_GRID);
    for (int i = 0; i < FN_GRID; ++i) {     // np.linspace(-0.3, 0.3, 45): start + i * step, the last point exactly the stop
        const double step = 0.6 / (FN_GRID - 1);
        host[o_lin + i] = (float)(i == FN_GRID - 1 ? 0.3 : -0.3 + i * step);
    }
    o_wg = reserve(2 * FN_HID);
    memcpy(&host[o_wg], hw->dec_w[0] + (size_t)FN_CODE * FN_HID, sizeof(float) * 2 * FN_HID);
    o_wp = reserve(3 * FN_HID);
    memcpy(&host[o_wp], hw->dec_w[3] + (size_t)FN_CODE * FN_HID, sizeof(float) * 3 * FN_HID);
    o_pk2a = reserve((size_t)FN_HID * FN_HID);
    fn_pack(&host[o_pk2a], hw->dec_w[1], FN_HID, FN_HID);
    o_pk2b = reserve((size_t)FN_HID * FN_HID);
    fn_pack(&host[o_pk2b], hw->dec_w[4], FN_HID, FN_HID);
    o_b2a = reserve(FN_HID); memcpy(&host[o_b2a], hw->dec_b[1], sizeof(float) * FN_HID);
    o_b2b = reserve(FN_HID); memcpy(&host[o_b2b], hw->dec_b[4], sizeof(float) * FN_HID);
    o_w3a = reserve(FN_HID * 3); memcpy(&host[o_w3a], hw->dec_w[2], sizeof(float) * FN_HID * 3);
    o_w3b = reserve(FN_HID * 3); memcpy(&host[o_w3b], hw->dec_w[5], sizeof(float) * FN_HID * 3);
    o_b3a = reserve(3); memcpy(&host[o_b3a], hw->dec_b[2], sizeof(float) * 3);
    o_b3b = reserve(3); memcpy(&host[o_b3b], hw->dec_b[5], sizeof(float) * 3);

    geoadv_fold *m = new geoadv_fold();
    const size_t bytes = sizeof(float) * host.size();
    if (hipMalloc(&m->arena, bytes) != hipSuccess) {
        delete m;
        set_error("fold_create: hipMalloc of %zu bytes failed", bytes);
        return GEOADV_ENOMEM;
    }
    const hipError_t e = hipMemcpy(m->arena, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->arena);
        delete m;
        set_error("fold_create: upload failed: %s", hipGetErrorString(e));
        return GEOADV_EHIP;
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
FoldScratch carve_fold(void *base, int bc, int n) {
    FoldScratch s;
    char *p = static_cast<char *>(base);
    auto take = [&](size_t bytes) { char *q = p; p += fn_rup(bytes, 256); return q; };
    const size_t bn = (size_t)bc * n;
    s.kval = reinterpret_cast<float *>(take(sizeof(float) * bn * FN_K));
    s.kidx = reinterpret_cast<int *>(take(sizeof(int) * bn * FN_K));
    s.knn_bytes = geoadv_knn_workspace_bytes(bc, n, n, FN_K);
    s.knn_ws = take(s.knn_bytes);
    s.cnt = reinterpret_cast<int *>(take(sizeof(int) * bn));
    s.fill = reinterpret_cast<int *>(take(sizeof(int) * bn));
    s.off = reinterpret_cast<int *>(take(sizeof(int) * bn));
    s.deg = reinterpret_cast<int *>(take(sizeof(int) * bn));
    s.raw = reinterpret_cast<int *>(take(sizeof(int) * bn * 32));
    s.col = reinterpret_cast<int *>(take(sizeof(int) * bn * 32));
    s.cov = reinterpret_cast<float *>(take(sizeof(float) * bn * 9));
    s.cols = reinterpret_cast<int *>(take(sizeof(int) * 2 * bn * FN_NB));
    s.f1 = reinterpret_cast<float *>(take(sizeof(float) * bn * 64));
    s.f2 = reinterpret_cast<float *>(take(sizeof(float) * bn * 128));
    s.keys = reinterpret_cast<unsigned *>(take(sizeof(unsigned) * (size_t)bc * FN_LAT));
    s.h = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * FN_CODE));
    s.code = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * FN_CODE));
    s.shift = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * 2 * FN_HID));
    s.bytes = (size_t)(p - static_cast<char *>(base));
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
    void *aligned = reinterpret_cast<void *>(fn_rup(reinterpret_cast<size_t>(workspace), 256));
    const int bc = fold_chunk(b, n);
    const FoldScratch s = carve_fold(aligned, bc, n);
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
    void *aligned = reinterpret_cast<void *>(fn_rup(reinterpret_cast<size_t>(workspace), 256));
    const int bc = fold_chunk(b, n);
    const FoldScratch s = carve_fold(aligned, bc, n);
    const int tiles = cdiv(n, FN_ROWS);
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

        int slices = 1;    // small batches split conv5's 1024 columns over up to 4 workgroups per tile
        while (slices < 4 && (size_t)tiles * nbc * slices < 2 * kCUs) slices *= 2;
        FoldEncArgs ea{};
        ea.pc = x; ea.cov = s.cov; ea.w0 = fold->w0; ea.sc0 = fold->sc[0]; ea.sh0 = fold->sh[0];
        ea.l1 = PackedLayer{fold->pk[0], 64, 64}; ea.l2 = PackedLayer{fold->pk[1], 64, 64};
        ea.l3 = PackedLayer{fold->pk[2], 64, 128}; ea.l4 = PackedLayer{fold->pk[3], 128, FN_LAT};
        for (int l = 0; l < 5; ++l) { ea.sc[l] = fold->sc[l]; ea.sh[l] = fold->sh[l]; }
        ea.cols = s.cols; ea.f1 = s.f1; ea.f2 = s.f2; ea.keys = s.keys; ea.n = n; ea.bc = nbc; ea.slices = slices;
        hipLaunchKernelGGL(fold_enc1_kernel, dim3(tiles, nbc), dim3(FN_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(fold_pool_conv4_kernel, dim3(tiles, nbc), dim3(FN_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        GA_HIP(hipMemsetAsync(s.keys, 0, sizeof(unsigned) * (size_t)nbc * FN_LAT, st));
        hipLaunchKernelGGL(fold_pool_conv5_kernel, dim3(tiles, nbc, slices), dim3(FN_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();

        const int fy = cdiv(nbc, FN_FC_CLOUDS);
        float *cd = code ? code + (size_t)c0 * FN_CODE : s.code;
        FoldFcArgs fa{};
        fa.keys = s.keys; fa.w = fold->fc1; fa.sc = fold->sc[5]; fa.sh = fold->sh[5]; fa.out = s.h; fa.N = FN_CODE;
        fa.bc = nbc; fa.relu = 1;
        hipLaunchKernelGGL(fold_fc_kernel<FN_LAT>, dim3(FN_CODE / 64, fy), dim3(FN_FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        fa.keys = nullptr; fa.in = s.h; fa.w = fold->fc2; fa.sc = nullptr; fa.sh = fold->fc2b; fa.out = cd; fa.relu = 0;
        hipLaunchKernelGGL(fold_fc_kernel<FN_CODE>, dim3(FN_CODE / 64, fy), dim3(FN_FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        fa.in = cd; fa.w = fold->shw; fa.sh = fold->shb; fa.out = s.shift; fa.N = 2 * FN_HID;
        hipLaunchKernelGGL(fold_fc_kernel<FN_CODE>, dim3(2 * FN_HID / 64, fy), dim3(FN_FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();

        FoldDecArgs da{};
        da.lin = fold->lin; da.shift = s.shift; da.wg = fold->wg; da.wp = fold->wp;
        da.l2a = PackedLayer{fold->pk2a, FN_HID, FN_HID}; da.l2b = PackedLayer{fold->pk2b, FN_HID, FN_HID};
        da.b2a = fold->b2a; da.b2b = fold->b2b; da.w3a = fold->w3a; da.b3a = fold->b3a; da.w3b = fold->w3b; da.b3b = fold->b3b;
        da.p1 = p1 ? p1 + (size_t)c0 * FN_G2 * 3 : nullptr;
        da.recon = recon ? recon + (size_t)c0 * FN_G2 * 3 : nullptr;
        da.bc = nbc;
        if (recon || p1) {
            hipLaunchKernelGGL(fold_dec_kernel, dim3(cdiv(nbc * FN_G2, FN_ROWS)), dim3(FN_THREADS), FN_DEC_LDS, st, da);
            GA_LAUNCH_CHECK();
        }
    }
    return GEOADV_OK;
}
