// geoadv_cls_input_grad: the gradient of a logit loss with respect to the points, through the inference graph of
// geoadv_cls_forward (classifier.hip) -- both T-Nets included, T1 and T2 differentiated as functions of the input.  fp32.
//
// The rules are cls_train.hip's: the ReLU gradient is [output > 0]; a max pool sends its gradient to ONE row per (cloud,
// column), the lowest row among equal maxima; a pooled +0 passes nothing.
//
// Per chunk of at most CG_CHUNK clouds, all on the caller's stream:
//   geoadv_cls_forward                the forward itself: logits, the three pooled vectors, T1 / T2 folded (W1', W3')
//   winner<1|3> x 3                   the forward's chains once more, tile by tile and bit for bit; a value that equals the
//                                     finished pool takes an atomicMin on its row index (order of tiles does not matter)
//   sort (cloud, pool)                (row, column) of every live column sorted by row: the pool's distinct winner rows
//                                     ("slots"), ascending, each with its run of columns; writes `winners`
//   w3t                               W3'^T of every cloud as MFMA fragments
//   head_bwd<CLS>                     loss (float64, rounded once), dZ, fc3^T fc2^T fc1^T -> d pooled[2]
//   grad_init                         grad = 0 (NaN for a cloud whose label is out of range)
//   rows<3, pool 2>                   per 64 slots: gather the rows, recompute conv1' .. conv4 for the ReLU masks, the pooled
//                                     layer's transpose as a sum over each row's own columns (sparse: 1024 x 128 products
//                                     per cloud, not rows x 1024 x 128), conv4^T conv3'^T conv2^T conv1'^T on the MFMA;
//                                     grad[row] +=, and the tile's partial dW3' = h2^T g, dW1' = x^T g
//   head_bwd<T2>                      dW3' partials summed in tile order, dT2 = dW3' Wc3^T, the T-Net2 head's transpose
//   rows<3, pool 1>                   the same through tconv2^T tconv1^T conv2^T conv1'^T; partial dW1'
//   head_bwd<T1>                      dW1' partials summed (pool 2's tiles, then pool 1's), dT1 = dW1' Wc1^T, T-Net1 head
//   rows<1, pool 0>                   tconv2^T tconv1^T; grad[row] +=
// A row's gradient is ((0 + pool 2's) + pool 1's) + pool 0's: three launches in stream order, each touching a row at most
// once -- no float atomics anywhere, every sum in a fixed order, nothing depends on the batch.  A point that wins no column
// is never touched after grad_init.  The folded form is differentiated (x @ W1', h2 @ W3'), as the forward computes it.
#include "cls_model.h"
#include <cmath>

namespace geoadv {

constexpr int CG_CHUNK = 64;                        // clouds per pass (bounds the scratch)
constexpr int CG_MAX_TILES = PT_POOL / PT_ROWS;     // a pool has at most 1024 winner rows
constexpr unsigned CG_NOKEY = 0xffffffffu;

// ------------------------------------------------------------------------------------------------ winners
template <int NMID>
__global__ __launch_bounds__(PT_THREADS, 2) void cls_winner_kernel(ClsChainArgs A, int *win) {
    __shared__ __attribute__((aligned(16))) float bufA[PT_ROWS * PT_SA];
    __shared__ __attribute__((aligned(16))) float bufB[PT_ROWS * PT_SB];
    __shared__ float pts[PT_ROWS * 3];
    const int tile = blockIdx.x, cloud = blockIdx.y, slice = blockIdx.z;
    const int n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    load_points_conv1(A.x + ((size_t)cloud * n + n0) * 3, live, A.w0 + (size_t)cloud * A.w0_cloud_stride, A.sc0, A.sh0, pts, bufA);
    if (NMID == 1) {
        cls_mid<128>(bufA, PT_SA, A.mid[0], cloud, bufB, PT_SB);
    } else {
        cls_mid<64>(bufA, PT_SA, A.mid[0], cloud, bufB, PT_SB);
        __syncthreads();
        cls_mid<64>(bufB, PT_SB, A.mid[1], cloud, bufA, PT_SA);
        __syncthreads();
        cls_mid<128>(bufA, PT_SA, A.mid[2], cloud, bufB, PT_SB);
    }
    __syncthreads();
    pooled_wide_winners(bufB, PT_SB, A.wide.L, A.wide.scale, A.wide.shift, slice, A.slices, live, n0,
                        A.pooled + (size_t)cloud * PT_POOL, win + (size_t)cloud * PT_POOL,
                        [](float v) { return __float_as_uint(fmaxf(v, 0.f)); });
}

// ------------------------------------------------------------------------------------------------ sort
// One workgroup per (cloud, pool).  key = row << 10 | column for a column whose pooled value is > 0, CG_NOKEY otherwise;
// sorted ascending.  slot s = the s-th distinct row; its columns are skey[segstart[s] .. segstart[s + 1]).
struct ClsSortArgs {
    const unsigned *pooled;      // [3][nb][1024]
    const int *win;              // [3][nb][1024]
    unsigned *skey;              // [3][nb][1024]
    int *segstart;               // [3][nb][1025]
    int *cnt;                    // [3][nb]
    int *winners;                // user: [nb][3][1024] or null
    int nb, n;
};
__global__ __launch_bounds__(PT_THREADS) void cls_sort_kernel(ClsSortArgs S) {
    __shared__ unsigned keys[PT_POOL];
    __shared__ int scan[2][PT_POOL];
    const int c = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const size_t o = ((size_t)p * S.nb + c) * PT_POOL;
    for (int col = t; col < PT_POOL; col += PT_THREADS) {
        const int w = S.win[o + col];
        const bool on = S.pooled[o + col] != 0 && w >= 0 && w < S.n;
        keys[col] = on ? ((unsigned)w << 10 | (unsigned)col) : CG_NOKEY;
        if (S.winners) S.winners[((size_t)c * 3 + p) * PT_POOL + col] = on ? w : 0;
    }
    __syncthreads();
    for (int k = 2; k <= PT_POOL; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < PT_POOL; i += PT_THREADS) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const unsigned a = keys[i], b = keys[ixj];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    // a slot starts where the row changes
    for (int e = t; e < PT_POOL; e += PT_THREADS)
        scan[0][e] = keys[e] != CG_NOKEY && (e == 0 || (keys[e] >> 10) != (keys[e - 1] >> 10));
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < PT_POOL; d <<= 1) {
        for (int e = t; e < PT_POOL; e += PT_THREADS) scan[cur ^ 1][e] = scan[cur][e] + (e >= d ? scan[cur][e - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int *seg = S.segstart + ((size_t)p * S.nb + c) * (PT_POOL + 1);
    for (int e = t; e < PT_POOL; e += PT_THREADS) {
        S.skey[o + e] = keys[e];
        const bool valid = keys[e] != CG_NOKEY;
        if (valid && (e == 0 || (keys[e] >> 10) != (keys[e - 1] >> 10))) seg[scan[cur][e] - 1] = e;
        if (valid && (e == PT_POOL - 1 || keys[e + 1] == CG_NOKEY)) seg[scan[cur][e]] = e + 1;      // the end of the last run
    }
    if (t == 0) S.cnt[p * S.nb + c] = scan[cur][PT_POOL - 1];
}

// W3'^T of a cloud in the 32x32x2 fragment layout, from W3' in that layout (ae.h, K = N = 64)
__device__ __forceinline__ int frag64(int k, int nn) {
    return (((nn >> 5) * 8 + (k >> 3)) * 64 + ((k & 7) >> 2) * 32 + (nn & 31)) * 4 + (k & 3);
}
__global__ __launch_bounds__(PT_THREADS) void cls_w3t_kernel(const float *w3p, float *w3pt) {
    const size_t o = (size_t)blockIdx.x * 4096;
    for (int e = threadIdx.x; e < 4096; e += PT_THREADS) {
        const int k = e >> 6, nn = e & 63;
        w3pt[o + frag64(nn, k)] = w3p[o + frag64(k, nn)];
    }
}

__global__ void cls_grad_init_kernel(float *grad, const int *flag, int per_cloud, size_t total) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < total) grad[e] = flag[e / per_cloud] ? __uint_as_float(0x7fc00000u) : 0.f;
}

// ------------------------------------------------------------------------------------------------ heads, transposed
enum { CG_HEAD_T1 = 0, CG_HEAD_T2 = 1, CG_HEAD_CLS = 2 };
struct ClsHeadBwdArgs {
    const unsigned *pooled;                         // [nb][1024] float bits: the head's input
    const float *w1, *sc1, *sh1;                    // 1024 -> 512
    const float *w2, *sc2, *sh2;                    // 512 -> 256
    const float *w3;                                // 256 -> M
    int M;
    // CLS: dZ from the loss
    const float *logits;                            // [nb][M]
    const int *labels;                              // [nb]
    int loss_kind;
    float kappa;
    float *loss;                                    // [nb] or null
    int *flag;                                      // [nb]: the label is out of range
    // T2: dW3' partials [nb][16][4096] (tiles < ceil(cnt_a / 64)); T1: dW1' partials [nb][2][16][192] (cnt_a's tiles, then cnt_b's)
    const float *part;
    const int *cnt_a, *cnt_b;
    const float *fold_w;                            // T2: conv3 [64][64]; T1: conv1 [3][64]
    float *dp;                                      // [nb][1024]: d loss / d pooled
};

template <int MODE>
__global__ __launch_bounds__(PT_THREADS) void cls_head_bwd_kernel(ClsHeadBwdArgs H) {
    __shared__ float in[PT_POOL], h1[512], part[512], h2[256], g2[256];
    __shared__ float dout[MODE == CG_HEAD_T2 ? 4096 : (MODE == CG_HEAD_CLS ? 1024 : 16)];
    __shared__ float dw[MODE == CG_HEAD_T2 ? 4096 : (MODE == CG_HEAD_T1 ? 192 : 1)];
    __shared__ float fw[MODE == CG_HEAD_T2 ? 64 * 65 : 1];
    __shared__ double ex[MODE == CG_HEAD_CLS ? 1024 : 1];
    __shared__ double red[2];
    const int c = blockIdx.x, t = threadIdx.x, M = H.M;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    // the forward's head (cls_head_kernel), for the ReLU masks
    for (int k = t; k < PT_POOL; k += PT_THREADS) in[k] = __uint_as_float(H.pooled[(size_t)c * PT_POOL + k]);
    __syncthreads();
    {
        float a = 0.f;
        const float *w = H.w1 + t;
#pragma unroll 8
        for (int k = 0; k < PT_POOL; ++k) a = fmaf(in[k], w[(size_t)k * 512], a);
        h1[t] = fmaxf(a * H.sc1[t] + H.sh1[t], 0.f);
    }
    __syncthreads();
    {
        const int o = t & 255, k0 = (t >> 8) * 256;
        float a = 0.f;
        const float *w = H.w2 + o;
#pragma unroll 8
        for (int k = k0; k < k0 + 256; ++k) a = fmaf(h1[k], w[(size_t)k * 256], a);
        part[t] = a;
    }
    __syncthreads();
    if (t < 256) h2[t] = fmaxf((part[t] + part[t + 256]) * H.sc2[t] + H.sh2[t], 0.f);
    // d loss / d (the head's output)
    if (MODE == CG_HEAD_CLS) {
        const float *Z = H.logits + (size_t)c * M;
        const int y = H.labels[c];
        const bool bad = y < 0 || y >= M;
        const float qnan = __uint_as_float(0x7fc00000u);
        if (H.loss_kind == GEOADV_CLS_LOSS_XENT) {
            if (t == 0) {
                double m = Z[0];
                for (int o = 1; o < M; ++o) m = fmax(m, (double)Z[o]);
                red[0] = m;
            }
            __syncthreads();
            for (int o = t; o < M; o += PT_THREADS) ex[o] = exp((double)Z[o] - red[0]);
            __syncthreads();
            if (t == 0) {
                double s = 0.0;
                for (int o = 0; o < M; ++o) s += ex[o];
                red[1] = s;
                if (H.loss) H.loss[c] = bad ? qnan : (float)(log(s) - ((double)Z[y] - red[0]));
            }
            __syncthreads();
            for (int o = t; o < M; o += PT_THREADS) dout[o] = bad ? qnan : (float)(ex[o] / red[1] - (o == y ? 1.0 : 0.0));
        } else {
            // Carlini-Wagner on the logits: m = the FIRST maximum over i != y, at j
            for (int o = t; o < M; o += PT_THREADS) dout[o] = bad ? qnan : 0.f;
            __syncthreads();
            if (t == 0) {
                if (bad) {
                    if (H.loss) H.loss[c] = qnan;
                } else {
                    int j = -1;
                    float m = 0.f;
                    for (int o = 0; o < M; ++o)
                        if (o != y && (j < 0 || Z[o] > m)) { j = o; m = Z[o]; }
                    const bool targeted = H.loss_kind == GEOADV_CLS_LOSS_CW_TARGETED;
                    const double diff = targeted ? (double)m - (double)Z[y] : (double)Z[y] - (double)m;
                    const double floor_ = -(double)H.kappa;
                    if (H.loss) H.loss[c] = (float)(diff > floor_ ? diff : floor_);
                    if (diff > floor_) {
                        dout[j] = targeted ? 1.f : -1.f;
                        dout[y] = targeted ? -1.f : 1.f;
                    }
                }
            }
        }
        if (t == 0) H.flag[c] = bad;
    } else if (MODE == CG_HEAD_T2) {
        const int tiles = (H.cnt_a[c] + PT_ROWS - 1) / PT_ROWS;
        const float *P = H.part + (size_t)c * CG_MAX_TILES * 4096;
        for (int e = t; e < 4096; e += PT_THREADS) {
            float a = 0.f;
            for (int q = 0; q < tiles; ++q) a += P[(size_t)q * 4096 + e];
            dw[e] = a;
            fw[(e >> 6) * 65 + (e & 63)] = H.fold_w[e];
        }
        __syncthreads();
        // W3'[k][nn] = sum_j T2[k][j] Wc3[j][nn]  =>  dT2[k][j] = sum_nn dW3'[k][nn] Wc3[j][nn]
        for (int e = t; e < 4096; e += PT_THREADS) {
            const int k = e >> 6, j = e & 63;
            float a = 0.f;
            for (int nn = 0; nn < 64; ++nn) a = fmaf(dw[64 * k + nn], fw[65 * j + nn], a);
            dout[e] = a;
        }
    } else {
        const int ta = (H.cnt_a[c] + PT_ROWS - 1) / PT_ROWS, tb = (H.cnt_b[c] + PT_ROWS - 1) / PT_ROWS;
        const float *P = H.part + (size_t)c * 2 * CG_MAX_TILES * 192;
        if (t < 192) {
            float a = 0.f;
            for (int q = 0; q < ta; ++q) a += P[(size_t)q * 192 + t];
            for (int q = 0; q < tb; ++q) a += P[(size_t)(CG_MAX_TILES + q) * 192 + t];
            dw[t] = a;
        }
        __syncthreads();
        if (t < 9) {
            const int k = t / 3, j = t - 3 * k;
            float a = 0.f;
            for (int nn = 0; nn < 64; ++nn) a = fmaf(dw[64 * k + nn], H.fold_w[64 * j + nn], a);
            dout[t] = a;
        }
    }
    __syncthreads();
    // the three layers transposed: a wave per input, its lanes over the outputs, summed in wave_sum's fixed order
    for (int k = wave; k < 256; k += PT_THREADS / 64) {
        const float *w = H.w3 + (size_t)k * M;
        float a = 0.f;
        for (int o = lane; o < M; o += 64) a = fmaf(dout[o], w[o], a);
        a = wave_sum(a);
        if (lane == 0) g2[k] = h2[k] > 0.f ? a * H.sc2[k] : 0.f;
    }
    __syncthreads();
    for (int j = wave; j < 512; j += PT_THREADS / 64) {
        const float *w = H.w2 + (size_t)j * 256;
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) a = fmaf(g2[lane + 64 * q], w[lane + 64 * q], a);
        a = wave_sum(a);
        if (lane == 0) part[j] = h1[j] > 0.f ? a * H.sc1[j] : 0.f;
    }
    __syncthreads();
    for (int i = wave; i < PT_POOL; i += PT_THREADS / 64) {
        const float *w = H.w1 + (size_t)i * 512;
        float a = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) a = fmaf(part[lane + 64 * q], w[lane + 64 * q], a);
        a = wave_sum(a);
        if (lane == 0) H.dp[(size_t)c * PT_POOL + i] = a;
    }
}

// ------------------------------------------------------------------------------------------------ winner rows, transposed
struct ClsRowsArgs {
    const float *x;                                 // [nb][n][3]
    int n;
    const float *w0; int w0_cloud_stride;           // forward layer 0 [3][64]
    const float *sc0, *sh0;
    ClsLayerDev mid[3];                             // the forward's narrow layers
    const float *mid_t[3]; int mid_t_stride[3];     // their transposes as fragments
    const float *wide_t, *wide_scale;               // the pooled layer: W^T [1024][128], its batch-norm scale
    const float *dp;                                // [nb][1024]
    const unsigned *skey;                           // [nb][1024]
    const int *segstart;                            // [nb][1025]
    const int *cnt;                                 // [nb]
    float *grad;                                    // [nb][n][3]
    float *dw_mid1;                                 // partial d(mid[1]'s weights) [nb][16][4096], or null
    float *dw0;                                     // partial d(w0) [nb][2][16][192] at this pool's half, or null
};

// out[64][64] = mask(out) * ((in @ W^T) * scale): a narrow layer's transpose, the ReLU mask taken from the forward
// activation that `out` holds and replaced by the gradient of the layer's pre-activation input
template <int K>
__device__ __forceinline__ void cls_mid_t(const float *in, int s_in, const float *wt, float *out, const float *scale) {
    layer_gemm<PT_ROWS, 64, 1>(in, s_in, PackedLayer{wt, K, 64}, nullptr, [&](int row, int col, float a) {
        float *o = out + row * PT_SA + col;
        *o = *o > 0.f ? a * scale[col] : 0.f;
    });
}

template <int NMID>
__global__ __launch_bounds__(PT_THREADS) void cls_rows_kernel(ClsRowsArgs A) {
    __shared__ __attribute__((aligned(16))) float X[PT_ROWS * PT_SA], Y[NMID == 3 ? PT_ROWS * PT_SA : 4], V[NMID == 3 ? PT_ROWS * PT_SA : 4];
    __shared__ __attribute__((aligned(16))) float Z[PT_ROWS * PT_SB];
    __shared__ float pts[PT_ROWS * 3];
    __shared__ int rows[PT_ROWS], seg[PT_ROWS + 1];
    const int tile = blockIdx.x, cloud = blockIdx.y, t = threadIdx.x;
    const int cnt = A.cnt[cloud], slot0 = tile * PT_ROWS;
    if (slot0 >= cnt) return;
    const int live = cnt - slot0 < PT_ROWS ? cnt - slot0 : PT_ROWS;
    const unsigned *skey = A.skey + (size_t)cloud * PT_POOL;
    if (t <= live) {
        const int s = A.segstart[(size_t)cloud * (PT_POOL + 1) + slot0 + t];
        seg[t] = s;
        if (t < live) rows[t] = (int)(skey[s] >> 10);
    }
    __syncthreads();
    const float *xc = A.x + (size_t)cloud * A.n * 3;
    gather_points_conv1(xc, rows, live, A.w0 + (size_t)cloud * A.w0_cloud_stride, A.sc0, A.sh0, pts, X);
    if (NMID == 1) {
        cls_mid<128>(X, PT_SA, A.mid[0], cloud, Z, PT_SB);
    } else {
        cls_mid<64>(X, PT_SA, A.mid[0], cloud, Y, PT_SA);
        __syncthreads();
        cls_mid<64>(Y, PT_SA, A.mid[1], cloud, V, PT_SA);
        __syncthreads();
        cls_mid<128>(V, PT_SA, A.mid[2], cloud, Z, PT_SB);
    }
    __syncthreads();
    // the pooled layer's transpose: slot s takes dp * scale of ITS columns only, in column order
    {
        const int k = t & 127;
        const float *dp = A.dp + (size_t)cloud * PT_POOL;
        const float sck = A.mid[NMID - 1].scale[k];
        for (int s = t >> 7; s < PT_ROWS; s += PT_THREADS / 128) {
            float a = 0.f;
            if (s < live)
                for (int e = seg[s]; e < seg[s + 1]; ++e) {
                    const int col = (int)(skey[e] & 1023u);
                    a = fmaf(dp[col] * A.wide_scale[col], A.wide_t[(size_t)col * 128 + k], a);
                }
            float *z = Z + s * PT_SB + k;
            *z = (s < live && *z > 0.f) ? a * sck : 0.f;
        }
    }
    __syncthreads();
    if (NMID == 3) {
        cls_mid_t<128>(Z, PT_SB, A.mid_t[2] + (size_t)cloud * A.mid_t_stride[2], V, A.mid[1].scale);
        __syncthreads();
        if (A.dw_mid1) {   // d(mid[1]'s weights)[k][nn] = sum_rows Y[row][k] V[row][nn]
            float *P = A.dw_mid1 + ((size_t)cloud * CG_MAX_TILES + tile) * 4096;
            for (int e = t; e < 4096; e += PT_THREADS) {
                const int k = e >> 6, nn = e & 63;
                float a = 0.f;
                for (int r = 0; r < PT_ROWS; ++r) a = fmaf(Y[r * PT_SA + k], V[r * PT_SA + nn], a);
                P[e] = a;
            }
            __syncthreads();
        }
        cls_mid_t<64>(V, PT_SA, A.mid_t[1] + (size_t)cloud * A.mid_t_stride[1], Y, A.mid[0].scale);
        __syncthreads();
        cls_mid_t<64>(Y, PT_SA, A.mid_t[0] + (size_t)cloud * A.mid_t_stride[0], X, A.sc0);
    } else {
        cls_mid_t<128>(Z, PT_SB, A.mid_t[0] + (size_t)cloud * A.mid_t_stride[0], X, A.sc0);
    }
    __syncthreads();
    // layer 0 transposed (fan-in 3, VALU): d x[row][d] = sum_c X[row][c] w0[d][c];  d w0[d][c] = sum_rows x[row][d] X[row][c]
    const float *w0 = A.w0 + (size_t)cloud * A.w0_cloud_stride;
    if (t < 3 * PT_ROWS) {
        const int s = t / 3, d = t - 3 * s;
        if (s < live) {
            float a = 0.f;
            for (int c = 0; c < 64; ++c) a = fmaf(X[s * PT_SA + c], w0[64 * d + c], a);
            A.grad[((size_t)cloud * A.n + rows[s]) * 3 + d] += a;
        }
    } else if (t < 6 * PT_ROWS && A.dw0) {
        const int e = t - 3 * PT_ROWS, d = e >> 6, c = e & 63;
        float a = 0.f;
        for (int r = 0; r < PT_ROWS; ++r) a = fmaf(pts[3 * r + d], X[r * PT_SA + c], a);
        A.dw0[((size_t)cloud * 2 * CG_MAX_TILES + tile) * 192 + e] = a;
    }
}

}  // namespace geoadv

using namespace geoadv;

namespace {
struct GradScratch {
    void *fwd;               // geoadv_cls_forward's own workspace
    float *logits;           // [nb][C] when the caller wants none
    int *labels;             // [nb] arg-max of the forward (unused)
    int *win;                // [3][nb][1024]
    unsigned *skey;          // [3][nb][1024]
    int *segstart;           // [3][nb][1025]
    int *cnt;                // [3][nb]
    int *flag;               // [nb]
    float *dp;               // [nb][1024]
    float *w3pt;             // [nb][4096]
    float *dw3;              // [nb][16][4096]
    float *dw1;              // [nb][2][16][192]
    size_t bytes;
};
GradScratch carve_grad(void *workspace, const geoadv_cls *cls, int nb, int n) {
    GradScratch s;
    Carver cv(workspace);
    s.fwd = cv.take<char>(geoadv_cls_workspace_bytes(cls, nb, n));
    s.logits = cv.take<float>((size_t)nb * cls->num_classes);
    s.labels = cv.take<int>(nb);
    s.win = cv.take<int>(3 * (size_t)nb * PT_POOL);
    s.skey = cv.take<unsigned>(3 * (size_t)nb * PT_POOL);
    s.segstart = cv.take<int>(3 * (size_t)nb * (PT_POOL + 1));
    s.cnt = cv.take<int>(3 * (size_t)nb);
    s.flag = cv.take<int>(nb);
    s.dp = cv.take<float>((size_t)nb * PT_POOL);
    s.w3pt = cv.take<float>((size_t)nb * 4096);
    s.dw3 = cv.take<float>((size_t)nb * CG_MAX_TILES * 4096);
    s.dw1 = cv.take<float>((size_t)nb * 2 * CG_MAX_TILES * 192);
    s.bytes = cv.bytes();
    return s;
}
ClsLayerDev layer_dev(const geoadv_cls *m, int l, int K, int N) {
    return ClsLayerDev{PackedLayer{m->packed[l], K, N}, m->scale[l], m->shift[l], 0};
}
}  // namespace

extern "C" size_t geoadv_cls_input_grad_workspace_bytes(const geoadv_cls *cls, int b, int n) {
    if (!cls || b <= 0) return 256;
    return carve_grad(nullptr, cls, std::min(b, CG_CHUNK), n).bytes + 256;
}

extern "C" int geoadv_cls_input_grad(const geoadv_cls *cls, int b, int n, const float *pc, const int *labels, int loss_kind,
                                     float kappa, float *loss, float *logits, int *winners, float *grad, void *ws, void *stream) {
    GA_REQUIRE(cls, "cls_input_grad: null handle");
    GA_REQUIRE(b >= 1, "cls_input_grad: batch %d must be >= 1", b);
    GA_REQUIRE(n >= 1 && n <= 16384, "cls_input_grad: n %d out of range [1, 16384]", n);
    GA_REQUIRE(pc && labels && grad && ws, "cls_input_grad: null points, labels, gradient or workspace");
    GA_REQUIRE(loss_kind == GEOADV_CLS_LOSS_XENT || loss_kind == GEOADV_CLS_LOSS_CW_TARGETED || loss_kind == GEOADV_CLS_LOSS_CW_UNTARGETED,
               "cls_input_grad: unknown loss_kind %d", loss_kind);
    GA_REQUIRE(std::isfinite(kappa) && kappa >= 0.f, "cls_input_grad: kappa must be finite and >= 0");
    const int C = cls->num_classes;
    GA_REQUIRE(loss_kind == GEOADV_CLS_LOSS_XENT || C >= 2, "cls_input_grad: the CW losses need at least 2 classes");
    hipStream_t st = as_stream(stream);
    const int tiles = cdiv(n, PT_ROWS);
    const int row_tiles = std::min(tiles, CG_MAX_TILES);
    const int bc = std::min(b, CG_CHUNK);

    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nb = std::min(bc, b - c0);
        const GradScratch g = carve_grad(ws, cls, nb, n);
        const float *x = pc + (size_t)c0 * n * 3;
        float *lg = logits ? logits + (size_t)c0 * C : g.logits;
        float *gr = grad + (size_t)c0 * n * 3;
        if (int rc = geoadv_cls_forward(cls, nb, n, x, lg, g.labels, nullptr, nullptr, g.fwd, stream)) return rc;
        const ClsScratch s = carve_cls(g.fwd, nb);                       // what the forward left: pooled bits, W1', W3'
        const int slices = pooled_slices(tiles, nb);
        const dim3 grid(tiles, nb, slices), rgrid(row_tiles, nb);
        const size_t pool = (size_t)nb * PT_POOL, segs = (size_t)nb * (PT_POOL + 1);

        // the three chains as the forward launched them
        ClsChainArgs ch[3] = {};
        for (int p = 0; p < 3; ++p) {
            ch[p].x = x; ch[p].n = n; ch[p].slices = slices;
            ch[p].pooled = s.pooled + p * pool;
        }
        ch[0].w0 = cls->raw[T1C1]; ch[0].w0_cloud_stride = 0; ch[0].sc0 = cls->scale[T1C1]; ch[0].sh0 = cls->shift[T1C1];
        ch[0].mid[0] = layer_dev(cls, T1C2, 64, 128);
        ch[0].wide = layer_dev(cls, T1C3, 128, 1024);
        for (int p = 1; p < 3; ++p) {
            ch[p].w0 = s.w1f; ch[p].w0_cloud_stride = 192; ch[p].sc0 = cls->scale[C1]; ch[p].sh0 = cls->shift[C1];
            ch[p].mid[0] = layer_dev(cls, C2, 64, 64);
        }
        ch[1].mid[1] = layer_dev(cls, T2C1, 64, 64);
        ch[1].mid[2] = layer_dev(cls, T2C2, 64, 128);
        ch[1].wide = layer_dev(cls, T2C3, 128, 1024);
        ch[2].mid[1] = ClsLayerDev{PackedLayer{s.w3p, 64, 64}, cls->scale[C3], cls->shift[C3], 4096};
        ch[2].mid[2] = layer_dev(cls, C4, 64, 128);
        ch[2].wide = layer_dev(cls, C5, 128, 1024);

        GA_HIP(hipMemsetAsync(g.win, 0x7f, sizeof(int) * 3 * pool, st));
        hipLaunchKernelGGL(cls_winner_kernel<1>, grid, dim3(PT_THREADS), 0, st, ch[0], g.win);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(cls_winner_kernel<3>, grid, dim3(PT_THREADS), 0, st, ch[1], g.win + pool);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(cls_winner_kernel<3>, grid, dim3(PT_THREADS), 0, st, ch[2], g.win + 2 * pool);
        GA_LAUNCH_CHECK();
        ClsSortArgs sa{s.pooled, g.win, g.skey, g.segstart, g.cnt, winners ? winners + (size_t)c0 * 3 * PT_POOL : nullptr, nb, n};
        hipLaunchKernelGGL(cls_sort_kernel, dim3(nb, 3), dim3(PT_THREADS), 0, st, sa);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(cls_w3t_kernel, dim3(nb), dim3(PT_THREADS), 0, st, s.w3p, g.w3pt);
        GA_LAUNCH_CHECK();

        // classifier head, pool 2
        ClsHeadBwdArgs ha{};
        ha.dp = g.dp;
        ha.pooled = s.pooled + 2 * pool;
        ha.w1 = cls->raw[F1]; ha.sc1 = cls->scale[F1]; ha.sh1 = cls->shift[F1];
        ha.w2 = cls->raw[F2]; ha.sc2 = cls->scale[F2]; ha.sh2 = cls->shift[F2];
        ha.w3 = cls->raw[F3]; ha.M = C;
        ha.logits = lg; ha.labels = labels + c0; ha.loss_kind = loss_kind; ha.kappa = kappa;
        ha.loss = loss ? loss + c0 : nullptr; ha.flag = g.flag;
        hipLaunchKernelGGL(cls_head_bwd_kernel<CG_HEAD_CLS>, dim3(nb), dim3(PT_THREADS), 0, st, ha);
        GA_LAUNCH_CHECK();
        const size_t total = (size_t)nb * n * 3;
        hipLaunchKernelGGL(cls_grad_init_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gr, g.flag, n * 3, total);
        GA_LAUNCH_CHECK();

        ClsRowsArgs ra{};
        ra.x = x; ra.n = n; ra.dp = g.dp; ra.grad = gr;
        auto rows_of = [&](int p) {
            ra.w0 = ch[p].w0; ra.w0_cloud_stride = ch[p].w0_cloud_stride; ra.sc0 = ch[p].sc0; ra.sh0 = ch[p].sh0;
            for (int i = 0; i < 3; ++i) ra.mid[i] = ch[p].mid[i];
            ra.skey = g.skey + p * pool; ra.segstart = g.segstart + p * segs; ra.cnt = g.cnt + p * nb;
        };
        rows_of(2);
        ra.mid_t[0] = cls->packed_t[C2]; ra.mid_t[1] = g.w3pt; ra.mid_t[2] = cls->packed_t[C4];
        ra.mid_t_stride[0] = 0; ra.mid_t_stride[1] = 4096; ra.mid_t_stride[2] = 0;
        ra.wide_t = cls->raw_t[C5]; ra.wide_scale = cls->scale[C5];
        ra.dw_mid1 = g.dw3; ra.dw0 = g.dw1;
        hipLaunchKernelGGL(cls_rows_kernel<3>, rgrid, dim3(PT_THREADS), 0, st, ra);
        GA_LAUNCH_CHECK();

        // T-Net2 head, pool 1
        ha.pooled = s.pooled + pool;
        ha.w1 = cls->raw[T2F1]; ha.sc1 = cls->scale[T2F1]; ha.sh1 = cls->shift[T2F1];
        ha.w2 = cls->raw[T2F2]; ha.sc2 = cls->scale[T2F2]; ha.sh2 = cls->shift[T2F2];
        ha.w3 = cls->raw[T2FEAT]; ha.M = 4096;
        ha.part = g.dw3; ha.cnt_a = g.cnt + 2 * nb; ha.cnt_b = nullptr; ha.fold_w = cls->raw[C3];
        hipLaunchKernelGGL(cls_head_bwd_kernel<CG_HEAD_T2>, dim3(nb), dim3(PT_THREADS), 0, st, ha);
        GA_LAUNCH_CHECK();
        rows_of(1);
        ra.mid_t[1] = cls->packed_t[T2C1]; ra.mid_t[2] = cls->packed_t[T2C2];
        ra.mid_t_stride[1] = 0;
        ra.wide_t = cls->raw_t[T2C3]; ra.wide_scale = cls->scale[T2C3];
        ra.dw_mid1 = nullptr; ra.dw0 = g.dw1 + (size_t)CG_MAX_TILES * 192;
        hipLaunchKernelGGL(cls_rows_kernel<3>, rgrid, dim3(PT_THREADS), 0, st, ra);
        GA_LAUNCH_CHECK();

        // T-Net1 head, pool 0
        ha.pooled = s.pooled;
        ha.w1 = cls->raw[T1F1]; ha.sc1 = cls->scale[T1F1]; ha.sh1 = cls->shift[T1F1];
        ha.w2 = cls->raw[T1F2]; ha.sc2 = cls->scale[T1F2]; ha.sh2 = cls->shift[T1F2];
        ha.w3 = cls->raw[T1XYZ]; ha.M = 9;
        ha.part = g.dw1; ha.cnt_a = g.cnt + 2 * nb; ha.cnt_b = g.cnt + nb; ha.fold_w = cls->raw[C1];
        hipLaunchKernelGGL(cls_head_bwd_kernel<CG_HEAD_T1>, dim3(nb), dim3(PT_THREADS), 0, st, ha);
        GA_LAUNCH_CHECK();
        rows_of(0);
        ra.mid_t[0] = cls->packed_t[T1C2];
        ra.wide_t = cls->raw_t[T1C3]; ra.wide_scale = cls->scale[T1C3];
        ra.dw_mid1 = nullptr; ra.dw0 = nullptr;
        hipLaunchKernelGGL(cls_rows_kernel<1>, rgrid, dim3(PT_THREADS), 0, st, ra);
        GA_LAUNCH_CHECK();
    }
    return GEOADV_OK;
}
