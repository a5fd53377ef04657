// geoadv_atlas_trainer: one TRAINING step of the AtlasNet point-cloud auto-encoder (transfer/atlasnet/training/trainer.py
// train_iteration: EncoderDecoder.forward(x, train=True), fuse_primitives, chamfer_loss, backward, torch.optim.Adam.step) on
// gfx950, fp32 in and out.
//
// Model (model/model_blocks.py): PointNet encoder conv1 3 -> 64, conv2 64 -> 128 (BN ReLU), conv3 128 -> 1024 (BN, NO
// ReLU), max over points, lin1, lin2 1024 -> 1024 (BN ReLU, statistics over the batch's clouds) = the latent z.  nb
// independent Mapping2Dto3D decoders: pre1 = conv1(template) + z (broadcast over the primitive's p points), BN ReLU, conv2
// 1024 -> 512 BN ReLU, num_layers x (512 -> 512 BN ReLU), last_conv 512 -> 3.  A decoder BN takes its statistics per
// primitive over batch * p rows.  decoder_bn = 0 (remove_all_batchNorms): the decoder's norms are identities, inv 1 shift 0.
// BatchNorm1d in train mode: eps 1e-5, the BIASED batch variance normalises, running = 0.9 running + 0.1 batch with the
// UNBIASED variance.  The reconstruction is fused primitive-major: recon[b][q * p + j] = decoder q's point j of cloud b.
// Loss = sum(dist1) / (B n) + sum(dist2) / (B nb p) (geoadv_nn_distance / geoadv_nn_distance_grad).
//
// TEMPLATE POINTS of a step (given_template = 0): coordinate d (0, 1) of point j of primitive q at the model's training
// step number T (num_batches_tracked before the step; a new optimizer does not reset it) is
//     key = mix(mix(mix(seed + G) ^ T) ^ (q << 32 | j));   r = mix(key + (d + 1) * G);   value = (r >> 40) * 2^-24
// with mix = splitmix64's finaliser (z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb;
// z ^= z >> 31), G = 0x9e3779b97f4a7c15, all in 64-bit wrap-around arithmetic.  r >> 40 has 24 bits, so the product is exact
// in fp32 and lies in [0, 1): host and device agree to the bit.
//
// FORM: the direct one, as fold_train.hip, on the batch-norm, global-max, loss, Adam and running-statistics kernels of
// train_bn.h (what is stored, what is recomputed and why lin1 / lin2's backward is in double: there).  STORED besides: the
// post-ReLU output of every BN layer.  The decoder's first layer is never materialised before its BN: pre1 =
// t1[q][j] + z[b] with t1 = conv1(template) [nb][p][1024]; over the product grid (b, j) its mean is mean_j t1 + mean_b z and
// its variance var_j t1 + var_b z (the cross term vanishes), the backward rebuilds it from t1 and z (train_bn.h: RB), and
// its gradient reduces to dz[b] = sum_q sum_j and dt1[q][j] = sum_b, each in ascending order.
//
// GEMMs on v_mfma_f32_32x32x2_f32.  The decoder's products (batched over the primitives) run on at_gemm_kernel: a 128 x 128
// tile per workgroup (each wave 64 x 64 = four accumulator blocks), operands double-buffered in LDS (the next K slice is
// loaded into registers while the current one is multiplied), the per-primitive bias in the epilogue.  Products whose grid
// of 128-tiles would leave most of the device idle, and all of the encoder's, go through ct_launch_gemm and its fixed-order
// split-K (train_tile.h).  No float atomics anywhere: two steps from the same state are bitwise identical.
//
// Adam (torch.optim.Adam, lr, betas .9 / .999, eps 1e-8, no weight decay): m += (g - m) * 0.1; v = 0.999 v + 0.001 g g;
// p -= lr / (1 - 0.9^t) * m / (sqrt(v) / sqrt(1 - 0.999^t) + eps), t = steps this optimizer has taken including this one.
#include "train_bn.h"

namespace geoadv {

constexpr float AT_EPS = 1e-5f;
constexpr int AT_LAT = 1024, AT_HID = 512;
constexpr long long AT_MAX_ROWS = 1ll << 17, AT_MAX_DEC_ROWS = 1ll << 18;

// ---- the decoder's GEMM ------------------------------------------------------------------------------------
constexpr int AG_T = 128, AG_KT = 16, AG_LDS = AG_T + 4;
// C[z] = sum_k A(i, k) B(k, j) + bias[z][j]; strides as GemmArgs.
struct BGemm {
    const float *A; long long sAi, sAk, sAz;
    const float *B; long long sBk, sBj, sBz;
    float *C; long long ldc, sCz;
    const float *bias; long long sBiasZ;
    int M, N, K;
};

__global__ __launch_bounds__(256) void at_gemm_kernel(BGemm g) {
    __shared__ float As[2][AG_KT][AG_LDS], Bs[2][AG_KT][AG_LDS];
    const int z = blockIdx.z, i0 = blockIdx.y * AG_T, j0 = blockIdx.x * AG_T;
    const float *A = g.A + z * g.sAz, *B = g.B + z * g.sBz;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, h = lane >> 5, li = lane & 31;
    const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
    const bool a_kfast = g.sAk == 1, b_jfast = g.sBj == 1;
    constexpr int Q = AG_KT * AG_T / 256;
    f32x16 acc[2][2] = {};
    float ra[Q], rb[Q];
#define AG_LOAD(K0)                                                                                                   \
    _Pragma("unroll") for (int q = 0; q < Q; ++q) {                                                                   \
        const int e = t + q * 256;                                                                                    \
        int r, k, c, kk;                                                                                              \
        if (a_kfast) { r = e / AG_KT; k = e % AG_KT; } else { k = e / AG_T; r = e % AG_T; }                           \
        if (b_jfast) { kk = e / AG_T; c = e % AG_T; } else { c = e / AG_KT; kk = e % AG_KT; }                         \
        const int gi = i0 + r, gk = (K0) + k, gj = j0 + c, gk2 = (K0) + kk;                                           \
        ra[q] = (gi < g.M && gk < g.K) ? A[gi * g.sAi + gk * g.sAk] : 0.f;                                            \
        rb[q] = (gj < g.N && gk2 < g.K) ? B[gk2 * g.sBk + gj * g.sBj] : 0.f;                                          \
    }
#define AG_STORE(BUF)                                                                                                 \
    _Pragma("unroll") for (int q = 0; q < Q; ++q) {                                                                   \
        const int e = t + q * 256;                                                                                    \
        int r, k, c, kk;                                                                                              \
        if (a_kfast) { r = e / AG_KT; k = e % AG_KT; } else { k = e / AG_T; r = e % AG_T; }                           \
        if (b_jfast) { kk = e / AG_T; c = e % AG_T; } else { c = e / AG_KT; kk = e % AG_KT; }                         \
        As[BUF][k][r] = ra[q];                                                                                        \
        Bs[BUF][kk][c] = rb[q];                                                                                       \
    }
    AG_LOAD(0)
    AG_STORE(0)
    __syncthreads();
    int cur = 0;
    for (int k0 = 0; k0 < g.K; k0 += AG_KT) {
        const bool more = k0 + AG_KT < g.K;
        if (more) { AG_LOAD(k0 + AG_KT) }
#pragma unroll
        for (int kk = 0; kk < AG_KT; kk += 2) {
            const float a0 = As[cur][kk + h][wr + li], a1 = As[cur][kk + h][wr + 32 + li];
            const float b0 = Bs[cur][kk + h][wc + li], b1 = Bs[cur][kk + h][wc + 32 + li];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
        if (more) { AG_STORE(cur ^ 1) }
        __syncthreads();
        cur ^= 1;
    }
#undef AG_LOAD
#undef AG_STORE
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int col = j0 + wc + ni * 32 + li;
            if (col >= g.N) continue;
            const float bv = g.bias ? g.bias[z * g.sBiasZ + col] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = i0 + wr + mi * 32 + acc_row(r, h);
                if (row < g.M) g.C[z * g.sCz + (size_t)row * g.ldc + col] = acc[mi][ni][r] + bv;
            }
        }
}

// The one launch of at_gemm_kernel: the step (Run::gemm) and geoadv_train_gemm both go through it.
inline hipError_t at_launch_gemm(const BGemm &g, int batch, hipStream_t st) {
    hipLaunchKernelGGL(at_gemm_kernel, dim3(cdiv(g.N, AG_T), cdiv(g.M, AG_T), batch), dim3(256), 0, st, g);
    return hipGetLastError();
}

// The same product on ct_launch_gemm (train_tile.h): its one bias serves every group, so g.sBiasZ is not read.
inline hipError_t at_launch_splitk(const BGemm &b, int batch, float *partials, hipStream_t st) {
    GemmArgs g{};
    g.A = b.A; g.sAi = b.sAi; g.sAk = b.sAk; g.sAz = b.sAz;
    g.B = b.B; g.sBk = b.sBk; g.sBj = b.sBj; g.sBz = b.sBz;
    g.C = b.C; g.ldc = b.ldc; g.sCz = b.sCz; g.bias = b.bias;
    g.alpha = 1.f; g.M = b.M; g.N = b.N; g.K = b.K; g.batch = batch;
    return ct_launch_gemm(g, partials, st);
}

// The decoder's bn1: pre1 = t1[q][j] + z[b] over the grid (b, j): mean = mean_j t1 + mean_b z, var = var_j t1 + var_b z.
__global__ __launch_bounds__(256) void at_bn1_stats_kernel(const float *t1, const float *z, int p, int B, int C, int G, const float *gamma,
                                                           const float *beta, float *mean, float *var, float *inv, float *shift) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G * C) return;
    const int g = e / C, c = e - g * C;
    double mt = 0.0, vt = 0.0, mz = 0.0, vz = 0.0;
    for (int j = 0; j < p; ++j) mt += (double)t1[((size_t)g * p + j) * C + c];
    mt /= p;
    for (int j = 0; j < p; ++j) { const double d = (double)t1[((size_t)g * p + j) * C + c] - mt; vt += d * d; }
    vt /= p;
    for (int b = 0; b < B; ++b) mz += (double)z[(size_t)b * C + c];
    mz /= B;
    for (int b = 0; b < B; ++b) { const double d = (double)z[(size_t)b * C + c] - mz; vz += d * d; }
    vz /= B;
    const float mf = (float)(mt + mz), vf = (float)(vt + vz);
    const float iv = gamma[e] * (1.0f / sqrtf(vf + AT_EPS));
    mean[e] = mf; var[e] = vf; inv[e] = iv; shift[e] = beta[e] - mf * iv;
}

// t1[q][j][c] = b1[q][c] + tmpl[q][j][0] * W1[q][0][c] + tmpl[q][j][1] * W1[q][1][c] (two fmas in that order)
__global__ __launch_bounds__(256) void at_t1_kernel(const float *tmpl, const float *w, const float *b, int p, int total, float *t1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = e % AT_LAT, qj = e / AT_LAT, q = qj / p;
    float v = b[q * AT_LAT + c];
    v = fmaf(w[(q * 2 + 0) * AT_LAT + c], tmpl[qj * 2 + 0], v);
    v = fmaf(w[(q * 2 + 1) * AT_LAT + c], tmpl[qj * 2 + 1], v);
    t1[e] = v;
}

__global__ __launch_bounds__(256) void at_template_kernel(unsigned long long seed, unsigned long long tracked, int p, int total, float *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int d = e & 1, qj = e >> 1, q = qj / p, j = qj - q * p;
    const unsigned long long key = mix64(mix64(mix64(seed + kGolden64) ^ tracked) ^ (((unsigned long long)q << 32) | (unsigned)j));
    const unsigned long long r = mix64(key + (unsigned long long)(d + 1) * kGolden64);
    out[e] = (float)(unsigned)(r >> 40) * 0x1p-24f;
}

// last_conv: out[row][o] = sum_c h[row][c] W[q][c][o] + b[q][o], one wave per row, lanes over channels, fixed-order sum
__global__ __launch_bounds__(256) void at_last_fwd_kernel(const float *h, const float *w, const float *b, int Rp, int rows, float *out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int q = row / Rp;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < AT_HID / 64; ++i) {
        const int c = lane + 64 * i;
        const float v = h[(size_t)row * AT_HID + c];
        const float *wc = w + ((size_t)q * AT_HID + c) * 3;
        s0 = fmaf(v, wc[0], s0); s1 = fmaf(v, wc[1], s1); s2 = fmaf(v, wc[2], s2);
    }
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) {
        out[(size_t)row * 3 + 0] = s0 + b[q * 3 + 0];
        out[(size_t)row * 3 + 1] = s1 + b[q * 3 + 1];
        out[(size_t)row * 3 + 2] = s2 + b[q * 3 + 2];
    }
}

// fuse_primitives: FWD: fused[b][q * p + j] = prim[q][b * p + j]; else prim = fused (the gradient's way back)
template <bool FWD>
__global__ __launch_bounds__(256) void at_fuse_kernel(float *prim, float *fused, int B, int nb, int p, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int d = (int)(e % 3);
    const size_t r = e / 3;
    const int j = (int)(r % p), b = (int)(r / p % B), q = (int)(r / p / B);
    const size_t f = (((size_t)b * nb + q) * p + j) * 3 + d;
    if (FWD) fused[f] = prim[e]; else prim[e] = fused[f];
}

// d pre1 [nb][B * p][1024] -> dt1[q][j][c] = sum_b (ascending)
__global__ __launch_bounds__(256) void at_dt1_kernel(const float *d, int B, int p, size_t total, float *dt1) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % AT_LAT);
    const size_t qj = e / AT_LAT, q = qj / p, j = qj % p;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s += (double)d[((q * B + b) * p + j) * AT_LAT + c];
    dt1[e] = (float)s;
}

// dzq[q][b][c] = sum_j (ascending) d pre1[q][b * p + j][c]
__global__ __launch_bounds__(256) void at_dzq_kernel(const float *d, int p, size_t total, double *dzq) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % AT_LAT);
    const size_t qb = e / AT_LAT;
    double s = 0.0;
    for (int j = 0; j < p; ++j) s += (double)d[(qb * p + j) * AT_LAT + c];
    dzq[e] = s;
}

// dz[b][c] = sum_q (ascending) dzq[q][b][c]
__global__ __launch_bounds__(256) void at_dz_kernel(const double *dzq, int nb, int per, float *dz) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double s = 0.0;
    for (int q = 0; q < nb; ++q) s += dzq[(size_t)q * per + e];
    dz[e] = (float)s;
}

// The decoder's conv1: db[q][c] = sum_j dt1, dW[q][d][c] = sum_j tmpl[q][j][d] dt1[q][j][c]
__global__ __launch_bounds__(256) void at_conv1_grad_kernel(const float *dt1, const float *tmpl, int p, int G, float *dw, float *db) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G * AT_LAT) return;
    const int q = e / AT_LAT, c = e - q * AT_LAT;
    double s = 0.0, w0 = 0.0, w1 = 0.0;
    for (int j = 0; j < p; ++j) {
        const double v = (double)dt1[((size_t)q * p + j) * AT_LAT + c];
        s += v;
        w0 += v * (double)tmpl[((size_t)q * p + j) * 2 + 0];
        w1 += v * (double)tmpl[((size_t)q * p + j) * 2 + 1];
    }
    db[e] = (float)s;
    dw[(q * 2 + 0) * AT_LAT + c] = (float)w0;
    dw[(q * 2 + 1) * AT_LAT + c] = (float)w1;
}

}  // namespace geoadv

using namespace geoadv;

namespace {
// layers: the encoder's conv1, conv2, conv3, lin1, lin2, then the decoder's conv1, conv2, conv_list[0 .. L), last_conv
enum { E1 = 0, E2, E3, L1, L2, D0, D1, MAXL = 12 };
static_assert(MAXL <= TA_MAXL && GEOADV_ATLAS_STATE_BN_MEAN == TA_BAT_MEAN && GEOADV_ATLAS_STATE_BN_VAR == TA_BAT_VAR &&
              GEOADV_ATLAS_STATE_RUNNING_MEAN == TA_RUN_MEAN && GEOADV_ATLAS_STATE_RUNNING_VAR == TA_RUN_VAR &&
              GEOADV_ATLAS_STATE_BN_INV == TA_INV && GEOADV_ATLAS_STATE_BN_SHIFT == TA_SHIFT,
              "geoadv_atlas_trainer_state passes these to TrainArena::view as they are");
}  // namespace

struct geoadv_atlas_trainer : TrainArena {            // a layer's groups: 1 (encoder) or nb
    int B, n, R, nb, p, Rp, rows, m, L, dbn;          // Rp = B * p rows per primitive, rows = nb * Rp, m = nb * p
    float lr;
    long long step, tracked;
    unsigned long long seed;
    float *a[MAXL], *h[MAXL], *pooled, *t1, *dt1, *tmpl, *prim, *recon, *dprim, *drecon, *dx;
    int *arg, *i1, *i2;
    float *d1, *d2, *gd1, *gd2, *loss;
    float *Y, *Z, *T, *dz, *dsm1, *dsm2, *partials;
    double *dzq;
    double2 *part;
    bool bn_of(int l) const { return layer[l].bn; }
};

namespace {
struct Run : TrainRun {
    geoadv_atlas_trainer *t;

    int rows(int l) const { return t->layer[l].rows; }                             // per group

    // Batched over the layer's groups: C[z] = A[z] (M x K, strides) B[z] (K x N, strides) + bias[z].  The 128-tile kernel where
    // its grid fills the device, else ct_launch_gemm (split-K) -- which has one bias for all groups, so only without one.
    void gemm(const float *A, long long sAi, long long sAk, long long sAz, const float *Bm, long long sBk, long long sBj, long long sBz,
              float *Cm, long long ldc, long long sCz, const float *bias, long long sBiasZ, int M, int N, int K, int batch) {
        if (!ok()) return;
        const long long tiles = (long long)cdiv(M, AG_T) * cdiv(N, AG_T) * batch;
        const BGemm g{A, sAi, sAk, sAz, Bm, sBk, sBj, sBz, Cm, ldc, sCz, bias, sBiasZ, M, N, K};
        const bool tile = (bias && batch > 1) || (tiles >= kCUs && N >= 64);
        err = tile ? at_launch_gemm(g, batch, st) : at_launch_splitk(g, batch, t->partials, st);
    }
    // out[g] = in[g] @ W_l[g] + b_l[g]
    void linear_fwd(int l, const float *in, float *out) {
        const int M = rows(l), K = t->kin(l), N = t->kout(l), G = t->groups(l);
        gemm(in, K, 1, (long long)M * K, W(l), N, 1, (long long)K * N, out, N, (long long)M * N, t->params + t->o_b[l], N, M, N, K, G);
    }
    void bn_relu(int l, float *y) {
        const int Rg = rows(l), C = t->kout(l), G = t->groups(l);
        const size_t total = (size_t)G * Rg * C, o = t->o_mv[l];
        if (l == D0)
            launch(tb_bn_relu_kernel<true>, dim3(blocks_of(total)), dim3(256), t->t1, t->h[L2], total, Rg, C, t->p, t->inv + o, t->shift + o, y);
        else
            launch(tb_bn_relu_kernel<false>, dim3(blocks_of(total)), dim3(256), t->a[l], nullptr, total, Rg, C, t->p, t->inv + o, t->shift + o, y);
    }
    void bn_layer(int l, const float *in, float *y) {
        linear_fwd(l, in, t->a[l]);
        if (t->bn_of(l)) batch_stats(l, t->a[l]);
        if (y) bn_relu(l, y);
    }

    // ---- backward pieces ----
    // dW_l[g] = in[g]^T da[g]
    void weight_grad(int l, const float *in, const float *da) {
        const int M = rows(l), K = t->kin(l), N = t->kout(l), G = t->groups(l);
        gemm(in, 1, K, (long long)M * K, da, N, 1, (long long)M * N, t->grads + t->o_w[l], N, (long long)K * N, nullptr, 0, K, N, M, G);
    }
    // din[g] = da[g] W_l[g]^T
    void input_grad(int l, const float *da, float *din) {
        const int M = rows(l), K = t->kin(l), N = t->kout(l), G = t->groups(l);
        gemm(da, N, 1, (long long)M * N, W(l), 1, N, (long long)K * N, din, K, (long long)M * K, nullptr, 0, M, K, N, G);
    }
    void linear_bwd(int l, const float *in, const float *da, float *din) {
        weight_grad(l, in, da);
        bias_grad(l, da);
        if (din) input_grad(l, da, din);
    }
    // BN + ReLU backward of layer l, dense dy -> da (may alias dy).  The decoder's first layer rebuilds its activation.
    void bn_bwd(int l, const float *dy, float *da) {
        const int Rg = rows(l), C = t->kout(l), G = t->groups(l), p = t->p;
        const size_t o = t->o_mv[l], total = (size_t)G * Rg * C;
        const float *mean = t->bat_mean + o, *var = t->bat_var + o, *iv = t->inv + o, *sh = t->shift + o, *gam = t->params + t->o_g[l];
        float *dgam = t->grads + t->o_g[l], *dbeta = t->grads + t->o_be[l];
        const bool rb = l == D0;
        const float *a = rb ? t->t1 : t->a[l], *z = rb ? t->h[L2] : nullptr;
        const dim3 flat(blocks_of(total));
        if (!t->bn_of(l)) {
            launch(rb ? tb_bn_bwd_apply_kernel<true, false> : tb_bn_bwd_apply_kernel<false, false>, flat, dim3(256), dy, a, z, total, Rg, C, p, mean,
                   var, mean, iv, sh, mean, mean, AT_EPS, da);
            return;
        }
        if (l == L1 || l == L2) {
            launch(tb_bn_bwd_fc_kernel, dim3(cdiv(C, 256)), dim3(256), dy, t->a[l], Rg, C, gam, iv, sh, AT_EPS, dgam, dbeta, da);
            return;
        }
        const int rpc = rpc_of(Rg), chunks = cdiv(Rg, rpc);
        launch(rb ? tb_bn_bwd_part_kernel<true> : tb_bn_bwd_part_kernel<false>, dim3(cdiv(C, 64), chunks, G), dim3(256), dy, a, z, Rg, C, p, rpc,
               mean, var, iv, sh, AT_EPS, t->part);
        launch(tb_bn_bwd_final_kernel, dim3(cdiv(G * C, 256)), dim3(256), t->part, chunks, C, G, 1.0 / Rg, dgam, dbeta, t->m1 + o, t->m2 + o);
        launch(rb ? tb_bn_bwd_apply_kernel<true, true> : tb_bn_bwd_apply_kernel<false, true>, flat, dim3(256), dy, a, z, total, Rg, C, p, mean, var,
               gam, iv, sh, t->m1 + o, t->m2 + o, AT_EPS, da);
    }
    // conv3's BN: dpool [B][1024] at the maximum's rows -> da [R][1024]
    void bn_bwd_gmax(const float *dpool, float *da) {
        const int l = E3, C = AT_LAT;
        const size_t o = t->o_mv[l], total = (size_t)t->R * C;
        const float *mean = t->bat_mean + o, *var = t->bat_var + o;
        launch(tb_bn_bwd_gmax_part_kernel, dim3(cdiv(C, 256)), dim3(256), dpool, t->arg, t->a[l], t->B, t->n, C, mean, var, AT_EPS, t->part);
        launch(tb_bn_bwd_final_kernel, dim3(cdiv(C, 256)), dim3(256), t->part, 1, C, 1, 1.0 / t->R, t->grads + t->o_g[l], t->grads + t->o_be[l],
               t->m1 + o, t->m2 + o);
        launch(tb_bn_bwd_gmax_apply_kernel, dim3(blocks_of(total)), dim3(256), dpool, t->arg, t->a[l], total, t->n, C, mean, var,
               t->params + t->o_g[l], t->m1 + o, t->m2 + o, AT_EPS, da);
    }
};

int run_step(geoadv_atlas_trainer *t, const float *x, hipStream_t st) {
    Run q{{{st}, t, AT_EPS, t->part, t->partials}, t};
    const int B = t->B, nb = t->nb, p = t->p, NL = t->nl, LAST = NL - 1;
    const dim3 blk(256);
    // ---- forward: encoder ----
    q.bn_layer(E1, x, t->h[E1]);
    q.bn_layer(E2, t->h[E1], t->h[E2]);
    q.bn_layer(E3, t->h[E2], nullptr);
    q.launch(tb_gmax_kernel, dim3(AT_LAT / 64, B), blk, t->a[E3], t->n, AT_LAT, t->inv + t->o_mv[E3], t->shift + t->o_mv[E3], t->pooled, t->arg);
    q.bn_layer(L1, t->pooled, t->h[L1]);
    q.bn_layer(L2, t->h[L1], t->h[L2]);                                   // the latent
    // ---- forward: decoder ----
    q.launch(at_t1_kernel, dim3(blocks_of(nb * p * AT_LAT)), blk, t->tmpl, q.W(D0), t->params + t->o_b[D0], p, nb * p * AT_LAT, t->t1);
    if (t->dbn) {
        const size_t o = t->o_mv[D0];
        q.launch(at_bn1_stats_kernel, dim3(cdiv(nb * AT_LAT, 256)), blk, t->t1, t->h[L2], p, B, AT_LAT, nb, t->params + t->o_g[D0],
                 t->params + t->o_be[D0], t->bat_mean + o, t->bat_var + o, t->inv + o, t->shift + o);
    }
    q.bn_relu(D0, t->h[D0]);
    for (int l = D1; l < LAST; ++l) q.bn_layer(l, t->h[l - 1], t->h[l]);
    q.launch(at_last_fwd_kernel, dim3(cdiv(t->rows, 4)), blk, t->h[LAST - 1], q.W(LAST), t->params + t->o_b[LAST], t->Rp, t->rows, t->prim);
    const size_t r3 = (size_t)t->rows * 3;
    q.launch(at_fuse_kernel<true>, dim3(blocks_of(r3)), blk, t->prim, t->recon, B, nb, p, r3);
    // ---- loss and its gradient ----
    if (q.ok())
        if (int rc = geoadv_nn_distance(B, t->n, x, t->m, t->recon, t->d1, t->i1, t->d2, t->i2, st)) return rc;
    q.launch(tb_loss_kernel, dim3(1), blk, t->d1, (size_t)t->R, t->d2, (size_t)t->rows, t->loss);
    if (q.ok())
        if (int rc = geoadv_nn_distance_grad(B, t->n, x, t->m, t->recon, t->gd1, t->i1, t->gd2, t->i2, t->dx, t->drecon, st)) return rc;
    q.launch(at_fuse_kernel<false>, dim3(blocks_of(r3)), blk, t->dprim, t->drecon, B, nb, p, r3);
    // ---- backward: decoder ----
    q.linear_bwd(LAST, t->h[LAST - 1], t->dprim, t->Y);                   // d h of the last hidden layer [nb][Rp][512]
    for (int l = LAST - 1; l >= D1; --l) {
        q.bn_bwd(l, t->Y, t->Z);                                          // d a_l
        q.linear_bwd(l, t->h[l - 1], t->Z, t->Y);                         // d h_{l-1} (l = D1: [nb][Rp][1024])
    }
    q.bn_bwd(D0, t->Y, t->Y);                                             // d pre1, in place
    const size_t tt = (size_t)nb * p * AT_LAT, tz = (size_t)nb * B * AT_LAT;
    q.launch(at_dt1_kernel, dim3(blocks_of(tt)), blk, t->Y, B, p, tt, t->dt1);
    q.launch(at_dzq_kernel, dim3(blocks_of(tz)), blk, t->Y, p, tz, t->dzq);
    q.launch(at_dz_kernel, dim3(cdiv(B * AT_LAT, 256)), blk, t->dzq, nb, B * AT_LAT, t->dz);
    q.launch(at_conv1_grad_kernel, dim3(cdiv(nb * AT_LAT, 256)), blk, t->dt1, t->tmpl, p, nb, t->grads + t->o_w[D0], t->grads + t->o_b[D0]);
    // ---- backward: encoder ----
    q.bn_bwd(L2, t->dz, t->dsm1);
    q.linear_bwd(L2, t->h[L1], t->dsm1, t->dsm2);                         // d h4 [B][1024]
    q.bn_bwd(L1, t->dsm2, t->dsm1);
    q.linear_bwd(L1, t->pooled, t->dsm1, t->dsm2);                        // d pooled [B][1024]
    q.bn_bwd_gmax(t->dsm2, t->Y);                                         // d a3 [R][1024]
    q.linear_bwd(E3, t->h[E2], t->Y, t->Z);                               // d h2 [R][128]
    q.bn_bwd(E2, t->Z, t->T);
    q.linear_bwd(E2, t->h[E1], t->T, t->Z);                               // d h1 [R][64]
    q.bn_bwd(E1, t->Z, t->T);
    q.linear_bwd(E1, x, t->T, nullptr);
    if (!q.ok()) {
        set_error("atlas_trainer_step: %s", hipGetErrorString(q.err));
        return GEOADV_EHIP;
    }
    // ---- optimizer, running statistics, counters ----
    if (int rc = q.adam_and_running<false>(t->lr, 0.f, t->step)) return rc;
    t->step += 1;
    t->tracked += 1;
    return GEOADV_OK;
}
}  // namespace

extern "C" int geoadv_atlas_trainer_create(geoadv_atlas_trainer **out, const geoadv_atlas_config *config, const geoadv_atlas_weights *init,
                                           const geoadv_atlas_train_config *cfg) {
    GA_REQUIRE(out && config && init && cfg, "atlas_trainer_create: null argument");
    GA_REQUIRE(config->dim_template == 2, "atlas_trainer_create: dim_template %d is not supported (2, the SQUARE template)", config->dim_template);
    GA_REQUIRE(config->activation == 0, "atlas_trainer_create: activation %d is not supported (0 = relu)", config->activation);
    GA_REQUIRE(config->bottleneck_size == AT_LAT && config->hidden_neurons == AT_HID,
               "atlas_trainer_create: bottleneck_size %d / hidden_neurons %d are not supported (1024 / 512)", config->bottleneck_size,
               config->hidden_neurons);
    GA_REQUIRE(config->num_layers >= 0 && config->num_layers <= 4, "atlas_trainer_create: num_layers %d out of range [0, 4]", config->num_layers);
    GA_REQUIRE(config->nb_primitives >= 1 && config->nb_primitives <= 128, "atlas_trainer_create: nb_primitives %d out of range [1, 128]",
               config->nb_primitives);
    GA_REQUIRE(cfg->batch != 1, "atlas_trainer_create: batch 1 cannot be trained: bn4 and bn5 (after lin1 and lin2) take their statistics "
                                "over the clouds of the batch and need at least 2");
    GA_REQUIRE(cfg->batch >= 2 && cfg->batch <= 1024, "atlas_trainer_create: batch %d out of range [2, 1024]", cfg->batch);
    GA_REQUIRE(cfg->n_points >= 1 && cfg->n_points <= 16384, "atlas_trainer_create: n_points %d out of range [1, 16384]", cfg->n_points);
    GA_REQUIRE((long long)cfg->batch * cfg->n_points <= AT_MAX_ROWS, "atlas_trainer_create: batch * n_points exceeds 2^17 rows");
    GA_REQUIRE(cfg->points_per_primitive >= 1 && (long long)cfg->points_per_primitive * config->nb_primitives <= 16384,
               "atlas_trainer_create: nb_primitives * points_per_primitive = %lld out of range [1, 16384]",
               (long long)cfg->points_per_primitive * config->nb_primitives);
    GA_REQUIRE((long long)cfg->batch * cfg->points_per_primitive * config->nb_primitives <= AT_MAX_DEC_ROWS,
               "atlas_trainer_create: nb_primitives * batch * points_per_primitive exceeds 2^18 decoder rows");
    GA_REQUIRE((long long)cfg->batch * cfg->points_per_primitive >= 2 || !config->decoder_bn,
               "atlas_trainer_create: a decoder batch norm needs at least 2 rows per primitive");
    GA_REQUIRE(cfg->initial_step >= 0 && cfg->initial_tracked >= 0, "atlas_trainer_create: initial_step and initial_tracked must be >= 0");
    const int L = config->num_layers, NL = 8 + L, dbn = config->decoder_bn ? 1 : 0;
    for (int l = 0; l < GEOADV_ATLAS_ENC_LAYERS; ++l)
        GA_REQUIRE(init->enc_w[l] && init->enc_b[l] && init->enc_gamma[l] && init->enc_beta[l] && init->enc_mean[l] && init->enc_var[l],
                   "atlas_trainer_create: null encoder pointer at layer %d", l);
    for (int l = 0; l < 3 + L; ++l) {
        GA_REQUIRE(init->dec_w[l] && init->dec_b[l], "atlas_trainer_create: null decoder pointer at layer %d", l);
        const bool has = init->dec_gamma[l] && init->dec_beta[l] && init->dec_mean[l] && init->dec_var[l];
        const bool none = !init->dec_gamma[l] && !init->dec_beta[l] && !init->dec_mean[l] && !init->dec_var[l];
        GA_REQUIRE((dbn && l < 2 + L) ? has : none, "atlas_trainer_create: decoder layer %d: batch-norm pointers do not match decoder_bn %d", l, dbn);
    }
    geoadv_atlas_trainer *t = new geoadv_atlas_trainer();
    t->B = cfg->batch; t->n = cfg->n_points; t->R = t->B * t->n; t->nb = config->nb_primitives; t->p = cfg->points_per_primitive;
    t->Rp = t->B * t->p; t->rows = t->nb * t->Rp; t->m = t->nb * t->p; t->L = L; t->dbn = dbn;
    t->lr = cfg->learning_rate; t->step = cfg->initial_step; t->tracked = cfg->initial_tracked;
    t->seed = (unsigned long long)cfg->seed;
    const int ein[5] = {3, 64, 128, AT_LAT, AT_LAT}, eout[5] = {64, 128, AT_LAT, AT_LAT, AT_LAT};
    TrainLayer table[MAXL];
    TrainInit in{};
    for (int l = 0; l < NL; ++l) {        // every layer but the last has a slot in the batch-norm arenas: identity constants without a norm
        const int d = l - D0;
        const bool slot = l < NL - 1;
        if (l < D0) table[l] = {ein[l], eout[l], 1, l <= E3 ? t->R : t->B, true, slot};
        else table[l] = {l == D0 ? 2 : l == D1 ? AT_LAT : AT_HID, l == D0 ? AT_LAT : slot ? AT_HID : 3, t->nb, t->Rp, dbn && slot, slot};
        in.w[l] = l < D0 ? init->enc_w[l] : init->dec_w[d]; in.b[l] = l < D0 ? init->enc_b[l] : init->dec_b[d];
        in.gamma[l] = l < D0 ? init->enc_gamma[l] : init->dec_gamma[d]; in.beta[l] = l < D0 ? init->enc_beta[l] : init->dec_beta[d];
        in.mean[l] = l < D0 ? init->enc_mean[l] : init->dec_mean[d]; in.var[l] = l < D0 ? init->enc_var[l] : init->dec_var[d];
    }
    t->lay_out(table, NL);
    const size_t R = t->R, B = t->B, rows = t->rows, nb = t->nb, p = t->p;
    hipError_t e = hipSuccess;
    std::vector<void *> &mem = t->allocs;
    t->alloc(true, e);
    for (int l = 0; l < NL - 1; ++l) {
        const size_t count = (l <= E3 ? R : l <= L2 ? B : rows) * t->kout(l);
        t->a[l] = l == D0 ? nullptr : dev_alloc<float>(mem, count, e);
        t->h[l] = l == E3 ? nullptr : dev_alloc<float>(mem, count, e);
    }
    t->pooled = dev_alloc<float>(mem, B * AT_LAT, e); t->arg = dev_alloc<int>(mem, B * AT_LAT, e);
    t->t1 = dev_alloc<float>(mem, nb * p * AT_LAT, e); t->dt1 = dev_alloc<float>(mem, nb * p * AT_LAT, e);
    t->tmpl = dev_alloc<float>(mem, nb * p * 2, e);
    t->prim = dev_alloc<float>(mem, rows * 3, e); t->recon = dev_alloc<float>(mem, rows * 3, e);
    t->dprim = dev_alloc<float>(mem, rows * 3, e); t->drecon = dev_alloc<float>(mem, rows * 3, e); t->dx = dev_alloc<float>(mem, R * 3, e);
    t->d1 = dev_alloc<float>(mem, R, e); t->i1 = dev_alloc<int>(mem, R, e); t->gd1 = dev_alloc<float>(mem, R, e);
    t->d2 = dev_alloc<float>(mem, rows, e); t->i2 = dev_alloc<int>(mem, rows, e); t->gd2 = dev_alloc<float>(mem, rows, e);
    t->loss = dev_alloc<float>(mem, 1, e);
    t->Y = dev_alloc<float>(mem, std::max(R, rows) * AT_LAT, e);
    t->Z = dev_alloc<float>(mem, std::max(R * 128, rows * AT_HID), e);
    t->T = dev_alloc<float>(mem, R * 128, e);
    t->dz = dev_alloc<float>(mem, B * AT_LAT, e); t->dsm1 = dev_alloc<float>(mem, B * AT_LAT, e); t->dsm2 = dev_alloc<float>(mem, B * AT_LAT, e);
    t->dzq = dev_alloc<double>(mem, nb * B * AT_LAT, e);
    t->partials = dev_alloc<float>(mem, CT_PARTIAL_FLOATS, e);
    t->part = dev_alloc<double2>(mem, std::max((size_t)cdiv((int)R, 256), nb * cdiv(t->Rp, 256)) * AT_LAT + 1024, e);
    t->upload(in, e);
    dev_upload(t->gd1, std::vector<float>(R, 1.f / (float)R), e);
    dev_upload(t->gd2, std::vector<float>(rows, 1.f / (float)rows), e);
    if (e != hipSuccess) {
        delete t;
        return train_create_error("atlas_trainer_create", e);
    }
    *out = t;
    return GEOADV_OK;
}

extern "C" void geoadv_atlas_trainer_destroy(geoadv_atlas_trainer *t) { delete t; }

extern "C" int geoadv_atlas_trainer_set_slots(geoadv_atlas_trainer *t, const float *slot1, const float *slot2) {
    GA_REQUIRE(t, "atlas_trainer_set_slots: null handle");
    return t->set_slots(slot1, slot2);
}

extern "C" int geoadv_atlas_trainer_set_learning_rate(geoadv_atlas_trainer *t, float learning_rate, int reset_optimizer) {
    GA_REQUIRE(t, "atlas_trainer_set_learning_rate: null handle");
    GA_REQUIRE(learning_rate >= 0.f, "atlas_trainer_set_learning_rate: the learning rate must be >= 0");
    if (reset_optimizer) {
        // no stream argument: wait for every step in flight on any stream, clear on the null stream, and return only once the
        // clear is done -- a step queued afterwards on a non-blocking stream (which the null stream does not order) sees zeros
        GA_HIP(hipDeviceSynchronize());
        GA_HIP(hipMemsetAsync(t->slot1, 0, sizeof(float) * t->P, nullptr));
        GA_HIP(hipMemsetAsync(t->slot2, 0, sizeof(float) * t->P, nullptr));
        GA_HIP(hipStreamSynchronize(nullptr));
        t->step = 0;
    }
    t->lr = learning_rate;
    return GEOADV_OK;
}

extern "C" int geoadv_atlas_trainer_step(geoadv_atlas_trainer *t, const float *x, int given_template, float *template_points, float *loss,
                                         void *stream) {
    GA_REQUIRE(t && x, "atlas_trainer_step: null argument");
    GA_REQUIRE(!given_template || template_points, "atlas_trainer_step: a given template needs its points");
    hipStream_t st = as_stream(stream);
    const size_t bytes = sizeof(float) * 2 * (size_t)t->nb * t->p;
    if (given_template) {
        GA_HIP(hipMemcpyAsync(t->tmpl, template_points, bytes, hipMemcpyDeviceToDevice, st));
    } else {
        const int total = t->nb * t->p * 2;
        hipLaunchKernelGGL(at_template_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, t->seed, (unsigned long long)t->tracked, t->p, total,
                           t->tmpl);
        GA_LAUNCH_CHECK();
        if (template_points) GA_HIP(hipMemcpyAsync(template_points, t->tmpl, bytes, hipMemcpyDeviceToDevice, st));
    }
    if (int rc = run_step(t, x, st)) return rc;
    if (loss) GA_HIP(hipMemcpyAsync(loss, t->loss, sizeof(float), hipMemcpyDeviceToDevice, st));
    return GEOADV_OK;
}

extern "C" int geoadv_atlas_trainer_buffers(geoadv_atlas_trainer *t, float **params, float **grads, size_t *count) {
    GA_REQUIRE(t, "atlas_trainer_buffers: null handle");
    t->buffers(params, grads, count);
    return GEOADV_OK;
}

extern "C" int geoadv_atlas_trainer_layout(const geoadv_atlas_trainer *t, size_t *offsets48, size_t *moving_offsets12) {
    GA_REQUIRE(t && offsets48, "atlas_trainer_layout: null argument");
    t->export_layout(offsets48, moving_offsets12, MAXL);
    return GEOADV_OK;
}

extern "C" int geoadv_atlas_trainer_counters(const geoadv_atlas_trainer *t, long long *step, long long *tracked) {
    GA_REQUIRE(t, "atlas_trainer_counters: null handle");
    if (step) *step = t->step;
    if (tracked) *tracked = t->tracked;
    return GEOADV_OK;
}

extern "C" int geoadv_atlas_trainer_state(const geoadv_atlas_trainer *t, int what, int layer, const void **ptr, size_t *count) {
    GA_REQUIRE(t && ptr && count, "atlas_trainer_state: null argument");
    const size_t B = t->B, R = t->R, rows = t->rows;
    switch (what) {
    case GEOADV_ATLAS_STATE_BN_MEAN: case GEOADV_ATLAS_STATE_BN_VAR: case GEOADV_ATLAS_STATE_RUNNING_MEAN: case GEOADV_ATLAS_STATE_RUNNING_VAR:
    case GEOADV_ATLAS_STATE_BN_INV: case GEOADV_ATLAS_STATE_BN_SHIFT: {
        const bool folded = what == GEOADV_ATLAS_STATE_BN_INV || what == GEOADV_ATLAS_STATE_BN_SHIFT;
        GA_REQUIRE(layer >= 0 && layer < t->nl - 1 && (folded || t->bn_of(layer)), "atlas_trainer_state: layer %d has no batch norm", layer);
        t->view(what, layer, ptr, count);
        return GEOADV_OK;
    }
    case GEOADV_ATLAS_STATE_PRE_BN:
        GA_REQUIRE(layer >= 0 && layer < t->nl - 1, "atlas_trainer_state: layer %d has no stored activation", layer);
        if (layer == D0) { *ptr = t->t1; *count = (size_t)t->nb * t->p * AT_LAT; return GEOADV_OK; }
        *ptr = t->a[layer]; *count = (layer <= E3 ? R : layer <= L2 ? B : rows) * t->kout(layer);
        return GEOADV_OK;
    case GEOADV_ATLAS_STATE_CHAMFER_IDX:
        GA_REQUIRE(layer == 0 || layer == 1, "atlas_trainer_state: Chamfer direction %d must be 0 or 1", layer);
        *ptr = layer == 0 ? t->i1 : t->i2; *count = layer == 0 ? R : rows;
        return GEOADV_OK;
    case GEOADV_ATLAS_STATE_GMAX_ROW: *ptr = t->arg; *count = B * AT_LAT; return GEOADV_OK;
    case GEOADV_ATLAS_STATE_TEMPLATE: *ptr = t->tmpl; *count = (size_t)t->nb * t->p * 2; return GEOADV_OK;
    case GEOADV_ATLAS_STATE_LATENT: *ptr = t->h[L2]; *count = B * AT_LAT; return GEOADV_OK;
    case GEOADV_ATLAS_STATE_RECON: *ptr = t->recon; *count = rows * 3; return GEOADV_OK;
    case GEOADV_ATLAS_STATE_SLOT1: t->view(TA_SLOT1, 0, ptr, count); return GEOADV_OK;
    case GEOADV_ATLAS_STATE_SLOT2: t->view(TA_SLOT2, 0, ptr, count); return GEOADV_OK;
    default: break;
    }
    set_error("atlas_trainer_state: unknown state %d", what);
    return GEOADV_EINVAL;
}

extern "C" size_t geoadv_train_gemm_partial_floats(void) { return CT_PARTIAL_FLOATS; }

extern "C" int geoadv_train_gemm(int kernel, const float *A, long long sAi, long long sAk, long long sAz, const float *B, long long sBk,
                                 long long sBj, long long sBz, float *C, long long ldc, long long sCz, const float *bias, long long sBiasZ,
                                 int M, int N, int K, int batch, float *partials, size_t partial_floats, int *ksplit_out, void *stream) {
    GA_REQUIRE(kernel == 0 || kernel == 1, "train_gemm: kernel %d must be 0 (split-K) or 1 (128-tile)", kernel);
    GA_REQUIRE(A && B && C, "train_gemm: null operand");
    GA_REQUIRE(M >= 1 && N >= 1 && K >= 1 && batch >= 1 && batch <= 1024 && M <= (1 << 20) && N <= (1 << 20),
               "train_gemm: M, N in 1 ... 2^20, K >= 1 and batch in 1 ... 1024 (got %d x %d over %d, batch %d)", M, N, K, batch);
    GA_REQUIRE(ldc >= N, "train_gemm: ldc %lld is below N = %d", ldc, N);
    const BGemm g{A, sAi, sAk, sAz, B, sBk, sBj, sBz, C, ldc, sCz, bias, sBiasZ, M, N, K};
    hipStream_t st = as_stream(stream);
    if (kernel == 1) {
        if (ksplit_out) *ksplit_out = 1;
        GA_HIP(at_launch_gemm(g, batch, st));
        return GEOADV_OK;
    }
    GA_REQUIRE(!(bias && batch > 1 && sBiasZ != 0), "train_gemm: the split-K kernel has one bias for all groups (bias stride %lld with batch %d)",
               sBiasZ, batch);
    GA_REQUIRE(partials && partial_floats >= CT_PARTIAL_FLOATS, "train_gemm: the split-K kernel needs %zu floats of partials (got %zu)",
               (size_t)CT_PARTIAL_FLOATS, partial_floats);
    if (ksplit_out) *ksplit_out = ct_ksplit(M, N, K, batch);
    GA_HIP(at_launch_splitk(g, batch, partials, st));
    return GEOADV_OK;
}
