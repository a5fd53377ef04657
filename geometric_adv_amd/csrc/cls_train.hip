// geoadv_cls_trainer: one TRAINING step of the PointNet classifier (classifier/train_classifier.py: train_one_epoch's
// sess.run([train_op, loss, pred]) at is_training = True) on gfx950, fp32 in and out.
//
// Graph (pointnet_cls.py get_model + transform_nets.py, the layers of GEOADV_CLS_*): every batch norm uses the batch's own
// tf.nn.moments (population variance, eps 1e-3) over the B*N rows of a conv layer or the B clouds of an fc layer
// (batch_norm_for_fc), applied after the conv/fc bias, ReLU after the BN.  T1 = transform_XYZ + I, T2 = transform_feat + I
// (the identity is added in the graph, not stored in the variable).  Max pool over points.  tf.nn.dropout(keep_prob 0.7) after
// the BN + ReLU of fc1 and fc2 as (x / 0.7f) * mask.  fc3 is linear.
// Loss: mean(sparse_softmax_cross_entropy(logits, label)) + 0.001 * l2_loss(T2 T2^T - I), l2_loss = 1/2 * sum over the batch.
//
// FORM: the DIRECT one.  Every pre-BN activation a_l is stored (about 1 GB at B = 32 x 2048; the three 1024-wide layers are
// 0.8 GB of it) and the step runs layer by layer: per-point GEMMs and weight gradients on v_mfma_f32_32x32x2_f32 (64 x 64 tiles
// per workgroup, fixed split-K with the partials added in a fixed order in double), batch statistics as per-chunk double
// partials added in a fixed order, so a step is bitwise reproducible.  The transforms are applied as stored products
// u = x T1 (3 wide) and v = h2 T2 (64 wide), per cloud.  The Gram / sparse-gradient algebra for the wide layers is
// not used: it is left for a later change, with this form as the yardstick it must match.
//
// Max-pool gradient: to ONE row per (cloud, channel), the first (lowest point index) maximum -- the rule of TF's CPU
// MaxPoolGrad and its GPU kernel without a mask; unpinned against cuDNN's.  ReLU gradient: [relu output > 0].
//
// Dropout randomness (TF's generator cannot be reproduced; same distribution, keep with probability 0.7):
//   mix(z)  = splitmix64's finaliser: z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27; z *= 0x94d049bb133111eb; z ^= z >> 31
//   h       = mix(mix(seed + G * (step + 1)) ^ ((layer << 48) | (cloud << 24) | channel)),  G = 0x9e3779b97f4a7c15 (mod 2^64)
//   keep    = (h >> 40) < 11744051          (11744051 = round(0.7 * 2^24))
// step = the global step counter `batch` before the step increments it, layer 0 = fc1's dropout, 1 = fc2's.
//
// Optimizers (TF 1.13): ApplyAdam (beta1 .9, beta2 .999, eps 1e-8, one shared pair of beta powers) or ApplyMomentum
// (accum = momentum * accum + g; var -= lr * accum).  Schedules with k = the step counter before the increment:
// lr = max(base * decay_rate^floor(k B / decay_step), 1e-5), bn_decay = min(0.99, 1 - 0.5 * 0.5^floor(k B / decay_step)).
// Moving statistics: ExponentialMovingAverage(bn_decay) of the moments tensors (zero slots, zero_debias = False):
// shadow -= (shadow - batch_stat) * (1 - bn_decay).
#include "train_bn.h"

namespace geoadv {

constexpr float CT_KEEP = 0.7f, CT_EPS = 1e-3f;
constexpr unsigned CT_KEEP_BELOW = 11744051u;

__device__ __forceinline__ float ct_keep(unsigned long long seed, long long step, int layer, int cloud, int ch) {
    const unsigned long long h = mix64(mix64(seed + kGolden64 * (unsigned long long)(step + 1)) ^
                                        (((unsigned long long)layer << 48) | ((unsigned long long)cloud << 24) | (unsigned long long)ch));
    return (unsigned)(h >> 40) < CT_KEEP_BELOW ? 1.f : 0.f;
}

// y = relu(a * inv + shift) [ -> (y / 0.7f) * mask ]; rows of `per_cloud` rows belong to one cloud (dropout only on fc rows).
__global__ __launch_bounds__(256) void ct_bn_fwd_kernel(const float *a, int R, int C, const float *inv, const float *shift, float *y,
                                                        int dropout_layer, unsigned long long seed, long long step, float *mask) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)R * C) return;
    const int c = (int)(e % C), r = (int)(e / C);
    float v = fmaxf(tb_pre(a[e], inv[c], shift[c]), 0.f);
    if (dropout_layer >= 0) {
        const float m = ct_keep(seed, step, dropout_layer, r, c);
        mask[e] = m;
        v = (v / CT_KEEP) * m;
    }
    y[e] = v;
}

// Max pool of relu(a * inv + shift) over the n rows of each cloud: the maximum and its FIRST row.  grid (ceil(C / 64), B).
__global__ __launch_bounds__(256) void ct_pool_kernel(const float *a, int n, int C, const float *inv, const float *shift, float *pooled,
                                                      int *arg) {
    __shared__ float mv[4][64];
    __shared__ int mi[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6, b = blockIdx.y;
    float best = -1.f;
    int bi = 0;
    if (c < C) {
        const float iv = inv[c], sh = shift[c];
        for (int r = ph; r < n; r += 4) {
            const float v = fmaxf(tb_pre(a[((size_t)b * n + r) * C + c], iv, sh), 0.f);
            if (v > best) { best = v; bi = r; }
        }
    }
    mv[ph][threadIdx.x & 63] = best;
    mi[ph][threadIdx.x & 63] = bi;
    __syncthreads();
    if (ph == 0 && c < C) {
        for (int p = 1; p < 4; ++p) {
            const float v = mv[p][threadIdx.x];
            const int i = mi[p][threadIdx.x];
            if (v > best || (v == best && i < bi)) { best = v; bi = i; }
        }
        pooled[(size_t)b * C + c] = best;
        arg[(size_t)b * C + c] = bi;
    }
}

// BN backward, dense dy (optionally through the dropout mask):  g = dy [* mask / 0.7] * [a * inv + shift > 0].
// Pass 1 (partials per chunk): (sum g, sum g * xhat) with xhat = (a - mean) * rsqrt(var + eps).
template <bool DROP>
__global__ __launch_bounds__(256) void ct_bn_bwd_part_kernel(const float *dy, const float *mask, const float *a, int R, int C,
                                                             int rows_per_chunk, const float *mean, const float *var, const float *inv,
                                                             const float *shift, double2 *part) {
    __shared__ double2 red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
    const int r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    double s = 0.0, q = 0.0;
    if (c < C) {
        const float rs = 1.0f / sqrtf(var[c] + CT_EPS), m = mean[c], iv = inv[c], sh = shift[c];
        for (int r = r0 + ph; r < r1; r += 4) {
            const size_t e = (size_t)r * C + c;
            const float av = a[e];
            float gv = tb_pre(av, iv, sh) > 0.f ? dy[e] : 0.f;
            if (DROP) gv = gv * mask[e] / CT_KEEP;
            s += (double)gv;
            q += (double)gv * (double)((av - m) * rs);
        }
    }
    red[ph][threadIdx.x & 63] = make_double2(s, q);
    __syncthreads();
    if (ph == 0 && c < C) {
        double2 o = red[0][threadIdx.x];
        for (int p = 1; p < 4; ++p) { o.x += red[p][threadIdx.x].x; o.y += red[p][threadIdx.x].y; }
        part[(size_t)blockIdx.y * C + c] = o;
    }
}

// Pool form of pass 1: g is nonzero only at the argmax row of each (cloud, channel): dbeta = sum_b g, dgamma = sum_b g xhat.
// One thread per channel, clouds in ascending order.  Writes the totals as a single chunk.
__global__ __launch_bounds__(256) void ct_bn_bwd_pool_part_kernel(const float *dpool, const int *arg, const float *a, int B, int n, int C,
                                                                  const float *mean, const float *var, const float *inv,
                                                                  const float *shift, double2 *part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float rs = 1.0f / sqrtf(var[c] + CT_EPS), m = mean[c], iv = inv[c], sh = shift[c];
    double s = 0.0, q = 0.0;
    for (int b = 0; b < B; ++b) {
        const float av = a[((size_t)b * n + arg[(size_t)b * C + c]) * C + c];
        const float gv = tb_pre(av, iv, sh) > 0.f ? dpool[(size_t)b * C + c] : 0.f;
        s += (double)gv;
        q += (double)gv * (double)((av - m) * rs);
    }
    part[c] = make_double2(s, q);
}

// Pass 3: da = gamma * rs * (g - m1 - xhat * m2).  MODE 0 dense dy, 1 dense dy through dropout, 2 pool (dpool at the argmax row).
template <int MODE>
__global__ __launch_bounds__(256) void ct_bn_bwd_apply_kernel(const float *dy, const float *mask, const int *arg, const float *a, int R,
                                                              int n, int C, const float *mean, const float *var, const float *gamma,
                                                              const float *inv, const float *shift, const float *m1, const float *m2,
                                                              float *da) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)R * C) return;
    const int c = (int)(e % C), r = (int)(e / C);
    const float av = a[e];
    float gv = 0.f;
    if (tb_pre(av, inv[c], shift[c]) > 0.f) {
        if (MODE == 2) {
            const int b = r / n;
            if (arg[(size_t)b * C + c] == r - b * n) gv = dy[(size_t)b * C + c];
        } else {
            gv = dy[e];
            if (MODE == 1) gv = gv * mask[e] / CT_KEEP;
        }
    }
    const float rs = 1.0f / sqrtf(var[c] + CT_EPS);
    const float xh = (av - mean[c]) * rs;
    da[e] = gamma[c] * rs * (gv - m1[c] - xh * m2[c]);
}

// ---- small kernels --------------------------------------------------------------------------------------------------------
// out[b][k*k] += I  (T = transform + I)
__global__ void ct_add_eye_kernel(float *t, int B, int k) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= B * k) return;
    t[(e / k) * k * k + (e % k) * (k + 1)] += 1.f;
}

// E = T2 T2^T - I in place (the Gram was written to E); reg partials: sum of E^2 per cloud, in double (fixed order)
__global__ __launch_bounds__(256) void ct_reg_kernel(float *E, int B, double *reg_cloud) {
    __shared__ double red[256];
    const int b = blockIdx.x;
    double s = 0.0;
    for (int e = threadIdx.x; e < 4096; e += 256) {
        float v = E[(size_t)b * 4096 + e];
        if (e / 64 == e % 64) v = v - 1.f;
        E[(size_t)b * 4096 + e] = v;
        s += (double)v * v;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int i = 0; i < 256; ++i) t += red[i];
        reg_cloud[b] = t;
    }
}

// Softmax cross entropy (per cloud, double), dlogits = (softmax - onehot) / B, argmax (first maximum), and the loss:
// mean CE + 0.001 * 0.5 * sum E^2.  One block, thread = cloud, then thread 0 adds the clouds in order.
__global__ __launch_bounds__(1024) void ct_loss_kernel(const float *logits, const int *labels, int B, int C, const double *reg_cloud,
                                                       float *dlogits, int *pred, float *loss, double *ce_cloud) {
    const int b = threadIdx.x;
    if (b < B) {
        const float *z = logits + (size_t)b * C;
        double mx = z[0];
        int best = 0;
        for (int j = 1; j < C; ++j) if (z[j] > z[best]) best = j;
        mx = z[best];
        double se = 0.0;
        for (int j = 0; j < C; ++j) se += exp((double)z[j] - mx);
        const int lab = labels[b];
        ce_cloud[b] = log(se) + mx - (double)z[lab];
        for (int j = 0; j < C; ++j)
            dlogits[(size_t)b * C + j] = (float)((exp((double)z[j] - mx) / se - (j == lab ? 1.0 : 0.0)) / B);
        pred[b] = best;
    }
    __syncthreads();
    if (b == 0) {
        double ce = 0.0, reg = 0.0;
        for (int i = 0; i < B; ++i) { ce += ce_cloud[i]; reg += reg_cloud[i]; }
        loss[0] = (float)(ce / B + 0.001 * 0.5 * reg);
    }
}

__global__ void ct_adam_kernel(float *p, float *m, float *v, const float *g, size_t count, float lr, float b1p, float b2p) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float alpha = lr * sqrtf(1.f - b2p) / (1.f - b1p);
    const float gv = g[e];
    const float mn = m[e] + (gv - m[e]) * (1.f - 0.9f);
    const float vn = v[e] + (gv * gv - v[e]) * (1.f - 0.999f);
    m[e] = mn; v[e] = vn;
    p[e] = p[e] - (mn * alpha) / (sqrtf(vn) + 1e-8f);
}

__global__ void ct_momentum_kernel(float *p, float *acc, const float *g, size_t count, float lr, float momentum) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float a = acc[e] * momentum + g[e];
    acc[e] = a;
    p[e] = p[e] - lr * a;
}

// shadow -= (shadow - stat) * (1 - decay) over the flat moving-statistics arena
__global__ void ct_ema_kernel(float *shadow, const float *stat, size_t count, float one_minus_decay) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    shadow[e] = shadow[e] - (shadow[e] - stat[e]) * one_minus_decay;
}

}  // namespace geoadv

using namespace geoadv;

namespace {
enum { T1C1 = 0, T1C2, T1C3, T1F1, T1F2, T1XYZ, C1, C2, T2C1, T2C2, T2C3, T2F1, T2F2, T2FEAT, C3, C4, C5, F1, F2, F3, NL };
const int kIn[NL] = {3, 64, 128, 1024, 512, 256, 3, 64, 64, 64, 128, 1024, 512, 256, 64, 64, 128, 1024, 512, 256};
const int kOut[NL] = {64, 128, 1024, 512, 256, 9, 64, 64, 64, 128, 1024, 512, 256, 4096, 64, 128, 1024, 512, 256, 0};
bool bn_of(int l) { return l != T1XYZ && l != T2FEAT && l != F3; }
bool per_point(int l) { return l <= T1C3 || (l >= C1 && l <= T2C3) || (l >= C3 && l <= C5); }
bool pooled_layer(int l) { return l == T1C3 || l == T2C3 || l == C5; }
static_assert(NL <= TA_MAXL && GEOADV_CLS_STATE_BN_MEAN == TA_BAT_MEAN && GEOADV_CLS_STATE_BN_VAR == TA_BAT_VAR &&
              GEOADV_CLS_STATE_MOVING_MEAN == TA_RUN_MEAN && GEOADV_CLS_STATE_MOVING_VAR == TA_RUN_VAR,
              "geoadv_cls_trainer_state passes these to TrainArena::view as they are");
}  // namespace

struct geoadv_cls_trainer : TrainArena {           // run_mean / run_var: the moving averages
    int B, n, R, C, optimizer;
    float base_lr, momentum, decay_rate;
    long long decay_step, step;
    unsigned long long seed;
    float b1p, b2p;
    float *a[NL], *h[NL];                         // pre-BN outputs; post-BN(-ReLU(-dropout)) outputs of stored layers
    float *u, *v, *t1, *t2, *E, *pooled[3], *mask[2], *logits, *dlogits, *loss;
    int *arg[3], *labels, *pred;
    float *da, *dA, *dB, *dC, *dsmall1, *dsmall2, *du, *dv, *dT1, *dT2, *partials;
    double2 *part;
    double *reg_cloud, *ce_cloud;
    int chunks, rows_per_chunk;
};

namespace {
struct Run : TrainRun {
    geoadv_cls_trainer *t;

    // C = A B
    static GemmArgs plain(const float *A, const float *B, float *C, int M, int N, int K) {
        GemmArgs g{};
        g.A = A; g.sAi = K; g.sAk = 1;
        g.B = B; g.sBk = N; g.sBj = 1;
        g.C = C; g.ldc = N;
        g.alpha = 1.f; g.M = M; g.N = N; g.K = K; g.batch = 1;
        return g;
    }
    int rows(int l) const { return t->layer[l].rows; }
    // a_l = in @ W_l + b_l
    void linear_fwd(int l, const float *in, float *outp) { gemm(fwd_args(l, in, outp, rows(l), 0, kIn[l], true)); }
    void batch_stats(int l) { TrainRun::batch_stats(l, t->a[l]); }
    // BN + ReLU (+ dropout) of a stored layer
    void bn_fwd(int l, int drop) {
        const int R = rows(l), C = t->kout(l);
        const size_t o = t->o_mv[l];
        launch(ct_bn_fwd_kernel, dim3(blocks_of((size_t)R * C)), dim3(256), t->a[l], R, C, t->inv + o, t->shift + o, t->h[l], drop, t->seed, t->step,
               drop >= 0 ? t->mask[drop] : nullptr);
    }
    void pool(int l, int which) {
        const size_t o = t->o_mv[l];
        launch(ct_pool_kernel, dim3(cdiv(t->kout(l), 64), t->B), dim3(256), t->a[l], t->n, t->kout(l), t->inv + o, t->shift + o, t->pooled[which],
               t->arg[which]);
    }
    void layer(int l, const float *in) { linear_fwd(l, in, t->a[l]); batch_stats(l); bn_fwd(l, l == F1 ? 0 : l == F2 ? 1 : -1); }

    // BN backward of layer l: mode 0 dense, 1 dense through dropout mask `drop`, 2 pool `which` (dy = dpool [B][C]).
    void bn_bwd(int l, int mode, const float *dy, int aux, float *da) {
        const int R = rows(l), C = t->kout(l);
        const size_t o = t->o_mv[l];
        const float *mean = t->bat_mean + o, *var = t->bat_var + o, *iv = t->inv + o, *sh = t->shift + o, *gam = t->params + t->o_g[l];
        const int rpc = rpc_of(R), chunks = mode == 2 ? 1 : cdiv(R, rpc);
        const dim3 rows_grid(cdiv(C, 64), chunks), flat(blocks_of((size_t)R * C));
        if (mode == 2)
            launch(ct_bn_bwd_pool_part_kernel, dim3(cdiv(C, 256)), dim3(256), dy, t->arg[aux], t->a[l], t->B, t->n, C, mean, var, iv, sh, t->part);
        else if (mode == 1)
            launch(ct_bn_bwd_part_kernel<true>, rows_grid, dim3(256), dy, t->mask[aux], t->a[l], R, C, rpc, mean, var, iv, sh, t->part);
        else
            launch(ct_bn_bwd_part_kernel<false>, rows_grid, dim3(256), dy, nullptr, t->a[l], R, C, rpc, mean, var, iv, sh, t->part);
        launch(tb_bn_bwd_final_kernel, dim3(cdiv(C, 256)), dim3(256), t->part, chunks, C, 1, 1.0 / R, t->grads + t->o_g[l], t->grads + t->o_be[l],
               t->m1 + o, t->m2 + o);
        if (mode == 0)
            launch(ct_bn_bwd_apply_kernel<0>, flat, dim3(256), dy, nullptr, nullptr, t->a[l], R, t->n, C, mean, var, gam, iv, sh, t->m1 + o,
                   t->m2 + o, da);
        else if (mode == 1)
            launch(ct_bn_bwd_apply_kernel<1>, flat, dim3(256), dy, t->mask[aux], nullptr, t->a[l], R, t->n, C, mean, var, gam, iv, sh, t->m1 + o,
                   t->m2 + o, da);
        else
            launch(ct_bn_bwd_apply_kernel<2>, flat, dim3(256), dy, nullptr, t->arg[aux], t->a[l], R, t->n, C, mean, var, gam, iv, sh, t->m1 + o,
                   t->m2 + o, da);
    }
    // dW_l = in^T da, db_l = sum da, din (=|+=) da W_l^T
    void linear_bwd(int l, const float *in, const float *da, float *din, int accumulate) {
        gemm(wgrad_args(l, in, da, rows(l), 0, kIn[l]));
        bias_grad(l, da);
        if (din) gemm(igrad_args(l, da, din, rows(l), 0, kIn[l], accumulate));
    }
    void add_eye(float *p, int kk) { launch(ct_add_eye_kernel, dim3(cdiv(t->B * kk, 256)), dim3(256), p, t->B, kk); }
};

int run_step(geoadv_cls_trainer *t, const float *x, const int *labels_dev, hipStream_t st) {
    Run q{{{st}, t, CT_EPS, t->part, t->partials}, t};
    const int B = t->B, n = t->n, R = t->R, NC = t->C;
    // ---- forward ----
    q.layer(T1C1, x);
    q.layer(T1C2, t->h[T1C1]);
    q.linear_fwd(T1C3, t->h[T1C2], t->a[T1C3]); q.batch_stats(T1C3); q.pool(T1C3, 0);
    q.layer(T1F1, t->pooled[0]);
    q.layer(T1F2, t->h[T1F1]);
    q.linear_fwd(T1XYZ, t->h[T1F2], t->t1);
    q.add_eye(t->t1, 3);
    {   // u = x T1 per cloud
        GemmArgs g = Run::plain(x, t->t1, t->u, n, 3, 3);
        g.sAz = (long long)n * 3; g.sBz = 9; g.sCz = (long long)n * 3; g.batch = B;
        q.gemm(g);
    }
    q.layer(C1, t->u);
    q.layer(C2, t->h[C1]);
    q.layer(T2C1, t->h[C2]);
    q.layer(T2C2, t->h[T2C1]);
    q.linear_fwd(T2C3, t->h[T2C2], t->a[T2C3]); q.batch_stats(T2C3); q.pool(T2C3, 1);
    q.layer(T2F1, t->pooled[1]);
    q.layer(T2F2, t->h[T2F1]);
    q.linear_fwd(T2FEAT, t->h[T2F2], t->t2);
    q.add_eye(t->t2, 64);
    {   // v = h2 T2 per cloud
        GemmArgs g = Run::plain(t->h[C2], t->t2, t->v, n, 64, 64);
        g.sAz = (long long)n * 64; g.sBz = 4096; g.sCz = (long long)n * 64; g.batch = B;
        q.gemm(g);
    }
    q.layer(C3, t->v);
    q.layer(C4, t->h[C3]);
    q.linear_fwd(C5, t->h[C4], t->a[C5]); q.batch_stats(C5); q.pool(C5, 2);
    q.layer(F1, t->pooled[2]);
    q.layer(F2, t->h[F1]);
    q.linear_fwd(F3, t->h[F2], t->logits);
    {   // E = T2 T2^T - I, its squared sum per cloud
        GemmArgs g{};
        g.A = t->t2; g.sAi = 64; g.sAk = 1; g.sAz = 4096;
        g.B = t->t2; g.sBk = 1; g.sBj = 64; g.sBz = 4096;
        g.C = t->E; g.ldc = 64; g.sCz = 4096;
        g.alpha = 1.f; g.M = 64; g.N = 64; g.K = 64; g.batch = B;
        q.gemm(g);
    }
    q.launch(ct_reg_kernel, dim3(B), dim3(256), t->E, B, t->reg_cloud);
    q.launch(ct_loss_kernel, dim3(1), dim3(1024), t->logits, labels_dev, B, NC, t->reg_cloud, t->dlogits, t->pred, t->loss, t->ce_cloud);
    // ---- backward ----
    q.linear_bwd(F3, t->h[F2], t->dlogits, t->dsmall1, 0);                 // d h_F2 [B][256]
    q.bn_bwd(F2, 1, t->dsmall1, 1, t->dsmall2);
    q.linear_bwd(F2, t->h[F1], t->dsmall2, t->dsmall1, 0);                 // d h_F1 [B][512]
    q.bn_bwd(F1, 1, t->dsmall1, 0, t->dsmall2);
    q.linear_bwd(F1, t->pooled[2], t->dsmall2, t->dsmall1, 0);             // d pool3 [B][1024]
    q.bn_bwd(C5, 2, t->dsmall1, 2, t->da);
    q.linear_bwd(C5, t->h[C4], t->da, t->dA, 0);                           // d h_C4 [R][128]
    q.bn_bwd(C4, 0, t->dA, 0, t->da);
    q.linear_bwd(C4, t->h[C3], t->da, t->dB, 0);                           // d h_C3 [R][64]
    q.bn_bwd(C3, 0, t->dB, 0, t->da);
    q.linear_bwd(C3, t->v, t->da, t->dv, 0);                               // d v [R][64]
    {   // dT2 = h2^T dv per cloud, + 0.002 E T2 (the regulariser)
        GemmArgs g{};
        g.A = t->h[C2]; g.sAi = 1; g.sAk = 64; g.sAz = (long long)n * 64;
        g.B = t->dv; g.sBk = 64; g.sBj = 1; g.sBz = (long long)n * 64;
        g.C = t->dT2; g.ldc = 64; g.sCz = 4096;
        g.alpha = 1.f; g.M = 64; g.N = 64; g.K = n; g.batch = B;
        q.gemm(g);
        GemmArgs r = Run::plain(t->E, t->t2, t->dT2, 64, 64, 64);
        r.sAz = 4096; r.sBz = 4096; r.sCz = 4096; r.batch = B; r.alpha = 0.002f; r.accumulate = 1;
        q.gemm(r);
        // d h2 = dv T2^T per cloud
        GemmArgs d{};
        d.A = t->dv; d.sAi = 64; d.sAk = 1; d.sAz = (long long)n * 64;
        d.B = t->t2; d.sBk = 1; d.sBj = 64; d.sBz = 4096;
        d.C = t->dC; d.ldc = 64; d.sCz = (long long)n * 64;
        d.alpha = 1.f; d.M = n; d.N = 64; d.K = 64; d.batch = B;
        q.gemm(d);
    }
    q.linear_bwd(T2FEAT, t->h[T2F2], t->dT2, t->dsmall1, 0);               // d h_T2F2 [B][256]
    q.bn_bwd(T2F2, 0, t->dsmall1, 0, t->dsmall2);
    q.linear_bwd(T2F2, t->h[T2F1], t->dsmall2, t->dsmall1, 0);
    q.bn_bwd(T2F1, 0, t->dsmall1, 0, t->dsmall2);
    q.linear_bwd(T2F1, t->pooled[1], t->dsmall2, t->dsmall1, 0);           // d pool2
    q.bn_bwd(T2C3, 2, t->dsmall1, 1, t->da);
    q.linear_bwd(T2C3, t->h[T2C2], t->da, t->dA, 0);                       // d h_T2C2 [R][128]
    q.bn_bwd(T2C2, 0, t->dA, 0, t->da);
    q.linear_bwd(T2C2, t->h[T2C1], t->da, t->dB, 0);                       // d h_T2C1 [R][64]
    q.bn_bwd(T2C1, 0, t->dB, 0, t->da);
    q.linear_bwd(T2C1, t->h[C2], t->da, t->dC, 1);                         // d h2 += (conv2 feeds T-Net2 and conv3)
    q.bn_bwd(C2, 0, t->dC, 0, t->da);
    q.linear_bwd(C2, t->h[C1], t->da, t->dB, 0);                           // d h_C1
    q.bn_bwd(C1, 0, t->dB, 0, t->da);
    q.linear_bwd(C1, t->u, t->da, t->du, 0);                               // d u [R][3]
    {   // dT1 = x^T du per cloud
        GemmArgs g{};
        g.A = x; g.sAi = 1; g.sAk = 3; g.sAz = (long long)n * 3;
        g.B = t->du; g.sBk = 3; g.sBj = 1; g.sBz = (long long)n * 3;
        g.C = t->dT1; g.ldc = 3; g.sCz = 9;
        g.alpha = 1.f; g.M = 3; g.N = 3; g.K = n; g.batch = B;
        q.gemm(g);
    }
    q.linear_bwd(T1XYZ, t->h[T1F2], t->dT1, t->dsmall1, 0);
    q.bn_bwd(T1F2, 0, t->dsmall1, 0, t->dsmall2);
    q.linear_bwd(T1F2, t->h[T1F1], t->dsmall2, t->dsmall1, 0);
    q.bn_bwd(T1F1, 0, t->dsmall1, 0, t->dsmall2);
    q.linear_bwd(T1F1, t->pooled[0], t->dsmall2, t->dsmall1, 0);           // d pool1
    q.bn_bwd(T1C3, 2, t->dsmall1, 0, t->da);
    q.linear_bwd(T1C3, t->h[T1C2], t->da, t->dA, 0);
    q.bn_bwd(T1C2, 0, t->dA, 0, t->da);
    q.linear_bwd(T1C2, t->h[T1C1], t->da, t->dB, 0);
    q.bn_bwd(T1C1, 0, t->dB, 0, t->da);
    q.linear_bwd(T1C1, x, t->da, nullptr, 0);
    (void)R;
    if (!q.ok()) {
        set_error("cls_trainer_step: %s", hipGetErrorString(q.err));
        return GEOADV_EHIP;
    }
    // ---- optimizer, moving averages, counters ----
    const double e = floor((double)t->step * B / (double)t->decay_step);
    const float lr = (float)std::max((double)t->base_lr * pow((double)t->decay_rate, e), 1e-5);
    const float bn_decay = (float)std::min(0.99, 1.0 - 0.5 * pow(0.5, e));
    const unsigned pg = blocks_of(t->P);
    if (t->optimizer == GEOADV_CLS_OPT_ADAM)
        hipLaunchKernelGGL(ct_adam_kernel, dim3(pg), dim3(256), 0, st, t->params, t->slot1, t->slot2, t->grads, t->P, lr, t->b1p, t->b2p);
    else
        hipLaunchKernelGGL(ct_momentum_kernel, dim3(pg), dim3(256), 0, st, t->params, t->slot1, t->grads, t->P, lr, t->momentum);
    GA_LAUNCH_CHECK();
    const unsigned mg = blocks_of(t->MV);
    hipLaunchKernelGGL(ct_ema_kernel, dim3(mg), dim3(256), 0, st, t->run_mean, t->bat_mean, t->MV, 1.f - bn_decay);
    GA_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_ema_kernel, dim3(mg), dim3(256), 0, st, t->run_var, t->bat_var, t->MV, 1.f - bn_decay);
    GA_LAUNCH_CHECK();
    if (t->optimizer == GEOADV_CLS_OPT_ADAM) { t->b1p = t->b1p * 0.9f; t->b2p = t->b2p * 0.999f; }
    t->step += 1;
    return GEOADV_OK;
}
}  // namespace

extern "C" int geoadv_cls_trainer_create(geoadv_cls_trainer **out, const geoadv_cls_weights *init, const geoadv_cls_train_config *cfg) {
    GA_REQUIRE(out && init && cfg, "cls_trainer_create: null argument");
    const int NC = init->num_classes;
    GA_REQUIRE(NC >= 1 && NC <= 1024, "cls_trainer_create: num_classes %d out of range [1, 1024]", NC);
    GA_REQUIRE(cfg->batch >= 1 && cfg->batch <= 1024, "cls_trainer_create: batch %d out of range [1, 1024]", cfg->batch);
    GA_REQUIRE(cfg->n_points >= 1 && cfg->n_points <= 16384, "cls_trainer_create: n_points %d out of range [1, 16384]", cfg->n_points);
    GA_REQUIRE((long long)cfg->batch * cfg->n_points <= (1 << 20), "cls_trainer_create: batch * n_points exceeds 2^20 rows");
    GA_REQUIRE(cfg->optimizer == GEOADV_CLS_OPT_ADAM || cfg->optimizer == GEOADV_CLS_OPT_MOMENTUM, "cls_trainer_create: unknown optimizer %d",
               cfg->optimizer);
    GA_REQUIRE(cfg->decay_step >= 1, "cls_trainer_create: decay_step must be >= 1");
    GA_REQUIRE(cfg->initial_step >= 0, "cls_trainer_create: initial_step must be >= 0");
    for (int l = 0; l < NL; ++l) {
        GA_REQUIRE(init->w[l] && init->b[l], "cls_trainer_create: null weight pointer at layer %d", l);
        if (bn_of(l)) GA_REQUIRE(init->gamma[l] && init->beta[l] && init->mean[l] && init->var[l], "cls_trainer_create: null batch-norm pointer at layer %d", l);
    }
    geoadv_cls_trainer *t = new geoadv_cls_trainer();
    t->B = cfg->batch; t->n = cfg->n_points; t->R = t->B * t->n; t->C = NC;
    t->optimizer = cfg->optimizer; t->base_lr = cfg->learning_rate; t->momentum = cfg->momentum;
    t->decay_step = cfg->decay_step; t->decay_rate = cfg->decay_rate; t->step = cfg->initial_step;
    t->seed = (unsigned long long)(unsigned)cfg->dropout_seed;
    t->b1p = 0.9f; t->b2p = 0.999f;
    TrainLayer table[NL];
    TrainInit in{};
    for (int l = 0; l < NL; ++l) {
        table[l] = {kIn[l], l == F3 ? NC : kOut[l], 1, per_point(l) ? t->R : t->B, bn_of(l), false};
        in.w[l] = init->w[l]; in.b[l] = init->b[l]; in.gamma[l] = init->gamma[l];
        in.beta[l] = init->beta[l]; in.mean[l] = init->mean[l]; in.var[l] = init->var[l];
    }
    t->lay_out(table, NL);
    const size_t R = t->R, B = t->B;
    hipError_t e = hipSuccess;
    std::vector<void *> &mem = t->allocs;
    t->alloc(false, e);
    for (int l = 0; l < NL; ++l) {
        t->a[l] = t->h[l] = nullptr;
        if (!bn_of(l)) continue;
        t->a[l] = dev_alloc<float>(mem, (per_point(l) ? R : B) * t->kout(l), e);
        if (!pooled_layer(l)) t->h[l] = dev_alloc<float>(mem, (per_point(l) ? R : B) * t->kout(l), e);
    }
    t->u = dev_alloc<float>(mem, R * 3, e); t->v = dev_alloc<float>(mem, R * 64, e);
    t->t1 = dev_alloc<float>(mem, B * 9, e); t->t2 = dev_alloc<float>(mem, B * 4096, e); t->E = dev_alloc<float>(mem, B * 4096, e);
    for (int i = 0; i < 3; ++i) { t->pooled[i] = dev_alloc<float>(mem, B * 1024, e); t->arg[i] = dev_alloc<int>(mem, B * 1024, e); }
    t->mask[0] = dev_alloc<float>(mem, B * 512, e); t->mask[1] = dev_alloc<float>(mem, B * 256, e);
    t->logits = dev_alloc<float>(mem, B * NC, e); t->dlogits = dev_alloc<float>(mem, B * NC, e); t->loss = dev_alloc<float>(mem, 1, e);
    t->labels = dev_alloc<int>(mem, B, e); t->pred = dev_alloc<int>(mem, B, e);
    t->da = dev_alloc<float>(mem, R * 1024, e); t->dA = dev_alloc<float>(mem, R * 128, e);
    t->dB = dev_alloc<float>(mem, R * 64, e); t->dC = dev_alloc<float>(mem, R * 64, e);
    t->dsmall1 = dev_alloc<float>(mem, B * 4096, e); t->dsmall2 = dev_alloc<float>(mem, B * 4096, e);
    t->du = dev_alloc<float>(mem, R * 3, e); t->dv = dev_alloc<float>(mem, R * 64, e);
    t->dT1 = dev_alloc<float>(mem, B * 9, e); t->dT2 = dev_alloc<float>(mem, B * 4096, e);
    t->partials = dev_alloc<float>(mem, CT_PARTIAL_FLOATS, e);
    t->part = dev_alloc<double2>(mem, std::max((size_t)cdiv((int)R, 256) * 1024, (size_t)cdiv((int)B, 256) * 4096) + 1024, e);
    t->reg_cloud = dev_alloc<double>(mem, B, e); t->ce_cloud = dev_alloc<double>(mem, B, e);
    t->upload(in, e);
    if (e != hipSuccess) {
        delete t;
        return train_create_error("cls_trainer_create", e);
    }
    *out = t;
    return GEOADV_OK;
}

extern "C" void geoadv_cls_trainer_destroy(geoadv_cls_trainer *t) { delete t; }

extern "C" int geoadv_cls_trainer_set_slots(geoadv_cls_trainer *t, const float *slot1, const float *slot2, float beta1_power,
                                            float beta2_power) {
    GA_REQUIRE(t, "cls_trainer_set_slots: null handle");
    if (int rc = t->set_slots(slot1, slot2)) return rc;
    t->b1p = beta1_power;
    t->b2p = beta2_power;
    return GEOADV_OK;
}

extern "C" int geoadv_cls_trainer_step(geoadv_cls_trainer *t, const float *x, const int *labels, float *loss, int *pred, void *stream) {
    GA_REQUIRE(t && x && labels, "cls_trainer_step: null argument");
    hipStream_t st = as_stream(stream);
    GA_HIP(hipMemcpyAsync(t->labels, labels, sizeof(int) * t->B, hipMemcpyDeviceToDevice, st));
    if (int rc = run_step(t, x, t->labels, st)) return rc;
    if (loss) GA_HIP(hipMemcpyAsync(loss, t->loss, sizeof(float), hipMemcpyDeviceToDevice, st));
    if (pred) GA_HIP(hipMemcpyAsync(pred, t->pred, sizeof(int) * t->B, hipMemcpyDeviceToDevice, st));
    return GEOADV_OK;
}

extern "C" int geoadv_cls_trainer_buffers(geoadv_cls_trainer *t, float **params, float **grads, size_t *count) {
    GA_REQUIRE(t, "cls_trainer_buffers: null handle");
    t->buffers(params, grads, count);
    return GEOADV_OK;
}

extern "C" int geoadv_cls_trainer_layout(const geoadv_cls_trainer *t, size_t *offsets80, size_t *moving_offsets20) {
    GA_REQUIRE(t && offsets80, "cls_trainer_layout: null argument");
    t->export_layout(offsets80, moving_offsets20, NL);
    return GEOADV_OK;
}

extern "C" int geoadv_cls_trainer_counters(const geoadv_cls_trainer *t, long long *step, float *beta1_power, float *beta2_power) {
    GA_REQUIRE(t, "cls_trainer_counters: null handle");
    if (step) *step = t->step;
    if (beta1_power) *beta1_power = t->b1p;
    if (beta2_power) *beta2_power = t->b2p;
    return GEOADV_OK;
}

extern "C" int geoadv_cls_trainer_state(const geoadv_cls_trainer *t, int what, int layer, const void **ptr, size_t *count) {
    GA_REQUIRE(t && ptr && count, "cls_trainer_state: null argument");
    const size_t B = t->B;
    switch (what) {
    case GEOADV_CLS_STATE_BN_MEAN: case GEOADV_CLS_STATE_BN_VAR: case GEOADV_CLS_STATE_MOVING_MEAN: case GEOADV_CLS_STATE_MOVING_VAR:
    case GEOADV_CLS_STATE_BN_INV: case GEOADV_CLS_STATE_BN_SHIFT:
        GA_REQUIRE(layer >= 0 && layer < NL && bn_of(layer), "cls_trainer_state: layer %d has no batch norm", layer);
        t->view(what == GEOADV_CLS_STATE_BN_INV ? TA_INV : what == GEOADV_CLS_STATE_BN_SHIFT ? TA_SHIFT : what, layer, ptr, count);
        return GEOADV_OK;
    case GEOADV_CLS_STATE_PRE_BN:
        GA_REQUIRE(layer >= 0 && layer < NL && bn_of(layer), "cls_trainer_state: layer %d has no batch norm", layer);
        *ptr = t->a[layer]; *count = (size_t)(per_point(layer) ? t->R : t->B) * t->kout(layer);
        return GEOADV_OK;
    case GEOADV_CLS_STATE_DROPOUT_MASK:
        GA_REQUIRE(layer == 0 || layer == 1, "cls_trainer_state: dropout layer %d must be 0 or 1", layer);
        *ptr = t->mask[layer]; *count = B * (layer == 0 ? 512 : 256);
        return GEOADV_OK;
    case GEOADV_CLS_STATE_POOL_ARGMAX:
        GA_REQUIRE(layer >= 0 && layer < 3, "cls_trainer_state: pool %d must be 0, 1 or 2", layer);
        *ptr = t->arg[layer]; *count = B * 1024;
        return GEOADV_OK;
    case GEOADV_CLS_STATE_T1: *ptr = t->t1; *count = B * 9; return GEOADV_OK;
    case GEOADV_CLS_STATE_T2: *ptr = t->t2; *count = B * 4096; return GEOADV_OK;
    case GEOADV_CLS_STATE_LOGITS: *ptr = t->logits; *count = B * t->C; return GEOADV_OK;
    case GEOADV_CLS_STATE_SLOT1: t->view(TA_SLOT1, 0, ptr, count); return GEOADV_OK;
    case GEOADV_CLS_STATE_SLOT2: t->view(TA_SLOT2, 0, ptr, count); return GEOADV_OK;
    default: break;
    }
    set_error("cls_trainer_state: unknown state %d", what);
    return GEOADV_EINVAL;
}
