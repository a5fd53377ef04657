// The batch-norm, column-sum, global-max, loss, Adam and running-statistics kernels of the layer-by-layer training steps
// (cls_train.hip, fold_train.hip, atlas_train.hip), each written once, and the host plumbing the three handles share:
// dev_alloc, blocks_of / rpc_of, the flat parameter and batch-norm arenas every handle derives from (TrainArena: layout,
// allocation, upload of the initial weights, set_slots, buffers, layout export, state lookup), the launch context (Launch) and
// a step on an arena (TrainRun: W, batch_stats, bias_grad, the GemmArgs of a dense layer's three products, the torch-form
// Adam and running-statistics tail).  As in train_tile.h every kernel is `static`: each translation unit that includes this
// header gets its own copy.  The GEMM and its split-K stay in train_tile.h; what depends on a model (its layer table and
// buffers, bn_bwd, dropout, ReLU pool, graph pool, the decoder's rebuilt statistics, the TensorFlow-form optimizers and EMA)
// stays with its trainer.
//
// BatchNorm in train mode: the BIASED batch variance normalises; eps is the trainer's (torch 1e-5, TF 1e-3) and is passed to
// every kernel that needs it.  inv = gamma / sqrt(var + eps), shift = beta - mean * inv, y = relu(a * inv + shift).
// STORED for the backward: the pre-BN activation a of every BN layer, the batch mean / var / inv / shift, the global
// maximum's rows.  RECOMPUTED: every ReLU mask of a BN layer (tb_pre(a, inv, shift) > 0, the forward's expression bit for
// bit) and xhat = (a - mean) * (1 / sqrt(var + eps)).  Batch statistics and the backward's two sums are per-chunk double
// partials added in a fixed order, no float atomics anywhere: two steps from the same state are bitwise identical.
//
// The grouped kernels take a [G][Rg][C] with constants [G][C] and partials part[(g * chunks + k) * C + c]; a dense layer is
// G = 1.  RB (tb_val): the activation is not stored but rebuilt as t1[g][r % p][c] + z[r / p][c] (AtlasNet's first decoder
// layer); everywhere else RB is false and z, p are not read.
//
// tb_bn_bwd_fc_kernel (rows = the batch's clouds, a few to a few hundred) works in double from the stored activation: with
// few rows g - mean(g) - xhat mean(g xhat) cancels almost completely (two rows: all but eps / (var + eps) of it), and xhat
// rounded to fp32 would decide what is left.  Its ReLU mask is still the forward's fp32 test.
#pragma once
#include "train_tile.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace geoadv {

__device__ __forceinline__ float tb_pre(float a, float inv, float shift) { return a * inv + shift; }

// The activation of group g, row r, column c.  RB: rebuilt as t1[g][r % p][c] + z[r / p][c].
template <bool RB>
__device__ __forceinline__ float tb_val(const float *a, const float *z, int g, int r, int c, int Rg, int C, int p) {
    if (RB) return a[((size_t)g * p + r % p) * C + c] + z[(size_t)(r / p) * C + c];
    return a[((size_t)g * Rg + r) * C + c];
}

// ---- column sums ------------------------------------------------------------------------------------------------------------
// Column partials over a chunk of rows in double, fixed order: MODE 0 = (sum a, sum a^2), MODE 1 = (sum a, 0).
// grid (ceil(C / 64), chunks, G), block 256 = 64 columns x 4 row phases.
template <int MODE>
static __global__ __launch_bounds__(256) void tb_colsum_kernel(const float *a, int Rg, int C, int rpc, double2 *part) {
    __shared__ double2 red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6, g = blockIdx.z;
    const int r0 = blockIdx.y * rpc, r1 = min(Rg, r0 + rpc);
    double s = 0.0, q = 0.0;
    if (c < C)
        for (int r = r0 + ph; r < r1; r += 4) {
            const double v = (double)a[((size_t)g * Rg + r) * C + c];
            s += v;
            if (MODE == 0) q += v * v;
        }
    red[ph][threadIdx.x & 63] = make_double2(s, q);
    __syncthreads();
    if (ph == 0 && c < C) {
        double2 o = red[0][threadIdx.x];
        for (int p = 1; p < 4; ++p) { o.x += red[p][threadIdx.x].x; o.y += red[p][threadIdx.x].y; }
        part[((size_t)g * gridDim.y + blockIdx.y) * C + c] = o;
    }
}

// Column sums -> a gradient vector (conv / fc bias): out[g][c] = sum of the partials' .x, fixed order.
static __global__ __launch_bounds__(256) void tb_colsum_final_kernel(const double2 *part, int chunks, int C, int G, float *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G * C) return;
    const int g = e / C, c = e - g * C;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[((size_t)g * chunks + k) * C + c].x;
    out[e] = (float)s;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------
// Batch statistics from the partials: mean, biased variance, folded constants.  One thread per (group, column).
static __global__ __launch_bounds__(256) void tb_bn_stats_kernel(const double2 *part, int chunks, int C, int G, double inv_rows,
                                                                 const float *gamma, const float *beta, float eps, float *mean,
                                                                 float *var, float *inv, float *shift) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G * C) return;
    const int g = e / C, c = e - g * C;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < chunks; ++k) { const double2 v = part[((size_t)g * chunks + k) * C + c]; s += v.x; q += v.y; }
    const double m = s * inv_rows;
    double v = q * inv_rows - m * m;
    if (v < 0.0) v = 0.0;
    const float mf = (float)m, vf = (float)v;
    const float iv = gamma[e] * (1.0f / sqrtf(vf + eps));
    mean[e] = mf; var[e] = vf; inv[e] = iv; shift[e] = beta[e] - mf * iv;
}

// y = relu(a * inv + shift), a [G][Rg][C], constants [G][C]
template <bool RB>
static __global__ __launch_bounds__(256) void tb_bn_relu_kernel(const float *a, const float *z, size_t total, int Rg, int C, int p,
                                                                const float *inv, const float *shift, float *y) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const size_t gr = e / C;
    const int g = (int)(gr / Rg), r = (int)(gr % Rg);
    y[e] = fmaxf(tb_pre(tb_val<RB>(a, z, g, r, c, Rg, C, p), inv[g * C + c], shift[g * C + c]), 0.f);
}

// Max over the n rows of each cloud of a * inv + shift (no ReLU): the maximum and its FIRST row.  grid (ceil(C / 64), B).
static __global__ __launch_bounds__(256) void tb_gmax_kernel(const float *a, int n, int C, const float *inv, const float *shift,
                                                             float *pooled, int *arg) {
    __shared__ float mv[4][64];
    __shared__ int mi[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6, b = blockIdx.y;
    float best = -INFINITY;
    int bi = 0;
    if (c < C) {
        const float iv = inv[c], sh = shift[c];
        if (ph < n) best = tb_pre(a[((size_t)b * n + ph) * C + c], iv, sh), bi = ph;
        for (int r = ph + 4; r < n; r += 4) {
            const float v = tb_pre(a[((size_t)b * n + r) * C + c], iv, sh);
            if (v > best) { best = v; bi = r; }
        }
    }
    mv[ph][threadIdx.x & 63] = best;
    mi[ph][threadIdx.x & 63] = bi;
    __syncthreads();
    if (ph == 0 && c < C) {
        for (int p = 1; p < 4 && p < n; ++p) {
            const float v = mv[p][threadIdx.x];
            const int i = mi[p][threadIdx.x];
            if (v > best || (v == best && i < bi)) { best = v; bi = i; }
        }
        pooled[(size_t)b * C + c] = best;
        arg[(size_t)b * C + c] = bi;
    }
}

// out = sum d1 / c1 + sum d2 / c2 (the Chamfer loss of two distance vectors): one block, strided double sums added in a fixed order
static __global__ __launch_bounds__(256) void tb_loss_kernel(const float *d1, size_t c1, const float *d2, size_t c2, float *out) {
    __shared__ double r1[256], r2[256];
    double s = 0.0, q = 0.0;
    for (size_t e = threadIdx.x; e < c1; e += 256) s += (double)d1[e];
    for (size_t e = threadIdx.x; e < c2; e += 256) q += (double)d2[e];
    r1[threadIdx.x] = s; r2[threadIdx.x] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < 256; ++i) { a += r1[i]; b += r2[i]; }
        out[0] = (float)(a / (double)c1 + b / (double)c2);
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------
// BN backward of a ReLU layer, dense dy:  g = dy * [a * inv + shift > 0].  Pass 1: (sum g, sum g * xhat) per chunk and group.
template <bool RB>
static __global__ __launch_bounds__(256) void tb_bn_bwd_part_kernel(const float *dy, const float *a, const float *z, int Rg, int C, int p,
                                                                    int rpc, const float *mean, const float *var, const float *inv,
                                                                    const float *shift, float eps, double2 *part) {
    __shared__ double2 red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6, g = blockIdx.z;
    const int r0 = blockIdx.y * rpc, r1 = min(Rg, r0 + rpc);
    double s = 0.0, q = 0.0;
    if (c < C) {
        const int k = g * C + c;
        const float rs = 1.0f / sqrtf(var[k] + eps), m = mean[k], iv = inv[k], sh = shift[k];
        for (int r = r0 + ph; r < r1; r += 4) {
            const float av = tb_val<RB>(a, z, g, r, c, Rg, C, p);
            const float gv = tb_pre(av, iv, sh) > 0.f ? dy[((size_t)g * Rg + r) * C + c] : 0.f;
            s += (double)gv;
            q += (double)gv * (double)((av - m) * rs);
        }
    }
    red[ph][threadIdx.x & 63] = make_double2(s, q);
    __syncthreads();
    if (ph == 0 && c < C) {
        double2 o = red[0][threadIdx.x];
        for (int pp = 1; pp < 4; ++pp) { o.x += red[pp][threadIdx.x].x; o.y += red[pp][threadIdx.x].y; }
        part[((size_t)g * gridDim.y + blockIdx.y) * C + c] = o;
    }
}

// Pass 1 of a BN without ReLU under the global maximum, whose g is dpool at the maximum's row of each (cloud, channel): clouds
// in ascending order, the totals written as a single chunk.
static __global__ __launch_bounds__(256) void tb_bn_bwd_gmax_part_kernel(const float *dpool, const int *arg, const float *a, int B, int n,
                                                                         int C, const float *mean, const float *var, float eps,
                                                                         double2 *part) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float rs = 1.0f / sqrtf(var[c] + eps), m = mean[c];
    double s = 0.0, q = 0.0;
    for (int b = 0; b < B; ++b) {
        const float av = a[((size_t)b * n + arg[(size_t)b * C + c]) * C + c];
        const float gv = dpool[(size_t)b * C + c];
        s += (double)gv;
        q += (double)gv * (double)((av - m) * rs);
    }
    part[c] = make_double2(s, q);
}

// Pass 2: dbeta, dgamma (into the gradient arena) and the means m1 = dbeta / rows, m2 = dgamma / rows, per (group, column)
static __global__ __launch_bounds__(256) void tb_bn_bwd_final_kernel(const double2 *part, int chunks, int C, int G, double inv_rows,
                                                                     float *dgamma, float *dbeta, float *m1, float *m2) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= G * C) return;
    const int g = e / C, c = e - g * C;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < chunks; ++k) { const double2 v = part[((size_t)g * chunks + k) * C + c]; s += v.x; q += v.y; }
    dbeta[e] = (float)s; dgamma[e] = (float)q;
    m1[e] = (float)(s * inv_rows); m2[e] = (float)(q * inv_rows);
}

// Pass 3: da = gamma * rs * (g - m1 - xhat * m2), dense dy through the ReLU.  BN false (no batch norm): da = g.
template <bool RB, bool BN>
static __global__ __launch_bounds__(256) void tb_bn_bwd_apply_kernel(const float *dy, const float *a, const float *z, size_t total, int Rg,
                                                                     int C, int p, const float *mean, const float *var, const float *gamma,
                                                                     const float *inv, const float *shift, const float *m1,
                                                                     const float *m2, float eps, float *da) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const size_t gr = e / C;
    const int g = (int)(gr / Rg), r = (int)(gr % Rg), k = g * C + c;
    const float av = tb_val<RB>(a, z, g, r, c, Rg, C, p);
    const float gv = tb_pre(av, inv[k], shift[k]) > 0.f ? dy[e] : 0.f;
    if (!BN) { da[e] = gv; return; }
    const float rs = 1.0f / sqrtf(var[k] + eps);
    const float xh = (av - mean[k]) * rs;
    da[e] = gamma[k] * rs * (gv - m1[k] - xh * m2[k]);
}

// Pass 3 under the global maximum: da = gamma * rs * ([row is the maximum's] dpool - m1 - xhat * m2)
static __global__ __launch_bounds__(256) void tb_bn_bwd_gmax_apply_kernel(const float *dpool, const int *arg, const float *a, size_t total,
                                                                          int n, int C, const float *mean, const float *var,
                                                                          const float *gamma, const float *m1, const float *m2, float eps,
                                                                          float *da) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const size_t r = e / C, b = r / n;
    const float gv = arg[b * C + c] == (int)(r - b * n) ? dpool[b * C + c] : 0.f;
    const float rs = 1.0f / sqrtf(var[c] + eps);
    const float xh = (a[e] - mean[c]) * rs;
    da[e] = gamma[c] * rs * (gv - m1[c] - xh * m2[c]);
}

// BN backward of an fc layer, one thread per column, all three passes in double (see the header).
static __global__ __launch_bounds__(256) void tb_bn_bwd_fc_kernel(const float *dy, const float *a, int R, int C, const float *gamma,
                                                                  const float *inv, const float *shift, float eps, float *dgamma,
                                                                  float *dbeta, float *da) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double m = 0.0, v = 0.0;
    for (int r = 0; r < R; ++r) m += (double)a[(size_t)r * C + c];
    m /= R;
    for (int r = 0; r < R; ++r) { const double d = (double)a[(size_t)r * C + c] - m; v += d * d; }
    v /= R;
    const double rs = 1.0 / sqrt(v + (double)eps);
    const float iv = inv[c], sh = shift[c];
    double s = 0.0, q = 0.0;
    for (int r = 0; r < R; ++r) {
        const size_t e = (size_t)r * C + c;
        const double gv = tb_pre(a[e], iv, sh) > 0.f ? (double)dy[e] : 0.0;
        s += gv;
        q += gv * (((double)a[e] - m) * rs);
    }
    dbeta[c] = (float)s; dgamma[c] = (float)q;
    const double m1 = s / R, m2 = q / R, gr = (double)gamma[c] * rs;
    for (int r = 0; r < R; ++r) {
        const size_t e = (size_t)r * C + c;
        const double gv = tb_pre(a[e], iv, sh) > 0.f ? (double)dy[e] : 0.0;
        da[e] = (float)(gr * (gv - m1 - ((double)a[e] - m) * rs * m2));
    }
}

// ---- optimizer, running statistics ----------------------------------------------------------------------------------------
// torch.optim.Adam (betas .9 / .999, eps 1e-8); bc1 = 1 - beta1^t, bc2s = sqrt(1 - beta2^t).  DECAY: g += wd * p first.
// (Without weight decay the term is not formed at all: g + 0 * p is not g for a negative-zero g or a non-finite p.)
template <bool DECAY>
static __global__ __launch_bounds__(256) void tb_adam_kernel(float *p, float *m, float *v, const float *g, size_t count, float lr, float wd,
                                                             float bc1, float bc2s) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float gv = DECAY ? g[e] + wd * p[e] : g[e];
    const float mn = m[e] + (gv - m[e]) * (1.f - 0.9f);
    const float vn = v[e] * 0.999f + (gv * gv) * (1.f - 0.999f);
    m[e] = mn; v[e] = vn;
    const float denom = sqrtf(vn) / bc2s + 1e-8f;
    p[e] = p[e] - (lr / bc1) * (mn / denom);
}

// running = 0.9 running + 0.1 stat * scale (scale = rows / (rows - 1) for the variance, null for the mean)
static __global__ __launch_bounds__(256) void tb_running_kernel(float *running, const float *stat, const float *scale, size_t count) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    const float s = scale ? stat[e] * scale[e] : stat[e];
    running[e] = running[e] * (1.f - 0.1f) + 0.1f * s;
}

// ---- host plumbing ----------------------------------------------------------------------------------------------------------
// A handle's device memory: hipMalloc of count elements (+ 16 bytes), zero filled, recorded in `allocs`.  After a failure
// (err set) nothing more is allocated or uploaded; dev_free_all releases what was.
template <class T> T *dev_alloc(std::vector<void *> &allocs, size_t count, hipError_t &err) {
    void *p = nullptr;
    if (err == hipSuccess) err = hipMalloc(&p, count * sizeof(T) + 16);
    if (err == hipSuccess) { allocs.push_back(p); err = hipMemset(p, 0, count * sizeof(T) + 16); }
    return static_cast<T *>(p);
}
inline void dev_free_all(std::vector<void *> &allocs) {
    for (void *p : allocs) (void)hipFree(p);
    allocs.clear();
}
inline void dev_upload(float *dst, const std::vector<float> &src, hipError_t &err) {
    if (err == hipSuccess) err = hipMemcpy(dst, src.data(), sizeof(float) * src.size(), hipMemcpyHostToDevice);
}
// What a *_trainer_create returns after a HIP failure (the caller has deleted its handle, which frees the device memory)
inline int train_create_error(const char *who, hipError_t err) {
    set_error("%s: %s", who, hipGetErrorString(err));
    return err == hipErrorOutOfMemory ? GEOADV_ENOMEM : GEOADV_EHIP;
}

inline unsigned blocks_of(size_t total) { return (unsigned)((total + 255) / 256); }
inline int rpc_of(int R) { return std::max(1, std::min(R, 256)); }     // rows per chunk of the column sums

// ---- the parameter arena ----------------------------------------------------------------------------------------------------
// One layer of a trainer: `groups` independent kin x kout products (AtlasNet's primitives; 1 elsewhere) over `rows` rows per
// group.  bn: a batch norm follows (gamma and beta in the arena, a slot in the batch-norm arenas).  mv_slot: a slot in the
// batch-norm arenas even without a norm (AtlasNet's decoder without norms: identity constants, inv 1 shift 0).
struct TrainLayer { int kin, kout, groups, rows; bool bn, mv_slot; };
constexpr int TA_MAXL = 20;
// The initial weights and moving statistics of every layer, as host pointers (the last four are read for bn layers only)
struct TrainInit { const float *w[TA_MAXL], *b[TA_MAXL], *gamma[TA_MAXL], *beta[TA_MAXL], *mean[TA_MAXL], *var[TA_MAXL]; };
enum { TA_BAT_MEAN = 0, TA_BAT_VAR, TA_RUN_MEAN, TA_RUN_VAR, TA_INV, TA_SHIFT, TA_SLOT1, TA_SLOT2 };     // TrainArena::view

// The flat buffers of a layer-by-layer trainer; every handle derives from it and is created with `new T()` (zeroed).
// params / grads / slot1 / slot2 hold P floats: per layer W [groups][kin][kout] at o_w, b at o_b, gamma at o_g, beta at o_be,
// each rounded up to 16 floats.  The batch-norm arenas hold MV floats, [groups][kout] per slot at o_mv: running (moving) and
// batch statistics, the folded constants inv / shift, the backward's means m1 / m2 and, where allocated, unbias = rows /
// (rows - 1).  The slots of the layers with a real norm come first: MVbn floats.  Layers without a slot have offset 0.
struct TrainArena {
    int nl;                                        // layers in use, <= TA_MAXL
    TrainLayer layer[TA_MAXL];
    size_t o_w[TA_MAXL], o_b[TA_MAXL], o_g[TA_MAXL], o_be[TA_MAXL], o_mv[TA_MAXL], P, MV, MVbn;
    std::vector<void *> allocs;                    // every device buffer of the handle, the model's own included
    float *params, *grads, *slot1, *slot2;         // slot1 = Adam m / Momentum accum, slot2 = Adam v
    float *run_mean, *run_var, *bat_mean, *bat_var, *inv, *shift, *m1, *m2, *unbias;

    ~TrainArena() { dev_free_all(allocs); }
    int kin(int l) const { return layer[l].kin; }
    int kout(int l) const { return layer[l].kout; }
    int groups(int l) const { return layer[l].groups; }
    size_t width(int l) const { return (size_t)layer[l].groups * layer[l].kout; }

    void lay_out(const TrainLayer *table, int layers) {
        auto rup16 = [](size_t v) { return (v + 15) / 16 * 16; };
        nl = layers; P = MV = MVbn = 0;
        for (int l = 0; l < nl; ++l) {
            layer[l] = table[l];
            const size_t C = width(l);
            o_w[l] = P; P = rup16(P + C * kin(l));
            o_b[l] = P; P = rup16(P + C);
            o_g[l] = o_be[l] = o_mv[l] = 0;
            if (layer[l].bn) {
                o_g[l] = P; P = rup16(P + C);
                o_be[l] = P; P = rup16(P + C);
            }
            if (layer[l].bn || layer[l].mv_slot) { o_mv[l] = MV; MV = rup16(MV + C); }
            if (layer[l].bn) MVbn = MV;
        }
    }
    void alloc(bool with_unbias, hipError_t &err) {
        for (float **p : {&params, &grads, &slot1, &slot2}) *p = dev_alloc<float>(allocs, P, err);
        for (float **p : {&run_mean, &run_var, &bat_mean, &bat_var, &inv, &shift, &m1, &m2}) *p = dev_alloc<float>(allocs, MV, err);
        if (with_unbias) unbias = dev_alloc<float>(allocs, MV, err);
    }
    void upload(const TrainInit &in, hipError_t &err) {
        if (err != hipSuccess) return;
        std::vector<float> hp(P, 0.f), hm(MV, 0.f), hv(MV, 0.f), hu(MV, 1.f);
        bool identity = false;
        for (int l = 0; l < nl; ++l) {
            const size_t C = width(l);
            identity = identity || layer[l].mv_slot;
            memcpy(&hp[o_w[l]], in.w[l], sizeof(float) * C * kin(l));
            memcpy(&hp[o_b[l]], in.b[l], sizeof(float) * C);
            if (!layer[l].bn) continue;
            memcpy(&hp[o_g[l]], in.gamma[l], sizeof(float) * C);
            memcpy(&hp[o_be[l]], in.beta[l], sizeof(float) * C);
            memcpy(&hm[o_mv[l]], in.mean[l], sizeof(float) * C);
            memcpy(&hv[o_mv[l]], in.var[l], sizeof(float) * C);
            const double rl = (double)layer[l].rows;
            if (unbias) std::fill_n(&hu[o_mv[l]], C, (float)(rl / (rl - 1.0)));
        }
        dev_upload(params, hp, err); dev_upload(run_mean, hm, err); dev_upload(run_var, hv, err);
        if (unbias) dev_upload(unbias, hu, err);
        if (identity) dev_upload(inv, std::vector<float>(MV, 1.f), err);
    }
    int set_slots(const float *s1, const float *s2) {
        if (s1) GA_HIP(hipMemcpy(slot1, s1, sizeof(float) * P, hipMemcpyHostToDevice));
        if (s2) GA_HIP(hipMemcpy(slot2, s2, sizeof(float) * P, hipMemcpyHostToDevice));
        return GEOADV_OK;
    }
    void buffers(float **params_out, float **grads_out, size_t *count) const {
        if (params_out) *params_out = params;
        if (grads_out) *grads_out = grads;
        if (count) *count = P;
    }
    // offsets[4 l ...] = o_w, o_b, o_g, o_be and moving[l] = o_mv of layers 0 .. maxl; (size_t)-1 for what a layer does not have
    void export_layout(size_t *offsets, size_t *moving, int maxl) const {
        for (int l = 0; l < maxl; ++l) {
            const bool have = l < nl, bn = have && layer[l].bn;
            offsets[4 * l] = have ? o_w[l] : (size_t)-1;
            offsets[4 * l + 1] = have ? o_b[l] : (size_t)-1;
            offsets[4 * l + 2] = bn ? o_g[l] : (size_t)-1;
            offsets[4 * l + 3] = bn ? o_be[l] : (size_t)-1;
            if (moving) moving[l] = bn ? o_mv[l] : (size_t)-1;
        }
    }
    // The TA_* array of layer l (the caller has checked that the layer has a slot), or a whole optimizer slot
    void view(int which, int l, const void **ptr, size_t *count) const {
        if (which >= TA_SLOT1) { *ptr = which == TA_SLOT1 ? slot1 : slot2; *count = P; return; }
        const float *base[] = {bat_mean, bat_var, run_mean, run_var, inv, shift};
        *ptr = base[which] + o_mv[l]; *count = width(l);
    }
};

// The stream of a step and its sticky error: after the first failure nothing more is launched and `err` stays the first.
struct Launch {
    hipStream_t st;
    hipError_t err = hipSuccess;

    bool ok() const { return err == hipSuccess; }
    void check() { if (err == hipSuccess) err = hipGetLastError(); }
    template <class... P, class... A> void launch(void (*kernel)(P...), dim3 grid, dim3 block, A... args) {
        if (err != hipSuccess) return;
        hipLaunchKernelGGL(kernel, grid, block, 0, st, static_cast<P>(args)...);
        check();
    }
    void gemm(const GemmArgs &g, float *partials) { if (err == hipSuccess) err = ct_launch_gemm(g, partials, st); }

    template <int MODE> void colsum(const float *a, int Rg, int C, int G, int rpc, double2 *part) {
        launch(tb_colsum_kernel<MODE>, dim3(cdiv(C, 64), cdiv(Rg, rpc), G), dim3(256), a, Rg, C, rpc, part);
    }
    // Batch statistics of a [G][Rg][C] and the folded constants
    void bn_batch_stats(const float *a, int Rg, int C, int G, double2 *part, const float *gamma, const float *beta, float eps, float *mean,
                     float *var, float *inv, float *shift) {
        const int rpc = rpc_of(Rg);
        colsum<0>(a, Rg, C, G, rpc, part);
        launch(tb_bn_stats_kernel, dim3(cdiv(G * C, 256)), dim3(256), part, cdiv(Rg, rpc), C, G, 1.0 / Rg, gamma, beta, eps, mean, var, inv,
               shift);
    }
    // db[g][c] = the column sums of da [G][Rg][C]
    void bias_colsum(const float *da, int Rg, int C, int G, double2 *part, float *db) {
        const int rpc = rpc_of(Rg);
        colsum<1>(da, Rg, C, G, rpc, part);
        launch(tb_colsum_final_kernel, dim3(cdiv(G * C, 256)), dim3(256), part, cdiv(Rg, rpc), C, G, db);
    }
};

// A step on an arena: the batch norm's eps and the two scratch buffers of the column sums and of the split-K.
struct TrainRun : Launch {
    TrainArena *A;
    float eps;
    double2 *part;
    float *partials;

    void gemm(const GemmArgs &g) { Launch::gemm(g, partials); }
    float *W(int l) const { return A->params + A->o_w[l]; }
    // Batch statistics of layer l's pre-BN activation a
    void batch_stats(int l, const float *a) {
        const size_t o = A->o_mv[l];
        bn_batch_stats(a, A->layer[l].rows, A->kout(l), A->groups(l), part, A->params + A->o_g[l], A->params + A->o_be[l], eps, A->bat_mean + o,
                       A->bat_var + o, A->inv + o, A->shift + o);
    }
    // d bias = the column sums of da over the layer's rows
    void bias_grad(int l, const float *da) { bias_colsum(da, A->layer[l].rows, A->kout(l), A->groups(l), part, A->grads + A->o_b[l]); }

    // The products of a dense layer on rows k0 .. k0 + K of W_l (N = kout):  out = in @ W (+ b_l) with in [M][K]
    GemmArgs fwd_args(int l, const float *in, float *out, int M, int k0, int K, bool bias) const {
        const int N = A->kout(l);
        GemmArgs g{};
        g.A = in; g.sAi = K; g.sAk = 1;
        g.B = W(l) + (size_t)k0 * N; g.sBk = N; g.sBj = 1;
        g.C = out; g.ldc = N;
        g.bias = bias ? A->params + A->o_b[l] : nullptr;
        g.alpha = 1.f; g.M = M; g.N = N; g.K = K; g.batch = 1;
        return g;
    }
    // dW = in^T da:  A(i = input channel, k = row) = in[row][i]
    GemmArgs wgrad_args(int l, const float *in, const float *da, int M, int k0, int K) const {
        const int N = A->kout(l);
        GemmArgs g{};
        g.A = in; g.sAi = 1; g.sAk = K;
        g.B = da; g.sBk = N; g.sBj = 1;
        g.C = A->grads + A->o_w[l] + (size_t)k0 * N; g.ldc = N;
        g.alpha = 1.f; g.M = K; g.N = N; g.K = M; g.batch = 1;
        return g;
    }
    // din (=|+=) da W^T:  B(k = output channel, j = input channel) = W[j][k]
    GemmArgs igrad_args(int l, const float *da, float *din, int M, int k0, int K, int accumulate) const {
        const int N = A->kout(l);
        GemmArgs d{};
        d.A = da; d.sAi = N; d.sAk = 1;
        d.B = W(l) + (size_t)k0 * N; d.sBk = 1; d.sBj = N;
        d.C = din; d.ldc = K;
        d.alpha = 1.f; d.M = M; d.N = K; d.K = N; d.batch = 1; d.accumulate = accumulate;
        return d;
    }
    // The tail of a torch-form step: torch.optim.Adam's step number step + 1 on the whole arena, then the running statistics
    template <bool DECAY> int adam_and_running(float lr, float wd, long long step) {
        const double tt = (double)(step + 1);
        const float bc1 = (float)(1.0 - pow(0.9, tt)), bc2s = (float)sqrt(1.0 - pow(0.999, tt));
        hipLaunchKernelGGL(tb_adam_kernel<DECAY>, dim3(blocks_of(A->P)), dim3(256), 0, st, A->params, A->slot1, A->slot2, A->grads, A->P, lr, wd,
                           bc1, bc2s);
        GA_LAUNCH_CHECK();
        const size_t mv = A->MVbn;
        hipLaunchKernelGGL(tb_running_kernel, dim3(blocks_of(mv)), dim3(256), 0, st, A->run_mean, A->bat_mean, (const float *)nullptr, mv);
        GA_LAUNCH_CHECK();
        hipLaunchKernelGGL(tb_running_kernel, dim3(blocks_of(mv)), dim3(256), 0, st, A->run_var, A->bat_var, A->unbias, mv);
        GA_LAUNCH_CHECK();
        return GEOADV_OK;
    }
};

}  // namespace geoadv
