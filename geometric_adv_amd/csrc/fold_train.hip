// geoadv_fold_trainer: one TRAINING step of the FoldingNet auto-encoder (transfer/foldingnet/train_foldingnet.py:76-117:
// FoldingNet_graph in train mode, ChamferLoss(points, recon), torch.optim.Adam with weight decay) on gfx950, fp32 in and out.
//
// Graph (foldingnet.py): in = cat(xyz, cov) 12 wide; conv1..conv3 (64) each BN + ReLU; graph pool 1 + ReLU; conv4 (128) BN
// ReLU; graph pool 2 + ReLU; conv5 (1024) BN, NO ReLU; max over points; fc1 (512) BN ReLU; fc2 (512) = the code; fold1 on
// [code, grid] 514 -> 512 -> 512 -> 3 (ReLU, no BN) = mid; fold2 on [code, mid] 515 -> 512 -> 512 -> 3 = recon.
// BatchNorm1d in train mode: eps 1e-5, the BIASED batch variance normalises (bn1..5 over batch * n rows, bn6 over the batch
// clouds), running = 0.9 running + 0.1 batch with the UNBIASED variance.  The graph (16-NN, covariance, symmetric adjacency)
// and the picks of both pools come from foldingnet.hip's kernels (fold_graph.h), the Chamfer scan and its gradient from
// geoadv_nn_distance / geoadv_nn_distance_grad.
//
// FORM: the direct one, as cls_train.hip, on the GEMM of train_tile.h and the batch-norm, global-max, loss, Adam and
// running-statistics kernels of train_bn.h (what is stored, what is recomputed and why the fc layer's backward is in double:
// there).  STORED besides: the post-ReLU outputs of conv1..conv4 and of the four hidden decoder layers, both pools' outputs
// and winners.  Two steps from the same state are bitwise identical.
//
// Decoder: the 512 code rows of each fold's first layer act once per cloud, s = code . W[0:512] + b; per grid point only the
// 2 (grid) or 3 (mid) point rows are added.  Backward, d s = the column sums of d pre over the cloud's 2025 points, then
// d code = d s . W[0:512]^T and d W[0:512] = code^T d s: products of batch rows, not batch * 2025.
//
// Pool backward (the reference's Graph_Pooling cannot be differentiated at batch > 1; this is the derivative of what its
// forward computes): every (point, channel) of a pool sends its gradient to the ONE element that attained the maximum --
// the point itself first, then the lowest of the 16 pick slots (strict > in that order) -- and only if that maximum is
// positive (the ReLU that follows; the pools' inputs are ReLU outputs, so a maximum is positive or zero).  Gathered by
// destination: point j adds, in ascending order of i over its sorted adjacency row (the adjacency is symmetric, so every
// i that can have picked j is there), the gradients of the (i, channel) whose winner is j.
// conv5's BN has no ReLU and gamma may be negative: the maximum over points is taken of a * inv + shift itself, and the
// first maximal row gets the gradient.
//
// Adam (torch.optim.Adam, lr, betas .9 / .999, eps 1e-8, weight_decay): g += wd * p on EVERY parameter; m += (g - m) * 0.1;
// v = 0.999 v + 0.001 g g; p -= lr / (1 - 0.9^t) * m / (sqrt(v) / sqrt(1 - 0.999^t) + eps), t = steps taken including this.
#include "train_bn.h"
#include "fold_graph.h"

namespace geoadv {

constexpr float FT_EPS = 1e-5f;
constexpr int FT_NB = 16, FT_GRID = 45, FT_G2 = FT_GRID * FT_GRID, FT_CODE = 512, FT_LAT = 1024;

// in[r][0:3] = xyz, in[r][3:12] = cov
__global__ __launch_bounds__(256) void ft_input_kernel(const float *x, const float *cov, int R, float *in) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= R * 12) return;
    const int r = e / 12, k = e - 12 * r;
    in[e] = k < 3 ? x[(size_t)r * 3 + k] : cov[(size_t)r * 9 + k - 3];
}

// Graph pool + ReLU of h [B n][C]: g = relu(max(h_i, h over the 16 columns)); win = the row (in the cloud) that attained a
// positive maximum -- the point itself first, then the lowest slot -- or -1.
__global__ __launch_bounds__(256) void ft_graph_pool_kernel(const float *h, const int *cols, int n, int C, size_t total, float *g, int *win) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const size_t r = e / C;
    const size_t base = r / n * n;
    float v = h[e];
    int w = (int)(r - base);
    const int *cl = cols + r * FT_NB;
#pragma unroll 4
    for (int t = 0; t < FT_NB; ++t) {
        const int j = (unsigned)cl[t] < (unsigned)n ? cl[t] : 0;
        const float u = h[(base + j) * C + c];
        if (u > v) { v = u; w = j; }
    }
    const bool pos = v > 0.f;
    g[e] = pos ? v : 0.f;
    win[e] = pos ? w : -1;
}

// A fold's first layer: H[r][k] = relu(s[cloud(r)][k] + sum_d pts[r][d] * wp[d][k]), D = 2 (the grid) or 3 (mid)
template <int D>
__global__ __launch_bounds__(256) void ft_fold_l1_kernel(const float *s, const float *pts, const float *wp, size_t total, float *H) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int k = (int)(e % FT_CODE);
    const size_t r = e / FT_CODE;
    float v = s[r / FT_G2 * FT_CODE + k];
#pragma unroll
    for (int d = 0; d < D; ++d) v = fmaf(wp[d * FT_CODE + k], pts[r * D + d], v);
    H[e] = fmaxf(v, 0.f);
}

__global__ __launch_bounds__(256) void ft_relu_kernel(float *y, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) y[e] = fmaxf(y[e], 0.f);
}

// d = H > 0 ? d : 0 (the backward of a ReLU whose output H was stored)
__global__ __launch_bounds__(256) void ft_mask_kernel(float *d, const float *H, size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e < total) d[e] = H[e] > 0.f ? d[e] : 0.f;
}

// Pool backward, gathered by destination: dh[j][c] = [win[j][c] == j] dg[j][c] + sum over i != j in j's sorted adjacency row,
// ascending, of [win[i][c] == j] dg[i][c].
__global__ __launch_bounds__(256) void ft_pool_bwd_kernel(const float *dg, const int *win, const int *off, const int *deg, const int *col,
                                                          int n, int C, size_t total, float *dh) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % C);
    const size_t r = e / C;
    const size_t cloud = r / n, base = cloud * n;
    const int j = (int)(r - base);
    float s = win[e] == j ? dg[e] : 0.f;
    const int *row = col + cloud * 32 * n + off[r];
    const int d = deg[r];
    for (int p = 0; p < d; ++p) {
        const int i = row[p];
        if ((unsigned)i >= (unsigned)n || i == j) continue;
        const size_t f = (base + i) * C + c;
        if (win[f] == j) s += dg[f];
    }
    dh[e] = s;
}

// out[k][c] = (float) part[k][c].x: the per-chunk column sums as a matrix (chunk = cloud)
__global__ __launch_bounds__(256) void ft_part_rows_kernel(const double2 *part, int count, float *out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < count) out[e] = (float)part[e].x;
}

}  // namespace geoadv

using namespace geoadv;

namespace {
// layers: conv1..conv5, fc1, fc2 (encoder), fold1.conv1..3, fold2.conv1..3
enum { E1 = 0, E2, E3, E4, E5, F1, F2, D0, D1, D2, D3, D4, D5, NL };
const int kIn[NL] = {12, 64, 64, 64, 128, FT_LAT, FT_CODE, FT_CODE + 2, 512, 512, FT_CODE + 3, 512, 512};
const int kOut[NL] = {64, 64, 64, 128, FT_LAT, FT_CODE, FT_CODE, 512, 512, 3, 512, 512, 3};
bool bn_of(int l) { return l <= F1; }
static_assert(NL <= TA_MAXL && GEOADV_FOLD_STATE_BN_MEAN == TA_BAT_MEAN && GEOADV_FOLD_STATE_BN_VAR == TA_BAT_VAR &&
              GEOADV_FOLD_STATE_RUNNING_MEAN == TA_RUN_MEAN && GEOADV_FOLD_STATE_RUNNING_VAR == TA_RUN_VAR &&
              GEOADV_FOLD_STATE_BN_INV == TA_INV && GEOADV_FOLD_STATE_BN_SHIFT == TA_SHIFT,
              "geoadv_fold_trainer_state passes these to TrainArena::view as they are");

// The one launch of each pool kernel and of the global maximum: the step (Run) and the geoadv_fold_train_pool / _pool_grad /
// _gmax entries all go through these.  rows = b * n.
void ft_launch_graph_pool(Launch &q, const float *h, const int *cols, size_t rows, int n, int C, float *g, int *win) {
    const size_t total = rows * C;
    q.launch(ft_graph_pool_kernel, dim3(blocks_of(total)), dim3(256), h, cols, n, C, total, g, win);
}
void ft_launch_pool_bwd(Launch &q, const float *dg, const int *win, const int *off, const int *deg, const int *col, size_t rows, int n, int C,
                        float *dh) {
    const size_t total = rows * C;
    q.launch(ft_pool_bwd_kernel, dim3(blocks_of(total)), dim3(256), dg, win, off, deg, col, n, C, total, dh);
}
void ft_launch_gmax(Launch &q, const float *a, int B, int n, int C, const float *inv, const float *shift, float *pooled, int *arg) {
    q.launch(tb_gmax_kernel, dim3(cdiv(C, 64), B), dim3(256), a, n, C, inv, shift, pooled, arg);
}
}  // namespace

struct geoadv_fold_trainer : TrainArena {
    int B, n, R, rows;                             // rows = B * 2025
    float lr, wd;
    long long step, ordinal;
    unsigned long long seed;
    float *in0, *a[6], *h[4], *g1, *g2, *pooled, *h6, *code, *s, *H[4], *mid, *recon, *grid;
    int *win1, *win2, *arg, *picks;
    float *d1, *d2, *gd1, *gd2, *dx, *drecon, *dmid, *loss, *mid_loss;
    int *i1, *i2;
    float *X, *Y, *Z, *ds, *dcode, *dsm1, *dsm2, *partials;
    double2 *part;
    void *graph_ws;
    FoldTrainGraph graph;
};

namespace {
struct Run : TrainRun {
    geoadv_fold_trainer *t;

    int rows(int l) const { return t->layer[l].rows; }
    // out = in @ W_l[k0 : k0 + K] + (bias ? b_l : 0)
    void linear_fwd(int l, const float *in, float *out, int M, int k0, int K, bool bias) { gemm(fwd_args(l, in, out, M, k0, K, bias)); }
    void bn_relu(int l, float *y) {
        const size_t total = (size_t)rows(l) * kOut[l], o = t->o_mv[l];
        launch(tb_bn_relu_kernel<false>, dim3(blocks_of(total)), dim3(256), t->a[l], nullptr, total, rows(l), kOut[l], 0, t->inv + o,
               t->shift + o, y);
    }
    void bn_layer(int l, const float *in, float *y) {
        linear_fwd(l, in, t->a[l], rows(l), 0, kIn[l], true);
        batch_stats(l, t->a[l]);
        if (y) bn_relu(l, y);
    }
    void graph_pool(const float *h, int which, int C, float *g, int *win) {
        ft_launch_graph_pool(*this, h, t->graph.cols + (size_t)which * t->R * FT_NB, (size_t)t->R, t->n, C, g, win);
    }
    void relu(float *y, size_t total) { launch(ft_relu_kernel, dim3(blocks_of(total)), dim3(256), y, total); }
    void mask(float *d, const float *H, size_t total) { launch(ft_mask_kernel, dim3(blocks_of(total)), dim3(256), d, H, total); }
    // one fold forward: l0 = its first layer, pts [rows][D] the grid or mid, H1 / H2 its hidden outputs, out [rows][3]
    void fold_fwd(int l0, const float *pts, int D, float *H1, float *H2, float *out) {
        linear_fwd(l0, t->code, t->s, t->B, 0, FT_CODE, true);
        const size_t total = (size_t)t->rows * 512;
        const float *wp = W(l0) + (size_t)FT_CODE * 512;
        launch(D == 2 ? ft_fold_l1_kernel<2> : ft_fold_l1_kernel<3>, dim3(blocks_of(total)), dim3(256), t->s, pts, wp, total, H1);
        linear_fwd(l0 + 1, H1, H2, t->rows, 0, 512, true);
        relu(H2, total);
        linear_fwd(l0 + 2, H2, out, t->rows, 0, 512, true);
    }
    int chamfer(const float *x, const float *pc, float *out) {
        if (!ok()) return GEOADV_EHIP;
        if (int rc = geoadv_nn_distance(t->B, t->n, x, FT_G2, pc, t->d1, t->i1, t->d2, t->i2, st)) return rc;
        launch(tb_loss_kernel, dim3(1), dim3(256), t->d1, (size_t)t->R, t->d2, (size_t)t->rows, out);
        return GEOADV_OK;
    }

    // ---- backward pieces ----
    // dW_l[k0 : k0 + K] = in^T da (in [M][K])
    void weight_grad(int l, const float *in, const float *da, int M, int k0, int K) { gemm(wgrad_args(l, in, da, M, k0, K)); }
    // din (=|+=) da W_l[k0 : k0 + K]^T
    void input_grad(int l, const float *da, float *din, int M, int k0, int K, int accumulate) {
        gemm(igrad_args(l, da, din, M, k0, K, accumulate));
    }
    void linear_bwd(int l, const float *in, const float *da, float *din) {
        weight_grad(l, in, da, rows(l), 0, kIn[l]);
        bias_grad(l, da);
        if (din) input_grad(l, da, din, rows(l), 0, kIn[l], 0);
    }
    // BN backward of layer l; gmax: dy = dpool [B][C] at the maximum's rows (conv5), else dense dy through the ReLU
    void bn_bwd(int l, bool gmax, const float *dy, float *da) {
        const int R = rows(l), C = kOut[l];
        const size_t o = t->o_mv[l], total = (size_t)R * C;
        const float *mean = t->bat_mean + o, *var = t->bat_var + o, *iv = t->inv + o, *sh = t->shift + o, *gam = t->params + t->o_g[l];
        float *dgam = t->grads + t->o_g[l], *dbeta = t->grads + t->o_be[l];
        if (l == F1) {
            launch(tb_bn_bwd_fc_kernel, dim3(cdiv(C, 256)), dim3(256), dy, t->a[l], R, C, gam, iv, sh, FT_EPS, dgam, dbeta, da);
            return;
        }
        const int rpc = rpc_of(R), chunks = gmax ? 1 : cdiv(R, rpc);
        if (gmax)
            launch(tb_bn_bwd_gmax_part_kernel, dim3(cdiv(C, 256)), dim3(256), dy, t->arg, t->a[l], t->B, t->n, C, mean, var, FT_EPS, t->part);
        else
            launch(tb_bn_bwd_part_kernel<false>, dim3(cdiv(C, 64), chunks), dim3(256), dy, t->a[l], nullptr, R, C, 0, rpc, mean, var, iv, sh,
                   FT_EPS, t->part);
        launch(tb_bn_bwd_final_kernel, dim3(cdiv(C, 256)), dim3(256), t->part, chunks, C, 1, 1.0 / R, dgam, dbeta, t->m1 + o, t->m2 + o);
        if (gmax)
            launch(tb_bn_bwd_gmax_apply_kernel, dim3(blocks_of(total)), dim3(256), dy, t->arg, t->a[l], total, t->n, C, mean, var, gam,
                   t->m1 + o, t->m2 + o, FT_EPS, da);
        else
            launch(tb_bn_bwd_apply_kernel<false, true>, dim3(blocks_of(total)), dim3(256), dy, t->a[l], nullptr, total, R, C, 0, mean, var, gam,
                   iv, sh, t->m1 + o, t->m2 + o, FT_EPS, da);
    }
    void pool_bwd(const float *dg, const int *win, int C, float *dh) {
        ft_launch_pool_bwd(*this, dg, win, t->graph.off, t->graph.deg, t->graph.col, (size_t)t->R, t->n, C, dh);
    }
    // one fold backward: dout [rows][3] -> every gradient of layers l0 .. l0 + 2, dcode (=|+=), dpts [rows][D] (or null)
    void fold_bwd(int l0, const float *pts, int D, const float *H1, const float *H2, const float *dout, float *dpts, int acc_code) {
        const int M = t->rows;
        const size_t total = (size_t)M * 512;
        weight_grad(l0 + 2, H2, dout, M, 0, 512);
        bias_grad(l0 + 2, dout);
        input_grad(l0 + 2, dout, t->Y, M, 0, 512, 0);
        mask(t->Y, H2, total);                                           // d pre of the second layer
        weight_grad(l0 + 1, H1, t->Y, M, 0, 512);
        bias_grad(l0 + 1, t->Y);
        input_grad(l0 + 1, t->Y, t->Z, M, 0, 512, 0);
        mask(t->Z, H1, total);                                           // d pre of the first layer
        weight_grad(l0, pts, t->Z, M, FT_CODE, D);                       // the point rows
        if (dpts) input_grad(l0, t->Z, dpts, M, FT_CODE, D, 0);
        colsum<1>(t->Z, M, 512, 1, FT_G2, t->part);                      // chunk = cloud: d s [B][512]
        launch(ft_part_rows_kernel, dim3(cdiv(t->B * 512, 256)), dim3(256), t->part, t->B * 512, t->ds);
        launch(tb_colsum_final_kernel, dim3(2), dim3(256), t->part, t->B, 512, 1, t->grads + t->o_b[l0]);
        weight_grad(l0, t->code, t->ds, t->B, 0, FT_CODE);               // the code rows
        input_grad(l0, t->ds, t->dcode, t->B, 0, FT_CODE, acc_code);
    }
};

int run_step(geoadv_fold_trainer *t, const float *x, hipStream_t st) {
    Run q{{{st}, t, FT_EPS, t->part, t->partials}, t};
    const int B = t->B, R = t->R;
    // ---- forward ----
    q.launch(ft_input_kernel, dim3(cdiv(R * 12, 256)), dim3(256), x, t->graph.cov, R, t->in0);
    q.bn_layer(E1, t->in0, t->h[0]);
    q.bn_layer(E2, t->h[0], t->h[1]);
    q.bn_layer(E3, t->h[1], t->h[2]);
    q.graph_pool(t->h[2], 0, 64, t->g1, t->win1);
    q.bn_layer(E4, t->g1, t->h[3]);
    q.graph_pool(t->h[3], 1, 128, t->g2, t->win2);
    q.bn_layer(E5, t->g2, nullptr);
    ft_launch_gmax(q, t->a[E5], B, t->n, FT_LAT, t->inv + t->o_mv[E5], t->shift + t->o_mv[E5], t->pooled, t->arg);
    q.bn_layer(F1, t->pooled, t->h6);
    q.linear_fwd(F2, t->h6, t->code, B, 0, FT_CODE, true);
    q.fold_fwd(D0, t->grid, 2, t->H[0], t->H[1], t->mid);
    q.fold_fwd(D3, t->mid, 3, t->H[2], t->H[3], t->recon);
    if (int rc = q.chamfer(x, t->mid, t->mid_loss)) return rc;
    if (int rc = q.chamfer(x, t->recon, t->loss)) return rc;
    if (q.ok())
        if (int rc = geoadv_nn_distance_grad(B, t->n, x, FT_G2, t->recon, t->gd1, t->i1, t->gd2, t->i2, t->dx, t->drecon, st)) return rc;
    // ---- backward ----
    q.fold_bwd(D3, t->mid, 3, t->H[2], t->H[3], t->drecon, t->dmid, 0);
    q.fold_bwd(D0, t->grid, 2, t->H[0], t->H[1], t->dmid, nullptr, 1);
    q.linear_bwd(F2, t->h6, t->dcode, t->dsm1);                           // d h6 [B][512]
    q.bn_bwd(F1, false, t->dsm1, t->dsm2);
    q.linear_bwd(F1, t->pooled, t->dsm2, t->dsm1);                        // d pooled [B][1024]
    q.bn_bwd(E5, true, t->dsm1, t->X);                                    // d a5 [R][1024]
    q.linear_bwd(E5, t->g2, t->X, t->Y);                                  // d g2 [R][128]
    q.pool_bwd(t->Y, t->win2, 128, t->Z);                                 // d h4
    q.bn_bwd(E4, false, t->Z, t->Y);                                      // d a4
    q.linear_bwd(E4, t->g1, t->Y, t->Z);                                  // d g1 [R][64]
    q.pool_bwd(t->Z, t->win1, 64, t->Y);                                  // d h3
    q.bn_bwd(E3, false, t->Y, t->Z);
    q.linear_bwd(E3, t->h[1], t->Z, t->Y);                                // d h2
    q.bn_bwd(E2, false, t->Y, t->Z);
    q.linear_bwd(E2, t->h[0], t->Z, t->Y);                                // d h1
    q.bn_bwd(E1, false, t->Y, t->Z);
    q.linear_bwd(E1, t->in0, t->Z, nullptr);
    if (!q.ok()) {
        set_error("fold_trainer_step: %s", hipGetErrorString(q.err));
        return GEOADV_EHIP;
    }
    // ---- optimizer, running statistics, counters ----
    if (int rc = q.adam_and_running<true>(t->lr, t->wd, t->step)) return rc;
    t->step += 1;
    return GEOADV_OK;
}
}  // namespace

extern "C" int geoadv_fold_trainer_create(geoadv_fold_trainer **out, const geoadv_fold_weights *init, const geoadv_fold_train_config *cfg) {
    GA_REQUIRE(out && init && cfg, "fold_trainer_create: null argument");
    GA_REQUIRE(cfg->batch != 1, "fold_trainer_create: batch 1 cannot be trained: bn6 (after fc1) takes its statistics over the "
                                "clouds of the batch and needs at least 2");
    GA_REQUIRE(cfg->batch >= 2 && cfg->batch <= 1024, "fold_trainer_create: batch %d out of range [2, 1024]", cfg->batch);
    GA_REQUIRE(cfg->n_points >= 17 && cfg->n_points <= 16384, "fold_trainer_create: n_points %d out of range [17, 16384]", cfg->n_points);
    GA_REQUIRE((long long)cfg->batch * cfg->n_points <= FOLD_TRAIN_MAX_ROWS, "fold_trainer_create: batch * n_points exceeds 2^17 rows");
    GA_REQUIRE(cfg->initial_step >= 0 && cfg->initial_ordinal >= 0, "fold_trainer_create: initial_step and initial_ordinal must be >= 0");
    for (int l = 0; l < GEOADV_FOLD_ENC_LAYERS; ++l) {
        GA_REQUIRE(init->enc_w[l] && init->enc_b[l], "fold_trainer_create: null encoder weight pointer at layer %d", l);
        if (bn_of(l))
            GA_REQUIRE(init->enc_gamma[l] && init->enc_beta[l] && init->enc_mean[l] && init->enc_var[l],
                       "fold_trainer_create: null batch-norm pointer at encoder layer %d", l);
    }
    for (int l = 0; l < GEOADV_FOLD_DEC_LAYERS; ++l)
        GA_REQUIRE(init->dec_w[l] && init->dec_b[l], "fold_trainer_create: null decoder pointer at layer %d", l);
    geoadv_fold_trainer *t = new geoadv_fold_trainer();
    t->B = cfg->batch; t->n = cfg->n_points; t->R = t->B * t->n; t->rows = t->B * FT_G2;
    t->lr = cfg->learning_rate; t->wd = cfg->weight_decay; t->step = cfg->initial_step; t->ordinal = cfg->initial_ordinal;
    t->seed = (unsigned long long)cfg->seed;
    TrainLayer table[NL];
    TrainInit in{};
    for (int l = 0; l < NL; ++l) {
        table[l] = {kIn[l], kOut[l], 1, l <= E5 ? t->R : l <= F2 ? t->B : t->rows, bn_of(l), false};
        in.w[l] = l <= F2 ? init->enc_w[l] : init->dec_w[l - D0];
        in.b[l] = l <= F2 ? init->enc_b[l] : init->dec_b[l - D0];
        if (!bn_of(l)) continue;
        in.gamma[l] = init->enc_gamma[l]; in.beta[l] = init->enc_beta[l]; in.mean[l] = init->enc_mean[l]; in.var[l] = init->enc_var[l];
    }
    t->lay_out(table, NL);
    const size_t R = t->R, B = t->B, rows = t->rows;
    hipError_t e = hipSuccess;
    std::vector<void *> &mem = t->allocs;
    t->alloc(true, e);
    t->in0 = dev_alloc<float>(mem, R * 12, e);
    for (int l = 0; l <= F1; ++l) t->a[l] = dev_alloc<float>(mem, (l <= E5 ? R : B) * kOut[l], e);
    for (int l = 0; l < 4; ++l) t->h[l] = dev_alloc<float>(mem, R * kOut[l], e);
    t->g1 = dev_alloc<float>(mem, R * 64, e); t->g2 = dev_alloc<float>(mem, R * 128, e);
    t->win1 = dev_alloc<int>(mem, R * 64, e); t->win2 = dev_alloc<int>(mem, R * 128, e);
    t->pooled = dev_alloc<float>(mem, B * FT_LAT, e); t->arg = dev_alloc<int>(mem, B * FT_LAT, e);
    t->h6 = dev_alloc<float>(mem, B * 512, e); t->code = dev_alloc<float>(mem, B * 512, e); t->s = dev_alloc<float>(mem, B * 512, e);
    for (int i = 0; i < 4; ++i) t->H[i] = dev_alloc<float>(mem, rows * 512, e);
    t->mid = dev_alloc<float>(mem, rows * 3, e); t->recon = dev_alloc<float>(mem, rows * 3, e); t->grid = dev_alloc<float>(mem, rows * 2, e);
    t->picks = dev_alloc<int>(mem, 2 * R * FT_NB, e);
    t->d1 = dev_alloc<float>(mem, R, e); t->i1 = dev_alloc<int>(mem, R, e); t->gd1 = dev_alloc<float>(mem, R, e);
    t->d2 = dev_alloc<float>(mem, rows, e); t->i2 = dev_alloc<int>(mem, rows, e); t->gd2 = dev_alloc<float>(mem, rows, e);
    t->dx = dev_alloc<float>(mem, R * 3, e); t->drecon = dev_alloc<float>(mem, rows * 3, e); t->dmid = dev_alloc<float>(mem, rows * 3, e);
    t->loss = dev_alloc<float>(mem, 1, e); t->mid_loss = dev_alloc<float>(mem, 1, e);
    t->X = dev_alloc<float>(mem, R * FT_LAT, e);
    t->Y = dev_alloc<float>(mem, std::max(R * 128, rows * 512), e); t->Z = dev_alloc<float>(mem, std::max(R * 128, rows * 512), e);
    t->ds = dev_alloc<float>(mem, B * 512, e); t->dcode = dev_alloc<float>(mem, B * 512, e);
    t->dsm1 = dev_alloc<float>(mem, B * FT_LAT, e); t->dsm2 = dev_alloc<float>(mem, B * FT_LAT, e);
    t->partials = dev_alloc<float>(mem, CT_PARTIAL_FLOATS, e);
    t->part = dev_alloc<double2>(mem, std::max((size_t)cdiv((int)R, 256) * FT_LAT, (size_t)cdiv((int)rows, 256) * 512) + 1024, e);
    t->graph_ws = dev_alloc<char>(mem, fold_train_graph_bytes(t->B, t->n), e);
    t->upload(in, e);
    if (e == hipSuccess) {
        std::vector<float> hg(rows * 2), g1(R, 1.f / (float)R), g2(rows, 1.f / (float)rows);
        for (size_t r = 0; r < rows; ++r) {      // np.linspace(-0.3, 0.3, 45); point p = row * 45 + column is (x_column, y_row)
            const int p = (int)(r % FT_G2);
            auto lin = [](int i) { return (float)(i == FT_GRID - 1 ? 0.3 : -0.3 + i * (0.6 / (FT_GRID - 1))); };
            hg[2 * r] = lin(p % FT_GRID); hg[2 * r + 1] = lin(p / FT_GRID);
        }
        dev_upload(t->grid, hg, e); dev_upload(t->gd1, g1, e); dev_upload(t->gd2, g2, e);
    }
    if (e != hipSuccess) {
        delete t;
        return train_create_error("fold_trainer_create", e);
    }
    *out = t;
    return GEOADV_OK;
}

extern "C" void geoadv_fold_trainer_destroy(geoadv_fold_trainer *t) { delete t; }

extern "C" int geoadv_fold_trainer_set_slots(geoadv_fold_trainer *t, const float *slot1, const float *slot2) {
    GA_REQUIRE(t, "fold_trainer_set_slots: null handle");
    return t->set_slots(slot1, slot2);
}

extern "C" int geoadv_fold_trainer_step(geoadv_fold_trainer *t, const float *x, int sampling, int *picks, float *loss, float *mid_loss,
                                        void *stream) {
    GA_REQUIRE(t && x, "fold_trainer_step: null argument");
    GA_REQUIRE(sampling == GEOADV_FOLD_PICKS_GIVEN || sampling == GEOADV_FOLD_PICKS_DEVICE,
               "fold_trainer_step: sampling %d is not 0 (given) or 1 (device)", sampling);
    GA_REQUIRE(sampling == GEOADV_FOLD_PICKS_DEVICE || picks, "fold_trainer_step: given sampling needs the picks");
    hipStream_t st = as_stream(stream);
    const size_t pick_bytes = sizeof(int) * 2 * (size_t)t->R * FT_NB;
    if (sampling == GEOADV_FOLD_PICKS_GIVEN) GA_HIP(hipMemcpyAsync(t->picks, picks, pick_bytes, hipMemcpyDeviceToDevice, st));
    if (int rc = fold_train_graph(t->B, t->n, x, sampling, t->seed, t->ordinal, t->picks, t->graph_ws, st, &t->graph)) return rc;
    if (int rc = run_step(t, x, st)) return rc;
    t->ordinal += t->B;
    if (sampling == GEOADV_FOLD_PICKS_DEVICE && picks) GA_HIP(hipMemcpyAsync(picks, t->picks, pick_bytes, hipMemcpyDeviceToDevice, st));
    if (loss) GA_HIP(hipMemcpyAsync(loss, t->loss, sizeof(float), hipMemcpyDeviceToDevice, st));
    if (mid_loss) GA_HIP(hipMemcpyAsync(mid_loss, t->mid_loss, sizeof(float), hipMemcpyDeviceToDevice, st));
    return GEOADV_OK;
}

extern "C" int geoadv_fold_trainer_buffers(geoadv_fold_trainer *t, float **params, float **grads, size_t *count) {
    GA_REQUIRE(t, "fold_trainer_buffers: null handle");
    t->buffers(params, grads, count);
    return GEOADV_OK;
}

extern "C" int geoadv_fold_trainer_layout(const geoadv_fold_trainer *t, size_t *offsets52, size_t *moving_offsets13) {
    GA_REQUIRE(t && offsets52, "fold_trainer_layout: null argument");
    t->export_layout(offsets52, moving_offsets13, NL);
    return GEOADV_OK;
}

extern "C" int geoadv_fold_trainer_counters(const geoadv_fold_trainer *t, long long *step, long long *ordinal) {
    GA_REQUIRE(t, "fold_trainer_counters: null handle");
    if (step) *step = t->step;
    if (ordinal) *ordinal = t->ordinal;
    return GEOADV_OK;
}

extern "C" int geoadv_fold_trainer_state(const geoadv_fold_trainer *t, int what, int layer, const void **ptr, size_t *count) {
    GA_REQUIRE(t && ptr && count, "fold_trainer_state: null argument");
    const size_t B = t->B, R = t->R, rows = t->rows;
    switch (what) {
    case GEOADV_FOLD_STATE_BN_MEAN: case GEOADV_FOLD_STATE_BN_VAR: case GEOADV_FOLD_STATE_RUNNING_MEAN: case GEOADV_FOLD_STATE_RUNNING_VAR:
    case GEOADV_FOLD_STATE_BN_INV: case GEOADV_FOLD_STATE_BN_SHIFT:
        GA_REQUIRE(layer >= 0 && layer < NL && bn_of(layer), "fold_trainer_state: layer %d has no batch norm", layer);
        t->view(what, layer, ptr, count);       // GEOADV_FOLD_STATE_BN_MEAN .. BN_SHIFT are TA_BAT_MEAN .. TA_SHIFT
        return GEOADV_OK;
    case GEOADV_FOLD_STATE_PRE_BN:
        GA_REQUIRE(layer >= 0 && layer < NL && bn_of(layer), "fold_trainer_state: layer %d has no batch norm", layer);
        *ptr = t->a[layer]; *count = (layer <= E5 ? R : B) * kOut[layer];
        return GEOADV_OK;
    case GEOADV_FOLD_STATE_POOL_WINNER:
        GA_REQUIRE(layer == 0 || layer == 1, "fold_trainer_state: pool %d must be 0 or 1", layer);
        *ptr = layer == 0 ? t->win1 : t->win2; *count = R * (layer == 0 ? 64 : 128);
        return GEOADV_OK;
    case GEOADV_FOLD_STATE_HIDDEN:
        GA_REQUIRE(layer >= 0 && layer < 4, "fold_trainer_state: hidden decoder layer %d must be 0 .. 3", layer);
        *ptr = t->H[layer]; *count = rows * 512;
        return GEOADV_OK;
    case GEOADV_FOLD_STATE_CHAMFER_IDX:
        GA_REQUIRE(layer == 0 || layer == 1, "fold_trainer_state: Chamfer direction %d must be 0 or 1", layer);
        *ptr = layer == 0 ? t->i1 : t->i2; *count = layer == 0 ? R : rows;
        return GEOADV_OK;
    case GEOADV_FOLD_STATE_GMAX_ROW: *ptr = t->arg; *count = B * FT_LAT; return GEOADV_OK;
    case GEOADV_FOLD_STATE_PICKS: *ptr = t->picks; *count = 2 * R * FT_NB; return GEOADV_OK;
    case GEOADV_FOLD_STATE_COLS: *ptr = t->graph.cols; *count = t->graph.cols ? 2 * R * FT_NB : 0; return GEOADV_OK;
    case GEOADV_FOLD_STATE_COV: *ptr = t->graph.cov; *count = t->graph.cov ? R * 9 : 0; return GEOADV_OK;
    case GEOADV_FOLD_STATE_CODE: *ptr = t->code; *count = B * FT_CODE; return GEOADV_OK;
    case GEOADV_FOLD_STATE_MID: *ptr = t->mid; *count = rows * 3; return GEOADV_OK;
    case GEOADV_FOLD_STATE_RECON: *ptr = t->recon; *count = rows * 3; return GEOADV_OK;
    case GEOADV_FOLD_STATE_SLOT1: t->view(TA_SLOT1, 0, ptr, count); return GEOADV_OK;
    case GEOADV_FOLD_STATE_SLOT2: t->view(TA_SLOT2, 0, ptr, count); return GEOADV_OK;
    default: break;
    }
    set_error("fold_trainer_state: unknown state %d", what);
    return GEOADV_EINVAL;
}

namespace {
int check_kernel_sizes(const char *who, int b, int n, int c) {
    GA_REQUIRE(b >= 1 && b <= 1024, "%s: b %d out of range [1, 1024]", who, b);
    GA_REQUIRE(n >= 1, "%s: n %d must be >= 1", who, n);
    GA_REQUIRE((long long)b * n <= FOLD_TRAIN_MAX_ROWS, "%s: b * n = %lld exceeds 2^17 rows", who, (long long)b * n);
    GA_REQUIRE(c >= 1 && c <= 65536, "%s: c %d out of range [1, 65536]", who, c);
    return GEOADV_OK;
}
int finish(const char *who, const Launch &q) {
    if (q.ok()) return GEOADV_OK;
    set_error("%s: %s", who, hipGetErrorString(q.err));
    return GEOADV_EHIP;
}
}  // namespace

extern "C" int geoadv_fold_train_pool(int b, int n, int c, const float *h, const int *cols, float *g, int *win, void *stream) {
    GA_REQUIRE(h && cols && g && win, "fold_train_pool: null argument");
    if (int rc = check_kernel_sizes("fold_train_pool", b, n, c)) return rc;
    Launch q{as_stream(stream)};
    ft_launch_graph_pool(q, h, cols, (size_t)b * n, n, c, g, win);
    return finish("fold_train_pool", q);
}

extern "C" int geoadv_fold_train_pool_grad(int b, int n, int c, const float *dg, const int *win, const int *off, const int *deg,
                                           const int *col, float *dh, void *stream) {
    GA_REQUIRE(dg && win && off && deg && col && dh, "fold_train_pool_grad: null argument");
    if (int rc = check_kernel_sizes("fold_train_pool_grad", b, n, c)) return rc;
    Launch q{as_stream(stream)};
    ft_launch_pool_bwd(q, dg, win, off, deg, col, (size_t)b * n, n, c, dh);
    return finish("fold_train_pool_grad", q);
}

extern "C" int geoadv_fold_train_gmax(int b, int n, int c, const float *a, const float *inv, const float *shift, float *pooled, int *arg,
                                      void *stream) {
    GA_REQUIRE(a && inv && shift && pooled && arg, "fold_train_gmax: null argument");
    if (int rc = check_kernel_sizes("fold_train_gmax", b, n, c)) return rc;
    Launch q{as_stream(stream)};
    ft_launch_gmax(q, a, b, n, c, inv, shift, pooled, arg);
    return finish("fold_train_gmax", q);
}
