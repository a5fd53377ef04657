// The kNN outlier loss of the kNN attack (Tsai, Yang, Chen, AAAI 2020) and its gradient with respect to every point (not in the
// reference; the rule is written out in include/geoadv.h and restated in numpy by tests/_knn_loss_model.py, bit for bit).
// Two steps per call: the self-kNN search (geoadv_knn_point_ws, grouping.hip) into the caller's workspace, then ONE launch of
// knn_outlier_loss_kernel, one 1024-thread workgroup per cloud as stat_defense.hip:
//   A  per point the k squared distances to its neighbours, recomputed from the coordinates, and the float64 score (kept in the
//      workspace: the later phases read it back instead of gathering again); the SOR statistics in the rule's fixed order
//   B  the mask, the loss, and per TARGET the number of masked points that list it (integer atomics on a workspace row)
//   C  an exclusive scan of those in-degrees: every target owns a segment of the edge list in the workspace
//   D  every masked point drops its own index into the segment of each of its neighbours (integer atomic cursor: the ORDER
//      inside a segment is left to the hardware -- the set is not)
//   E  every target's thread adds the gather term (its own neighbours, column order) and then its segment in ASCENDING source
//      index, by repeatedly taking the smallest source not yet added: the order of the rule, whatever order D stored.  That is
//      O(d^2) in the in-degree d, so it serves d <= KL_SEGMENT_CAP; a target beyond it (ties naming one low-index neighbour,
//      a hub) is queued
//   F  a wave per queued target walks ALL points in ascending order, 64 at a time, and adds the sources a ballot finds, lowest
//      lane first: O(n k / 64) per hub, no bound on d, nothing truncated.
// No float atomics anywhere: every float64 sum is formed by one thread (or redundantly by every lane of one wave) in the
// rule's order, so two calls give the same bits.  Nothing in LDS grows with n or k: scores, in-degrees, cursors, the edge list
// and the hub queue live in the workspace (n = 2048, k = 5: 80 KB a cloud beside the search's rows, L2-resident).
// Visibility inside the workgroup: a word that an atomic has changed (in-degree, cursor) is only ever read by an agent-scope
// atomic load, never by a plain load that this CU's L1 could answer from an older copy; plain stores (scores, edges, queue) are
// read by other waves of the same workgroup after __syncthreads(), through the L1 they share.
#include <float.h>
#include <math.h>
#include "stat_sums.h"
#include "knn_loss.h"

namespace geoadv {

constexpr int KL_MAX_K = 15;              // k + 1 columns of the search fit its 17-slot register lists
constexpr int KL_MAX_N = 32767;           // the rule's limit (the mask is the complement of sor_filter's inliers)
constexpr int KL_SEARCH_MAX_N = 16384;    // geoadv_knn_point_ws holds a row of the cloud in LDS (grouping.hip ROW_MAX_N)
constexpr int KL_SEGMENT_CAP = 16;        // in-degree up to which a target's own thread orders its segment

struct KlLds {
    double wsum[DF_WAVES];
    int wcnt[DF_WAVES];
    int nhub;
};

__device__ __forceinline__ int kl_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// neighbour c of point p: column c + 1 of the search's row (column 0 is dropped, as geoadv_knn_dists does).  The index is
// clamped for the loads that follow: a search on non-finite input owes nobody an index inside the cloud.
__device__ __forceinline__ int kl_neighbour(const int *nbr, int stride, int p, int c, int n) {
    const int j = nbr[(size_t)p * stride + 1 + c];
    return min(max(j, 0), n - 1);
}

// The two rules of the launch (include/geoadv.h): the SOR rule, and the off-surface defense's (GEOADV_KNN_LOSS_SURFACE), whose score
// is geoadv_outlier_filter's fp32 mean distance and whose mask is that filter's `score > thresh`.  A template parameter of
// everything below: the SOR instances contain nothing of the surface rule (its square roots and float64 divisions least of all).
constexpr int KL_RULE_SOR = 0, KL_RULE_SURFACE = 1;
constexpr int KL_SURFACE_MAX_K = 7;       // geoadv_outlier_filter's limit: numpy's float32 mean of fewer than 8 elements is a left-to-right sum

struct KlStats { double mu, bound; };     // (surface rule: mu = (double)thr, bound unused)

template <int RULE>
__device__ __forceinline__ bool kl_masked(double s, const KlStats &st) {
    if (RULE == KL_RULE_SURFACE) return (float)s > (float)st.mu;         // both are floats widened: the filter's fp32 test; NaN fails, +inf passes
    const double d = s - st.mu;
    return isfinite(s) && s > st.mu && __dmul_rn(d, d) > st.bound;
}

// SOR rule: G += (double)x_i - (double)x_j, component by component.  Surface rule: G += ((double)x_i - (double)x_j) / (double)d with
// d = sqrtf(fp32 squared distance) recomputed from the two points (the same bits from either end); d == 0 adds nothing.
template <int RULE>
__device__ __forceinline__ void kl_add_diff(double (&G)[3], const float (&xi)[3], const float *xj) {
    if (RULE == KL_RULE_SURFACE) {
        const float dx = xi[0] - xj[0], dy = xi[1] - xj[1], dz = xi[2] - xj[2];
        const float d = sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
        if (d == 0.f) return;
        const double dd = (double)d;
#pragma unroll
        for (int a = 0; a < 3; ++a) G[a] += __ddiv_rn((double)xi[a] - (double)xj[a], dd);
        return;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) G[a] += (double)xi[a] - (double)xj[a];
}

// How a point's gradient leaves the launch.  The op (APPLY = false) stores it: grad_i = (float)(G_i * scale).  The attack loop's
// instance (APPLY = true, launch_knn_term below) adds it, weighted, to the Chamfer gradient that is already there:
//   g_i <- fadd_rn(g_i, fmul_rn(dist_weight[cloud], fmul_rn(knn_weight, grad_i)))       every product and the sum rounded to fp32
template <bool APPLY>
__device__ __forceinline__ void kl_emit(float *grad, int i, const double (&G)[3], double scale, float weight, float wb) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = (float)__dmul_rn(G[a], scale);
        if (APPLY) grad[3 * i + a] = __fadd_rn(grad[3 * i + a], __fmul_rn(wb, __fmul_rn(weight, d)));
        else grad[3 * i + a] = d;
    }
}

// APPLY: grad_all is the loop's g_dist [b,n,3] (read and written), `weight` the handle's knn_weight, dist_weight [b] the per-cloud
// weight the Chamfer gradient in g_dist already carries; score_all / mask_all / idx_all / stats are not looked at.
// RULE: alpha2 is alpha * alpha of the SOR rule, (double)thr of the surface rule.
template <bool APPLY, int RULE>
__global__ __launch_bounds__(DF_THREADS) void knn_outlier_loss_kernel(int n, int k, double alpha2, const float *xyz, const int *nbr_all,
                                                                      double *sc_all, int *deg_all, int *cur_all, int *edge_all,
                                                                      int *hub_all, double *loss, float *grad_all, double *score_all,
                                                                      unsigned char *mask_all, int *idx_all, double *stats,
                                                                      float weight, const float *dist_weight) {
    __shared__ KlLds L;
    const size_t cl = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int stride = k + 1;
    const float *x = xyz + cl * n * 3;
    const int *nbr = nbr_all + cl * n * stride;
    double *sc = sc_all + cl * n;
    int *deg = deg_all + cl * n, *cur = cur_all + cl * n, *hub = hub_all + cl * n;
    int *edge = edge_all + cl * n * k;
    if (t == 0) L.nhub = 0;

    // ---- A: scores and statistics (the SOR rule; step 1 of the summation order: thread t adds points t, t + T, ...) --------------
    constexpr int MAX_K = RULE == KL_RULE_SURFACE ? KL_SURFACE_MAX_K : KL_MAX_K;
    double acc = 0.0, cnt = 0.0;
    for (int p = t; p < n; p += DF_THREADS) {
        const float px = x[3 * p], py = x[3 * p + 1], pz = x[3 * p + 2];
        float val[MAX_K];
#pragma unroll
        for (int c = 0; c < MAX_K; ++c) {
            val[c] = 0.f;
            if (c < k) {
                const int raw = nbr[(size_t)p * stride + 1 + c];
                if (!APPLY && idx_all) idx_all[(cl * n + p) * k + c] = raw;
                const int j = min(max(raw, 0), n - 1);
                const float dx = px - x[3 * j], dy = py - x[3 * j + 1], dz = pz - x[3 * j + 2];
                val[c] = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
            }
        }
        double s;
        if (RULE == KL_RULE_SURFACE) {           // knn_score of defense.hip on registers: fp32, left to right, no division for k = 1
            float f = sqrtf(val[0]);
#pragma unroll
            for (int c = 1; c < MAX_K; ++c) if (c < k) f = __fadd_rn(f, sqrtf(val[c]));
            s = (double)(k > 1 ? __fdiv_rn(f, (float)k) : f);
        } else {
            s = (double)val[0];
#pragma unroll
            for (int c = 1; c < MAX_K; ++c) if (c < k) s += (double)val[c];      // sor_score on registers: the same sums in the same order
            s = s / (double)k;
        }
        sc[p] = s;
        deg[p] = 0;
        if (!APPLY && score_all) score_all[cl * n + p] = s;
        const bool fin = RULE == KL_RULE_SURFACE ? s == s : isfinite(s);         // (surface rule: the scores that are not NaN are counted)
        if (RULE == KL_RULE_SOR) acc += fin ? s : 0.0;                           // (surface rule: no statistics, the count alone)
        cnt += fin ? 1.0 : 0.0;
    }
    const double m = sd_block_sum64(cnt, L.wsum);
    KlStats st;
    double var = 0.0;
    if (RULE == KL_RULE_SURFACE) {               // no statistics: the threshold is given (the sum above was the barrier phase B needs)
        st.mu = alpha2;
        st.bound = 0.0;
    } else {
        const double sum = sd_block_sum64(acc, L.wsum);
        st.mu = m > 0.0 ? sum / m : 0.0;
        acc = 0.0;
        for (int p = t; p < n; p += DF_THREADS) {
            const double s = sc[p];
            const double d = s - st.mu;
            acc += isfinite(s) ? __dmul_rn(d, d) : 0.0;
        }
        const double sq = sd_block_sum64(acc, L.wsum);
        var = m >= 2.0 ? sq / (m - 1.0) : 0.0;
        st.bound = __dmul_rn(alpha2, var);
    }

    // ---- B: mask, loss, in-degrees (the barriers of the sums above order the zeroing of deg before these atomics) ----------------
    acc = 0.0;
    cnt = 0.0;
    for (int p = t; p < n; p += DF_THREADS) {
        const double s = sc[p];
        const bool w = kl_masked<RULE>(s, st);
        if (!APPLY && mask_all) mask_all[cl * n + p] = w ? 1 : 0;
        acc += w ? (RULE == KL_RULE_SURFACE ? s - st.mu : s) : 0.0;              // surface rule: the hinge (double)s_p - (double)thr
        cnt += w ? 1.0 : 0.0;
        if (w && grad_all)
            for (int c = 0; c < k; ++c) atomicAdd(&deg[kl_neighbour(nbr, stride, p, c, n)], 1);
    }
    const double nmask = sd_block_sum64(cnt, L.wsum);
    const double lsum = sd_block_sum64(acc, L.wsum);
    if (t == 0) {
        loss[cl] = lsum / (double)n;
        if (!APPLY && stats) { stats[4 * cl] = st.mu; stats[4 * cl + 1] = var; stats[4 * cl + 2] = m; stats[4 * cl + 3] = nmask; }
    }
    if (!grad_all) return;
    float *grad = grad_all + cl * n * 3;
    const float wb = APPLY ? dist_weight[cl] : 1.0f;

    // ---- C: exclusive scan of the in-degrees, 1024 targets a round: cur[i] = the start of target i's segment ----------------------
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += DF_THREADS) {
        const int p = p0 + t;
        const int d = p < n ? kl_load(&deg[p]) : 0;
        int incl = d;
#pragma unroll
        for (int s = 1; s < kWave; s <<= 1) {
            const int v = __shfl_up(incl, s, kWave);
            incl += lane >= s ? v : 0;
        }
        if (lane == 63) L.wcnt[wave] = incl;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < DF_WAVES; ++w) {
            const int cw = L.wcnt[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (p < n) cur[p] = base + before + incl - d;
        base += total;
        __syncthreads();
    }

    // ---- D: placement.  base <= n k: every masked point adds k edges, and the segments tile [0, base) -----------------------------
    for (int p = t; p < n; p += DF_THREADS) {
        if (!kl_masked<RULE>(sc[p], st)) continue;
        for (int c = 0; c < k; ++c) {
            const int slot = atomicAdd(&cur[kl_neighbour(nbr, stride, p, c, n)], 1);
            if (slot >= 0 && slot < n * k) edge[slot] = p;                       // (always true; the edge list has n k entries)
        }
    }
    __syncthreads();

    // ---- E: the gradient of every target with a short segment; the others are queued -----------------------------------------------
    const double scale = (RULE == KL_RULE_SURFACE ? 1.0 : 2.0) / ((double)n * (double)k);
    for (int i = t; i < n; i += DF_THREADS) {
        const int d = kl_load(&deg[i]);
        if (d > KL_SEGMENT_CAP) {
            hub[atomicAdd(&L.nhub, 1)] = i;
            continue;
        }
        const float xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
        double G[3] = {0.0, 0.0, 0.0};
        if (kl_masked<RULE>(sc[i], st))
            for (int c = 0; c < k; ++c) kl_add_diff<RULE>(G, xi, x + 3 * kl_neighbour(nbr, stride, i, c, n));
        const int end = min(kl_load(&cur[i]), n * k), start = max(end - d, 0);      // (the clamps never bind: after D, cur[i] is the segment's end)
        int last = -1;
        for (int done = 0; done < d;) {
            int next = n, mult = 0;                                              // the smallest source above `last`, and how often it occurs
            for (int e = start; e < end; ++e) {
                const int p = edge[e];
                if (p > last && p < next) { next = p; mult = 1; }
                else if (p == next) ++mult;
            }
            if (mult == 0) break;                                                // (never: the segment holds d sources)
            for (int r = 0; r < mult; ++r) kl_add_diff<RULE>(G, xi, x + 3 * next);
            done += mult;
            last = next;
        }
        kl_emit<APPLY>(grad, i, G, scale, weight, wb);
    }
    __syncthreads();

    // ---- F: the queued targets, a wave each: all points in ascending order, every lane forming the same sum ------------------------
    const int nhub = L.nhub;
    for (int h = wave; h < nhub; h += DF_WAVES) {
        const int i = min(max(hub[h], 0), n - 1);                                    // (a queued target is a point of the cloud)
        const float xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
        double G[3] = {0.0, 0.0, 0.0};
        if (kl_masked<RULE>(sc[i], st))
            for (int c = 0; c < k; ++c) kl_add_diff<RULE>(G, xi, x + 3 * kl_neighbour(nbr, stride, i, c, n));
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const int p = p0 + lane;
            int mult = 0;
            float xp[3] = {0.f, 0.f, 0.f};
            if (p < n && kl_masked<RULE>(sc[p], st)) {
                for (int c = 0; c < k; ++c) mult += kl_neighbour(nbr, stride, p, c, n) == i ? 1 : 0;
                xp[0] = x[3 * p]; xp[1] = x[3 * p + 1]; xp[2] = x[3 * p + 2];
            }
            unsigned long long hits = __ballot(mult > 0);
            while (hits) {
                const int src = __ffsll((long long)hits) - 1;
                hits &= hits - 1;
                const float xs[3] = {__shfl(xp[0], src, kWave), __shfl(xp[1], src, kWave), __shfl(xp[2], src, kWave)};
                const int reps = __shfl(mult, src, kWave);
                for (int r = 0; r < reps; ++r) kl_add_diff<RULE>(G, xi, xs);
            }
        }
        if (lane == 0) kl_emit<APPLY>(grad, i, G, scale, weight, wb);
    }
}

// The workspace, carved from `base` (over a null base: measured only): the search's own workspace, its values and indices, then
// the launch's per-point arrays
struct KlScratch {
    char *knn;
    size_t knn_bytes;
    float *val;
    int *idx;
    double *sc;
    int *deg, *cur, *hub, *edge;
    size_t bytes;
};
static KlScratch kl_scratch(void *base, int b, int n, int k) {
    const size_t bn = (size_t)b * n;
    Carver c(base);
    KlScratch s;
    s.knn_bytes = geoadv_knn_workspace_bytes(b, n, n, k + 1);
    s.knn = c.take<char>(s.knn_bytes);
    s.val = c.take<float>(bn * (k + 1));
    s.idx = c.take<int>(bn * (k + 1));
    s.sc = c.take<double>(bn);
    s.deg = c.take<int>(bn);
    s.cur = c.take<int>(bn);
    s.hub = c.take<int>(bn);
    s.edge = c.take<int>(bn * k);
    s.bytes = c.bytes();
    return s;
}

static bool kl_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + nb && pb < pa + na;
}

static bool kl_shape_ok(int b, int n, int k) { return b >= 0 && b <= 65535 && k >= 1 && k <= KL_MAX_K && n >= k + 2 && n <= KL_MAX_N; }

static int kl_check(const char *op, int rule, int b, int n, int k, double alpha, const float *xyz, const double *loss, const float *grad,
                    const void *workspace, size_t workspace_bytes) {
    GA_REQUIRE(rule == KL_RULE_SOR || rule == KL_RULE_SURFACE, "%s: unknown rule %d", op, rule);
    GA_REQUIRE(b >= 0 && b <= 65535, "%s: batch %d must be in [0, 65535]", op, b);
    GA_REQUIRE(k >= 1 && k <= KL_MAX_K, "%s: k=%d must be in [1, %d]", op, k, KL_MAX_K);
    if (rule == KL_RULE_SURFACE) {        // alpha is the threshold, used as (float)alpha
        GA_REQUIRE(k <= KL_SURFACE_MAX_K, "%s: the surface rule takes k in [1, %d] as geoadv_outlier_filter does (k=%d)", op, KL_SURFACE_MAX_K, k);
        GA_REQUIRE(alpha >= 0.0 && alpha <= (double)FLT_MAX, "%s: the surface rule's threshold must be in [0, FLT_MAX] (got %g)", op, alpha);
    }
    GA_REQUIRE(n >= k + 2 && n <= KL_MAX_N, "%s: n=%d must be in [k + 2 = %d, %d]", op, n, k + 2, KL_MAX_N);
    GA_REQUIRE(n <= KL_SEARCH_MAX_N, "%s: the k-NN search takes at most %d points per cloud (n=%d)", op, KL_SEARCH_MAX_N, n);
    GA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "%s: alpha must be finite and >= 0 (got %g)", op, alpha);
    if (b == 0) return GEOADV_OK;
    GA_REQUIRE(xyz && loss, "%s: null pointer", op);
    const size_t need = geoadv_knn_outlier_loss_workspace_bytes(b, n, k);
    GA_REQUIRE(workspace && workspace_bytes >= need, "%s: workspace too small (%zu bytes, need %zu)", op, workspace_bytes, need);
    const size_t bytes = (size_t)b * n * 3 * sizeof(float);
    GA_REQUIRE(!grad || !kl_overlap(grad, bytes, xyz, bytes), "%s: grad overlaps xyz", op);
    return GEOADV_OK;
}

// what the kernel takes in its `alpha2` place: alpha * alpha of the SOR rule, the fp32 threshold (widened) of the surface rule
static double kl_rule_arg(int rule, double alpha) { return rule == KL_RULE_SURFACE ? (double)(float)alpha : alpha * alpha; }

static int kl_launch(int rule, int b, int n, int k, double alpha, const float *xyz, double *loss, float *grad, double *score,
                     unsigned char *mask, int *idx, double *stats, const KlScratch &s, hipStream_t st) {
    const double arg = kl_rule_arg(rule, alpha);
    if (rule == KL_RULE_SURFACE)
        knn_outlier_loss_kernel<false, KL_RULE_SURFACE><<<b, DF_THREADS, 0, st>>>(n, k, arg, xyz, s.idx, s.sc, s.deg, s.cur, s.edge, s.hub, loss, grad,
                                                                                  score, mask, idx, stats, 0.f, nullptr);
    else
        knn_outlier_loss_kernel<false, KL_RULE_SOR><<<b, DF_THREADS, 0, st>>>(n, k, arg, xyz, s.idx, s.sc, s.deg, s.cur, s.edge, s.hub, loss, grad,
                                                                              score, mask, idx, stats, 0.f, nullptr);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

// The term of the attack loop (attack.hip: do_step; the rule at geoadv_attack_config in include/geoadv.h): the op's search with its
// default kernel choice, then the APPLY instance of the launch, both on `st`, both on the caller's workspace
// (geoadv_knn_outlier_loss_workspace_bytes(b, n, k) bytes).  The shape was checked when the handle was created.
// rule: 0 = the SOR rule with `alpha`; 1 = the surface rule, `alpha` its threshold (geoadv_attack_config.knn_rule / knn_thresh).
int launch_knn_term(int rule, int b, int n, int k, double alpha, float weight, const float *dist_weight, const float *xyz, float *g_dist,
                    double *loss, void *workspace, size_t workspace_bytes, hipStream_t st) {
    if (int rc = kl_check("attack knn term", rule, b, n, k, alpha, xyz, loss, g_dist, workspace, workspace_bytes)) return rc;
    const KlScratch s = kl_scratch(workspace, b, n, k);
    if (int rc = geoadv_knn_point_ws(GEOADV_KNN_AUTO, b, n, n, k + 1, xyz, xyz, s.val, s.idx, s.knn, s.knn_bytes, st)) return rc;
    const double arg = kl_rule_arg(rule, alpha);
    if (rule == KL_RULE_SURFACE)
        knn_outlier_loss_kernel<true, KL_RULE_SURFACE><<<b, DF_THREADS, 0, st>>>(n, k, arg, xyz, s.idx, s.sc, s.deg, s.cur, s.edge, s.hub, loss, g_dist,
                                                                                 nullptr, nullptr, nullptr, nullptr, weight, dist_weight);
    else
        knn_outlier_loss_kernel<true, KL_RULE_SOR><<<b, DF_THREADS, 0, st>>>(n, k, arg, xyz, s.idx, s.sc, s.deg, s.cur, s.edge, s.hub, loss, g_dist,
                                                                             nullptr, nullptr, nullptr, nullptr, weight, dist_weight);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

}  // namespace geoadv

using namespace geoadv;

extern "C" size_t geoadv_knn_outlier_loss_workspace_bytes(int b, int n, int k) {
    if (!kl_shape_ok(b, n, k) || b == 0) return 256;
    return kl_scratch(nullptr, b, n, k).bytes + 256;       // (+ 256: the workspace pointer is aligned up here)
}

extern "C" int geoadv_knn_outlier_loss(int kernel, int b, int n, int k, double alpha, const float *xyz, double *loss, float *grad,
                                       double *score, unsigned char *mask, int *idx, double *stats, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    const int rule = (kernel & GEOADV_KNN_LOSS_SURFACE) ? KL_RULE_SURFACE : KL_RULE_SOR;      // the one flag a kernel choice may carry
    kernel &= ~GEOADV_KNN_LOSS_SURFACE;
    GA_REQUIRE(kernel >= GEOADV_KNN_AUTO && kernel <= GEOADV_KNN_GRID_SHELLS, "knn_outlier_loss: unknown k-NN kernel %d", kernel);
    if (int rc = kl_check("knn_outlier_loss", rule, b, n, k, alpha, xyz, loss, grad, workspace, workspace_bytes)) return rc;
    if (b == 0) return GEOADV_OK;
    const KlScratch s = kl_scratch(workspace, b, n, k);
    if (int rc = geoadv_knn_point_ws(kernel, b, n, n, k + 1, xyz, xyz, s.val, s.idx, s.knn, s.knn_bytes, stream)) return rc;
    return kl_launch(rule, b, n, k, alpha, xyz, loss, grad, score, mask, idx, stats, s, as_stream(stream));
}

extern "C" int geoadv_debug_knn_outlier_loss_launch(int b, int n, int k, double alpha, const float *xyz, double *loss, float *grad,
                                                    void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = kl_check("debug_knn_outlier_loss_launch", KL_RULE_SOR, b, n, k, alpha, xyz, loss, grad, workspace, workspace_bytes)) return rc;
    if (b == 0) return GEOADV_OK;
    return kl_launch(KL_RULE_SOR, b, n, k, alpha, xyz, loss, grad, nullptr, nullptr, nullptr, nullptr, kl_scratch(workspace, b, n, k), as_stream(stream));
}
