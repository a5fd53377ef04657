// geoadv_cls_evaluate: the voted evaluation of classifier/tst_classifier.py (eval_one_epoch) for one batch, on one stream,
// without a host synchronisation; and geoadv_rotate_y, provider.rotate_point_cloud_by_angle.
//
// Per vote v of V:
//   rotate_y        the batch turned by v / V * 2 pi about the up axis into workspace              (1 launch)
//   cls_forward     the six launches of classifier.hip, called as they are: logits, the vote's arg-max, T2
//   cls_eval_close  one workgroup per cloud: pred_sum += logits (float64), vote_counts[arg-max] += 1, the cloud's cross
//                   entropy and 0.5 * ||T2 T2^T - I||_F^2 into workspace; after the last vote the first maximum of pred_sum
//   cls_eval_loss   one workgroup: loss[v] = mean_b(CE) + 0.001 * sum_b(reg)                       (only with labels)
// Votes follow each other on the stream, so a (cloud, class) entry of pred_sum is added to by one thread per vote, in vote
// order: the float64 sum has one value.  Nothing is atomic and every reduction is a fixed tree, so two runs are bit-equal.
//
// ARITHMETIC of the closing kernel.
//   rotation   float32 coordinates times the float64 matrix [[c,0,s],[0,1,0],[-s,0,c]] (row vector times matrix), all three
//              products and both sums of a coordinate in float64, rounded to float32 once -- numpy's float32 @ float64
//              product without a fused multiply-add (the library is compiled with -ffp-contract=off).
//   CE         float64 from the float32 logits: m = max z, log(sum exp(z - m)) + m - z[label].  C <= 1024 exp per cloud is
//              nothing against the forward, and float64 leaves only the final rounding of the loss to float32, well inside
//              (C + 8) * 2^-24 * max(1, |z|max + log C) per cloud whatever the order of the sum.
//   reg        a_ij = sum_k t_ik t_jk as a 64-term float32 fmaf chain from LDS (plain VALU: 0.26 M multiply-adds per cloud
//              against the forward's ~0.9 G per cloud at n = 2048, so the simplest form wins over an MFMA tile): |a_ij -
//              exact| <= 64 * 2^-24 * sum_k |t_ik||t_jk|; e_ij = a_ij - [i == j] adds one rounding, 2^-24 |e_ij|.  The
//              squares are formed and summed in float64 (a float32 square is exact in float64), so the sum over the 4096
//              entries adds nothing to speak of; the per-entry bound is the 66 * 2^-24 * sum_k |t_ik||t_jk| of the test.
//   loss       the per-cloud CE and reg are float64 in workspace; cls_eval_loss sums them in float64 (thread t takes clouds
//              t, t + 256, ..., then a fixed tree over the 256 threads) and rounds the vote's loss to float32 once.
// A label outside [0, C) makes its cloud's CE a NaN without reading the logits at it: that vote's loss is NaN.
#include "common.h"
#include "host_util.h"
#include <math.h>

namespace geoadv {

constexpr int EV_THREADS = 256;
constexpr int EV_TS = 65;                           // LDS row stride of T2: 64 + 1, so that lanes j = 0..63 of t[j][k] hit 32 banks

// ---- rotation ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void rotate_point(float x, float y, float z, double c, double s, float &ox, float &oy, float &oz) {
    const double dx = x, dy = y, dz = z;
    ox = (float)((dx * c + dy * 0.0) + dz * -s);
    oy = (float)((dx * 0.0 + dy * 1.0) + dz * 0.0);
    oz = (float)((dx * s + dy * 0.0) + dz * c);
}

// VEC: thread g < groups turns points 4 g .. 4 g + 3 (three 16-byte loads and stores; both pointers 16-byte aligned), the next
// points % 4 threads one tail point each.  !VEC: one point per thread.
template <bool VEC>
__global__ __launch_bounds__(EV_THREADS) void rotate_y_kernel(const float *in, float *out, size_t points, double c, double s) {
    const size_t g = (size_t)blockIdx.x * EV_THREADS + threadIdx.x;
    size_t p = g;
    if (VEC) {
        const size_t groups = points / 4;
        if (g < groups) {
            const float4 *src = reinterpret_cast<const float4 *>(in) + 3 * g;
            const float4 a = src[0], b = src[1], d = src[2];
            float4 oa, ob, od;
            rotate_point(a.x, a.y, a.z, c, s, oa.x, oa.y, oa.z);
            rotate_point(a.w, b.x, b.y, c, s, oa.w, ob.x, ob.y);
            rotate_point(b.z, b.w, d.x, c, s, ob.z, ob.w, od.x);
            rotate_point(d.y, d.z, d.w, c, s, od.y, od.z, od.w);
            float4 *dst = reinterpret_cast<float4 *>(out) + 3 * g;
            dst[0] = oa; dst[1] = ob; dst[2] = od;
            return;
        }
        p = 4 * groups + (g - groups);
    }
    if (p >= points) return;
    float ox, oy, oz;
    rotate_point(in[3 * p], in[3 * p + 1], in[3 * p + 2], c, s, ox, oy, oz);
    out[3 * p] = ox; out[3 * p + 1] = oy; out[3 * p + 2] = oz;
}

static int launch_rotate(const float *in, float *out, size_t points, double c, double s, hipStream_t st) {
    const bool vec = ((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & 15) == 0;
    const size_t threads = vec ? points / 4 + points % 4 : points;
    const size_t blocks = (threads + EV_THREADS - 1) / EV_THREADS;
    GA_REQUIRE(blocks <= 0x7fffffffull, "rotate_y: %zu points are too many for one launch", points);
    if (vec)
        hipLaunchKernelGGL(rotate_y_kernel<true>, dim3((unsigned)blocks), dim3(EV_THREADS), 0, st, in, out, points, c, s);
    else
        hipLaunchKernelGGL(rotate_y_kernel<false>, dim3((unsigned)blocks), dim3(EV_THREADS), 0, st, in, out, points, c, s);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

// ---- the closing kernel ------------------------------------------------------------------------------------------
// fixed tree over the EV_THREADS values of red[]: every thread gets the result
template <class Op>
__device__ __forceinline__ double block_reduce(double v, double *red, Op op) {
    const int t = threadIdx.x;
    __syncthreads();                                // red[] may still be read from an earlier reduction
    red[t] = v;
    __syncthreads();
    for (int w = EV_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = op(red[t], red[t + w]);
        __syncthreads();
    }
    return red[0];
}

struct ClsCloseArgs {
    const float *logits;                            // [b][C], this vote's
    const int *vote_label;                          // [b], this vote's arg-max (first maximum)
    const float *t2;                                // [b][4096], this vote's feature transform (read only with labels)
    const int *labels;                              // [b] or null: no loss
    double *pred_sum;                               // [b][C], zeroed before vote 0
    int *vote_counts;                               // [b][C] or null, zeroed before vote 0
    int *pred;                                      // [b] or null; written when `last`
    double *ce, *reg;                               // [b] each (with labels)
    int C, last;
};

__global__ __launch_bounds__(EV_THREADS) void cls_eval_close_kernel(ClsCloseArgs A) {
    __shared__ float T[64 * EV_TS];
    __shared__ double ps[1024];
    __shared__ double red[EV_THREADS];
    const int c = blockIdx.x, t = threadIdx.x, C = A.C;
    const float *z = A.logits + (size_t)c * C;

    // votes: pred_sum (one thread per class, so no two threads touch an entry) and the count of this vote's arg-max
    double *sum = A.pred_sum + (size_t)c * C;
    for (int o = t; o < C; o += EV_THREADS) {
        const double v = sum[o] + (double)z[o];
        sum[o] = v;
        ps[o] = v;
    }
    if (t == 0 && A.vote_counts) A.vote_counts[(size_t)c * C + A.vote_label[c]] += 1;       // (the arg-max lies in [0, C))
    __syncthreads();
    if (A.last && A.pred && t == 0) {
        // np.argmax: the first maximum; a NaN counts as the maximum (the first NaN wins)
        int best = 0;
        double bv = ps[0];
        for (int o = 1; o < C && !(bv != bv); ++o)
            if (ps[o] > bv || ps[o] != ps[o]) { best = o; bv = ps[o]; }
        A.pred[c] = best;
    }
    if (!A.labels) return;                          // (uniform over the launch)

    // cross entropy, float64
    const int lab = A.labels[c];
    double m = -INFINITY;
    for (int o = t; o < C; o += EV_THREADS) m = fmax(m, (double)z[o]);
    m = block_reduce(m, red, [](double a, double b) { return fmax(a, b); });
    double s = 0.0;
    for (int o = t; o < C; o += EV_THREADS) s += exp((double)z[o] - m);
    s = block_reduce(s, red, [](double a, double b) { return a + b; });
    if (t == 0) A.ce[c] = (lab >= 0 && lab < C) ? (log(s) + m) - (double)z[lab] : (double)NAN;

    // 0.5 * || T2 T2^T - I ||_F^2: thread (i0 = t / 64, j = t % 64) owns the entries (i0 + 4 r, j), r = 0 .. 15
    const float *t2 = A.t2 + (size_t)c * 4096;
    for (int e = t; e < 4096; e += EV_THREADS) T[(e >> 6) * EV_TS + (e & 63)] = t2[e];
    __syncthreads();
    const int j = t & 63, i0 = t >> 6;
    float a[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
    for (int k = 0; k < 64; ++k) {
        const float tj = T[j * EV_TS + k];
#pragma unroll
        for (int r = 0; r < 16; ++r) a[r] = fmaf(T[(i0 + 4 * r) * EV_TS + k], tj, a[r]);
    }
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float e = a[r] - (i0 + 4 * r == j ? 1.f : 0.f);
        sq += (double)e * (double)e;
    }
    sq = block_reduce(sq, red, [](double a, double b) { return a + b; });
    if (t == 0) A.reg[c] = 0.5 * sq;
}

// loss = mean_b(CE) + 0.001 * sum_b(reg) (pointnet_cls.get_loss with reg_weight 0.001), one workgroup
__global__ __launch_bounds__(EV_THREADS) void cls_eval_loss_kernel(const double *ce, const double *reg, int b, float *loss) {
    __shared__ double red[EV_THREADS];
    double sc = 0.0, sr = 0.0;
    for (int c = threadIdx.x; c < b; c += EV_THREADS) { sc += ce[c]; sr += reg[c]; }
    sc = block_reduce(sc, red, [](double a, double b) { return a + b; });
    sr = block_reduce(sr, red, [](double a, double b) { return a + b; });
    if (threadIdx.x == 0) *loss = (float)(sc / (double)b + 0.001 * sr);
}

}  // namespace geoadv

using namespace geoadv;

extern "C" int geoadv_rotate_y(int b, int n, const float *pc, double cos_angle, double sin_angle, float *out, void *stream) {
    GA_REQUIRE(b >= 0 && n >= 0, "rotate_y: negative shape (%d, %d)", b, n);
    if (b == 0 || n == 0) return GEOADV_OK;
    GA_REQUIRE(pc && out, "rotate_y: null pointer");
    return launch_rotate(pc, out, (size_t)b * n, cos_angle, sin_angle, as_stream(stream));
}

namespace {
struct EvalScratch {
    float *rot, *logits, *t2;
    int *vote_label;
    double *ce, *reg, *pred_sum;
    void *forward;
    size_t bytes;
};
EvalScratch carve_eval(void *workspace, const geoadv_cls *cls, int b, int n, int C) {
    EvalScratch s;
    Carver cv(workspace);
    s.rot = cv.take<float>((size_t)b * n * 3);
    s.logits = cv.take<float>((size_t)b * C);
    s.t2 = cv.take<float>((size_t)b * 4096);
    s.vote_label = cv.take<int>((size_t)b);
    s.ce = cv.take<double>((size_t)b);
    s.reg = cv.take<double>((size_t)b);
    s.pred_sum = cv.take<double>((size_t)b * C);
    s.forward = cv.take<char>(geoadv_cls_workspace_bytes(cls, b, n));
    s.bytes = cv.bytes();
    return s;
}
// geoadv_cls is defined in cls_model.h (classifier.hip's handle); its first member is `int num_classes`, and a pointer to a standard-layout struct
// points to its first member
int classes_of(const geoadv_cls *cls) { return *reinterpret_cast<const int *>(cls); }
}  // namespace

extern "C" size_t geoadv_cls_evaluate_workspace_bytes(const geoadv_cls *cls, int b, int n) {
    if (!cls || b <= 0 || n <= 0) return 256;
    return carve_eval(nullptr, cls, b, n, classes_of(cls)).bytes + 256;
}

extern "C" int geoadv_cls_evaluate(const geoadv_cls *cls, int b, int n, const float *pc, const int *labels, int num_votes,
                                   const double *cos_sin, float *loss, int *pred, double *pred_sum, int *vote_counts,
                                   void *workspace, void *stream) {
    GA_REQUIRE(cls, "cls_evaluate: null handle");
    GA_REQUIRE(b >= 1, "cls_evaluate: batch %d must be >= 1", b);
    GA_REQUIRE(n >= 1 && n <= 16384, "cls_evaluate: n %d out of range [1, 16384]", n);
    GA_REQUIRE(num_votes >= 1 && num_votes <= 64, "cls_evaluate: num_votes %d out of range [1, 64]", num_votes);
    GA_REQUIRE(pc && workspace, "cls_evaluate: null point cloud or workspace");
    hipStream_t st = as_stream(stream);
    const int C = classes_of(cls);
    const EvalScratch s = carve_eval(workspace, cls, b, n, C);
    const bool want_loss = labels && loss;

    ClsCloseArgs ca{};
    ca.logits = s.logits;
    ca.vote_label = s.vote_label;
    ca.t2 = s.t2;
    ca.labels = want_loss ? labels : nullptr;
    ca.pred_sum = pred_sum ? pred_sum : s.pred_sum;
    ca.vote_counts = vote_counts;
    ca.pred = pred;
    ca.ce = s.ce;
    ca.reg = s.reg;
    ca.C = C;
    GA_HIP(hipMemsetAsync(ca.pred_sum, 0, sizeof(double) * (size_t)b * C, st));
    if (vote_counts) GA_HIP(hipMemsetAsync(vote_counts, 0, sizeof(int) * (size_t)b * C, st));
    for (int v = 0; v < num_votes; ++v) {
        double c, sn;
        if (cos_sin) {
            c = cos_sin[2 * v];
            sn = cos_sin[2 * v + 1];
        } else {                                    // tst_classifier.py:134: vote_idx / float(num_votes) * np.pi * 2
            const double angle = (double)v / (double)num_votes * M_PI * 2;
            c = cos(angle);
            sn = sin(angle);
        }
        if (int rc = launch_rotate(pc, s.rot, (size_t)b * n, c, sn, st)) return rc;
        if (int rc = geoadv_cls_forward(cls, b, n, s.rot, s.logits, s.vote_label, nullptr, want_loss ? s.t2 : nullptr, s.forward,
                                        stream))
            return rc;
        ca.last = v == num_votes - 1;
        hipLaunchKernelGGL(cls_eval_close_kernel, dim3(b), dim3(EV_THREADS), 0, st, ca);
        GA_LAUNCH_CHECK();
        if (want_loss) {
            hipLaunchKernelGGL(cls_eval_loss_kernel, dim3(1), dim3(EV_THREADS), 0, st, s.ce, s.reg, b, loss + v);
            GA_LAUNCH_CHECK();
        }
    }
    return GEOADV_OK;
}
