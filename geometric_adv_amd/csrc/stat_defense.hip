// The two baseline defenses of the point-cloud attack literature on the device (neither is in the reference; the rules are
// written out in include/geoadv.h and restated in numpy by tests/_stat_defense_model.py, bit for bit):
//   sor_filter   statistical outlier removal: per cloud the mean and the variance of the kNN score in float64, summed in a
//                fixed order, then the packing of outlier_filter with the threshold mean + alpha * std (tested without sqrt);
//   random_drop  simple random sampling: per cloud the `drop` smallest of n counter-based 64-bit draws, found by a radix
//                select, then the packing of the kept points and of the dropped indices.
// One 1024-thread workgroup per cloud, as in defense.hip.  Nothing is kept between the passes over a cloud: a score is a
// handful of loads (the rows stay in L2) and a draw two mix64, so each pass recomputes them and no size needs scratch memory.
// Launch- and latency-bound at a batch's size (32 x 2048 points: 0.8 MB in, 0.8 MB out, a few dozen barriers per workgroup on
// 32 of 256 CUs): the time is the launch plus the chain of barriers, and nothing here is tuned beyond that.
#include <math.h>
#include "defense_pack.h"
#include "stat_sums.h"

namespace geoadv {

__global__ __launch_bounds__(DF_THREADS) void sor_filter_kernel(int n, const float *pc, const float *knn, int stride, int k, double alpha2,
                                                                float *outlier_pc, short *outlier_idx, short *outlier_num,
                                                                float *inlier_pc, double *stats) {
    __shared__ CompactLds L;
    __shared__ double wsum[DF_WAVES];
    const size_t c = blockIdx.x;
    const float *cloud = pc + c * n * 3;
    const float *rows = knn + c * n * stride;
    float *opc = outlier_pc ? outlier_pc + c * n * 3 : nullptr;
    short *oix = outlier_idx ? outlier_idx + c * n : nullptr;
    float *ipc = inlier_pc + c * n * 3;

    // step 1 of the summation order: thread t adds points t, t + T, ... in ascending order, starting at +0.0
    double acc = 0.0, cnt = 0.0;
    for (int p = threadIdx.x; p < n; p += DF_THREADS) {
        const double s = sor_score(rows + (size_t)p * stride, k);
        const bool fin = isfinite(s);
        acc += fin ? s : 0.0;
        cnt += fin ? 1.0 : 0.0;
    }
    const double m = sd_block_sum64(cnt, wsum);             // (a count below 2^15: exact in any order)
    const double sum = sd_block_sum64(acc, wsum);
    const double mu = m > 0.0 ? sum / m : 0.0;
    acc = 0.0;
    for (int p = threadIdx.x; p < n; p += DF_THREADS) {
        const double s = sor_score(rows + (size_t)p * stride, k);
        const double d = s - mu;
        acc += isfinite(s) ? __dmul_rn(d, d) : 0.0;
    }
    const double sq = sd_block_sum64(acc, wsum);
    const double var = m >= 2.0 ? sq / (m - 1.0) : 0.0;
    const double bound = __dmul_rn(alpha2, var);
    if (stats && threadIdx.x == 0) { stats[3 * c] = mu; stats[3 * c + 1] = var; stats[3 * c + 2] = m; }

    auto inlier = [&](int p) {
        const double s = sor_score(rows + (size_t)p * stride, k);
        const double d = s - mu;
        return isfinite(s) && (s <= mu || __dmul_rn(d, d) <= bound);
    };
    if (opc || oix || outlier_num) {
        const int no = block_compact(n, L, [&](int p) { return !inlier(p); },
                                     [&](int p, int slot) {
                                         if (opc) copy_point(opc + 3 * (size_t)slot, cloud + 3 * (size_t)p);
                                         if (oix) oix[slot] = (short)p;                       // n <= 32767: never wraps
                                     });
        const int last_o = L.last;
        __syncthreads();
        if (opc) pad_cloud(opc, cloud, no, n, last_o);
        if (oix) for (int s = no + threadIdx.x; s < n; s += DF_THREADS) oix[s] = 0;
        if (outlier_num && threadIdx.x == 0) outlier_num[c] = (short)no;
    }
    const int ni = block_compact(n, L, inlier, [&](int p, int slot) { copy_point(ipc + 3 * (size_t)slot, cloud + 3 * (size_t)p); });
    const int last_i = L.last;
    __syncthreads();
    pad_cloud(ipc, cloud, ni, n, last_i);
}

// r(p) of the rule, from key0 = mix(mix(seed + G) ^ counter)
__device__ __forceinline__ unsigned long long srs_draw(unsigned long long key0, unsigned long long slot, int p) {
    return mix64(mix64(key0 ^ ((slot << 32) | (unsigned long long)p)) + 48ull * kGolden64);
}

struct SelectLds {
    unsigned hist[256];
    unsigned long long prefix;
    unsigned need;
};

__global__ __launch_bounds__(DF_THREADS) void random_drop_kernel(int n, const float *pc, int drop, unsigned long long seed,
                                                                 unsigned long long counter, unsigned long long slot_offset,
                                                                 float *kept_pc, int *dropped_idx) {
    __shared__ CompactLds L;
    __shared__ SelectLds S;
    const size_t c = blockIdx.x;
    const int t = threadIdx.x, lane = t & 63;
    const float *cloud = pc + c * n * 3;
    float *kept = kept_pc + c * n * 3;
    const unsigned long long slot = slot_offset + c;
    const unsigned long long key0 = mix64(mix64(seed + kGolden64) ^ counter);

    // thr = the drop-th smallest draw of the cloud: radix select, 8 bits a pass from the top.  Among the draws whose upper
    // bits equal `prefix`, the need-th smallest (1-based) is wanted; a pass counts them by their next 8 bits in LDS and wave 0
    // picks the bin that holds it.  The draws are distinct, so exactly `drop` of them are <= thr.
    unsigned long long thr = 0;
    if (drop > 0) {
        unsigned long long prefix = 0;
        unsigned need = (unsigned)drop;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (t < 256) S.hist[t] = 0u;
            __syncthreads();
            const unsigned long long upper = shift == 56 ? 0ull : ~0ull << (shift + 8);
            for (int p = t; p < n; p += DF_THREADS) {
                const unsigned long long r = srs_draw(key0, slot, p);
                if ((r & upper) == prefix) atomicAdd(&S.hist[(unsigned)(r >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (t < 64) {
                unsigned cb[4], sum = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { cb[j] = S.hist[4 * lane + j]; sum += cb[j]; }
                unsigned incl = sum;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const unsigned v = __shfl_up(incl, d, kWave);
                    incl += lane >= d ? v : 0u;
                }
                const unsigned long long reach = __ballot(incl >= need);       // never empty: at least `need` draws match the prefix
                if (reach != 0ull && lane == __ffsll((long long)reach) - 1) {
                    unsigned rem = need - (incl - sum);                         // in [1, sum]
                    unsigned digit = 4u * lane + 3u;
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        if (rem <= cb[j]) { digit = 4u * lane + j; break; }
                        rem -= cb[j];
                    }
                    S.prefix = prefix | ((unsigned long long)digit << shift);
                    S.need = rem;
                }
            }
            __syncthreads();
            prefix = S.prefix;
            need = S.need;
        }
        thr = prefix;
    }
    auto dropped = [&](int p) { return drop > 0 && srs_draw(key0, slot, p) <= thr; };
    if (dropped_idx && drop > 0) {
        int *dix = dropped_idx + c * drop;
        block_compact(n, L, dropped, [&](int p, int s) { if (s < drop) dix[s] = p; });
        __syncthreads();
    }
    const int nk = block_compact(n, L, [&](int p) { return !dropped(p); },
                                 [&](int p, int s) { copy_point(kept + 3 * (size_t)s, cloud + 3 * (size_t)p); });
    const int last = L.last;
    __syncthreads();
    pad_cloud(kept, cloud, nk, n, last);
}

static bool sd_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const char *pa = (const char *)a, *pb = (const char *)b;
    return pa < pb + nb && pb < pa + na;
}

}  // namespace geoadv

using namespace geoadv;

extern "C" int geoadv_sor_filter(int b, int n, const float *pc, const float *knn_dists, int knn_stride, int k, double alpha,
                                 float *outlier_pc, short *outlier_idx, short *outlier_num, float *inlier_pc, double *stats,
                                 void *stream) {
    GA_REQUIRE(b >= 0 && n >= 1 && n <= 32767, "sor_filter: bad dimensions (b=%d n=%d): b >= 0 and 1 <= n <= 32767 (the indices are int16)", b, n);
    GA_REQUIRE(k >= 1 && k <= knn_stride && knn_stride <= 64, "sor_filter: 1 <= k <= knn_stride <= 64 (got k=%d, knn_stride=%d)", k, knn_stride);
    GA_REQUIRE(alpha >= 0.0 && isfinite(alpha), "sor_filter: alpha must be finite and >= 0 (got %g)", alpha);
    if (b == 0) return GEOADV_OK;
    GA_REQUIRE(pc && knn_dists && inlier_pc, "sor_filter: null pointer");
    sor_filter_kernel<<<b, DF_THREADS, 0, as_stream(stream)>>>(n, pc, knn_dists, knn_stride, k, alpha * alpha, outlier_pc, outlier_idx,
                                                                outlier_num, inlier_pc, stats);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

extern "C" int geoadv_random_drop(int b, int n, const float *pc, int drop, unsigned long long seed, unsigned long long counter,
                                  unsigned long long slot_offset, float *kept_pc, int *dropped_idx, void *stream) {
    GA_REQUIRE(b >= 0 && n >= 1 && n <= 32767, "random_drop: bad dimensions (b=%d n=%d): b >= 0 and 1 <= n <= 32767", b, n);
    GA_REQUIRE(drop >= 0 && drop < n, "random_drop: drop=%d must be in [0, n=%d)", drop, n);
    GA_REQUIRE(slot_offset <= (1ull << 32) - (unsigned long long)b, "random_drop: slot_offset %llu + b %d exceeds 2^32 slots", slot_offset, b);
    if (b == 0) return GEOADV_OK;
    GA_REQUIRE(pc && kept_pc, "random_drop: null pointer");
    const size_t bytes = (size_t)b * n * 3 * sizeof(float);
    GA_REQUIRE(!sd_overlap(kept_pc, bytes, pc, bytes), "random_drop: kept_pc overlaps pc");
    random_drop_kernel<<<b, DF_THREADS, 0, as_stream(stream)>>>(n, pc, drop, seed, counter, slot_offset, kept_pc, dropped_idx);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
