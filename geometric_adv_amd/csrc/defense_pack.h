// The packing helpers of the defense kernels (defense.hip: outlier_filter, critical_split; stat_defense.hip: sor_filter,
// random_drop): one 1024-thread workgroup per cloud, packing = wave ballots + a 16-entry LDS scan per 1024-point chunk, in
// point order.
#pragma once
#include "common.h"

namespace geoadv {

constexpr int DF_THREADS = 1024;
constexpr int DF_WAVES = DF_THREADS / 64;

struct CompactLds {
    int wcnt[DF_WAVES];
    int last;               // index of the last kept point so far (-1: none)
};

// Stable packing of the points p in [0, n) with keep(p): emit(p, slot) for slot = 0, 1, ... in point order.  Returns the
// number kept; L.last = the last kept point.  Every thread of the workgroup must call it.
template <class Keep, class Emit>
__device__ __forceinline__ int block_compact(int n, CompactLds &L, Keep keep, Emit emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) L.last = -1;
    int base = 0;
    for (int p0 = 0; p0 < n; p0 += DF_THREADS) {
        const int p = p0 + threadIdx.x;
        const bool f = p < n && keep(p);
        const unsigned long long bal = __ballot(f);
        if (lane == 0) L.wcnt[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < DF_WAVES; ++w) {
            const int cw = L.wcnt[w];
            before += w < wave ? cw : 0;
            total += cw;
        }
        if (f) {
            const int r = before + __popcll(bal & ((1ull << lane) - 1ull));
            emit(p, base + r);
            if (r == total - 1) L.last = p;
        }
        base += total;
        __syncthreads();
    }
    return base;
}

__device__ __forceinline__ void copy_point(float *dst, const float *src) { dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2]; }

// slots [count, n) of a packed cloud: the last packed point again (adversary_utils.py:168-169,175-176; ae_utils.py:71,77),
// zeros when nothing was packed (the reference's arrays start as zeros)
__device__ __forceinline__ void pad_cloud(float *dst, const float *cloud, int count, int n, int last) {
    float px = 0.f, py = 0.f, pz = 0.f;
    if (count > 0) { px = cloud[3 * last]; py = cloud[3 * last + 1]; pz = cloud[3 * last + 2]; }
    for (int s = count + threadIdx.x; s < n; s += DF_THREADS) { dst[3 * s] = px; dst[3 * s + 1] = py; dst[3 * s + 2] = pz; }
}

}  // namespace geoadv
