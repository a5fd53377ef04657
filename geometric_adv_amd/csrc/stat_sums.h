// The float64 sums and the kNN score of the per-cloud statistics kernels (stat_defense.hip: sor_filter; knn_loss.hip:
// knn_outlier_loss): the fixed summation order of the SOR rule in include/geoadv.h, one 1024-thread workgroup per cloud.
#pragma once
#include "defense_pack.h"

namespace geoadv {

// the xor butterfly of wave_sum64 (dataset.hip): step 2 of the summation order of the rule
__device__ __forceinline__ double sd_wave_sum64(double v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// steps 2 and 3 of the summation order: the butterfly within every wave, then the wave sums in ascending order.  Every thread
// of the workgroup must call it; every thread gets the sum.
__device__ __forceinline__ double sd_block_sum64(double v, double *wsum /* LDS [DF_WAVES] */) {
    v = sd_wave_sum64(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    double total = wsum[0];
#pragma unroll
    for (int w = 1; w < DF_WAVES; ++w) total += wsum[w];
    __syncthreads();                                        // wsum is free for the next sum
    return total;
}

__device__ __forceinline__ double sor_score(const float *row, int k) {
    double s = (double)row[0];
    for (int j = 1; j < k; ++j) s += (double)row[j];
    return s / (double)k;
}

}  // namespace geoadv
