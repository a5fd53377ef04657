// The dataset stage's one device operator: sort_axes (src/shift_rotate_util.py:22-62), which the reference runs as a Python
// loop over the clouds before every training and evaluation run.  Per cloud: the x / y / z extents (max - min in fp32); the
// longer of x and y becomes x (z never moves); where x and y were swapped because x was STRICTLY shorter, axis int(neg_rot) of
// the result is negated, which makes the swap a rotation by -90 / +90 degrees about z instead of a reflection.
// One 256-thread workgroup per cloud (grid-stride over the clouds): pass 1 takes the four extremes of x and y per lane, per wave (DPP) and
// per workgroup (LDS); pass 2 re-reads the cloud (L2-resident: at most 192 KB) and writes it permuted.  Copies and sign flips
// only, so the output is the reference's bit for bit.
//
// The order is the reference's np.argsort([ex, ey, 0])[::-1] wherever the reference accepts the cloud: [0,1,2] for ex > ey,
// [1,0,2] for ex < ey and -- numpy's small-array sort being stable -- ALSO [1,0,2] for ex == ey > 0 (swapped, not negated).
// With an x or y extent of exactly 0 that expression moves z and the reference stops at its own assertion
// (shift_rotate_util.py:60); here the same rule goes on holding: swapped iff ex <= ey, negated iff ex < ey.
#include "common.h"

namespace geoadv {

constexpr int SA_THREADS = 256;
constexpr int SA_WAVES = SA_THREADS / kWave;
constexpr int SA_MAX_GRID = 65535;
constexpr int SA_MAX_N = 16384;

// np.minimum / np.maximum: a NaN operand wins (fminf / fmaxf would drop it), so a NaN coordinate gives a NaN extent as in numpy
template <bool MAX>
__device__ __forceinline__ float extreme(float a, float b) {
    return a != a ? a : (b != b ? b : (MAX ? fmaxf(a, b) : fminf(a, b)));
}

// min (MAX = false) or max over the 64 lanes of a wave; every lane gets it.  The DPP steps of wave_sum (common.h).
template <bool MAX>
__device__ __forceinline__ float wave_extreme(float v) {
#define GA_EXT_DPP(CTRL)                                                                                               \
    do {                                                                                                               \
        const float o_ = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));     \
        v = extreme<MAX>(v, o_);                                                                                       \
    } while (0)
    GA_EXT_DPP(0xB1);      // quad_perm [1,0,3,2]
    GA_EXT_DPP(0x4E);      // quad_perm [2,3,0,1]
    GA_EXT_DPP(0x141);     // row_half_mirror
    GA_EXT_DPP(0x140);     // row_mirror
#undef GA_EXT_DPP
    float r = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
#pragma unroll
    for (int row = 1; row < 4; ++row) {
        const float o = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16 * row));
        r = extreme<MAX>(r, o);
    }
    return r;
}

__global__ __launch_bounds__(SA_THREADS) void sort_axes_kernel(int b, int n, const float *pc, float *out, int *axes_idx, int neg_rot) {
    __shared__ float red[SA_WAVES][4];      // min x, min y, max x, max y (z never decides anything)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int c = blockIdx.x; c < b; c += gridDim.x) {
        const float *cloud = pc + (size_t)c * n * 3;
        float *dst = out + (size_t)c * n * 3;
        // lanes past the cloud's end keep point 0 (n >= 1): nothing outside [0, 3 n) is read
        float lo[2] = {cloud[0], cloud[1]};
        float hi[2] = {lo[0], lo[1]};
        for (int p = t; p < n; p += SA_THREADS) {
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float v = cloud[3 * (size_t)p + a];
                lo[a] = extreme<false>(lo[a], v);
                hi[a] = extreme<true>(hi[a], v);
            }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            lo[a] = wave_extreme<false>(lo[a]);
            hi[a] = wave_extreme<true>(hi[a]);
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < 2; ++a) { red[wave][a] = lo[a]; red[wave][2 + a] = hi[a]; }
        }
        __syncthreads();
        float ext[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            float l = red[0][a], h = red[0][2 + a];
#pragma unroll
            for (int w = 1; w < SA_WAVES; ++w) { l = extreme<false>(l, red[w][a]); h = extreme<true>(h, red[w][2 + a]); }
            ext[a] = h - l;
        }
        // argsort orders a NaN extent as the largest
        const bool swap = ext[1] != ext[1] || (ext[0] == ext[0] && ext[0] <= ext[1]);
        const bool flip = ext[0] < ext[1];
        if (axes_idx && t < 3) axes_idx[3 * (size_t)c + t] = t == 2 ? 2 : (swap ? 1 - t : t);
        for (int p = t; p < n; p += SA_THREADS) {
            const float x = cloud[3 * (size_t)p], y = cloud[3 * (size_t)p + 1], z = cloud[3 * (size_t)p + 2];
            float ox = swap ? y : x, oy = swap ? x : y;
            if (flip) { if (neg_rot) oy = -oy; else ox = -ox; }
            dst[3 * (size_t)p] = ox;
            dst[3 * (size_t)p + 1] = oy;
            dst[3 * (size_t)p + 2] = z;
        }
        __syncthreads();        // red[] is rewritten by the next cloud of this workgroup
    }
}

}  // namespace geoadv

using namespace geoadv;

extern "C" int geoadv_sort_axes(int b, int n, const float *pc, float *out, int *axes_idx, int neg_rot, void *stream) {
    GA_REQUIRE(b >= 1 && n >= 1 && n <= SA_MAX_N, "sort_axes: bad dimensions (b=%d, n=%d): b >= 1 and 1 <= n <= %d", b, n, SA_MAX_N);
    GA_REQUIRE(pc && out, "sort_axes: null pointer");
    GA_REQUIRE(pc != out, "sort_axes: in place is not supported");
    sort_axes_kernel<<<std::min(b, SA_MAX_GRID), SA_THREADS, 0, as_stream(stream)>>>(b, n, pc, out, axes_idx, neg_rot ? 1 : 0);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
