// The dataset stage's device operators.  sort_axes (src/shift_rotate_util.py:22-62), which the reference runs as a Python
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
//
// batch_gather: the training batch built on the device in one launch -- clouds gathered by index out of a resident array
// (clean = the bits of data[index[i]]), the fed copy with Gaussian noise or clipped jitter and a rotation (one matrix for the
// batch or one per cloud), in either order: noise then rotation is src/general_utils.py:124-144 (apply_augmentations), rotation
// then noise the classifier's provider order.  The rotation is batch.dot(R): the point as a row vector times R, products and
// sums in float64, rounded once to fp32 (as geoadv_rotate_y, cls_eval.hip).
//
// Noise of output slot s = slot_offset + i, point p, coordinate c (numpy's generator cannot be reproduced on the device; same
// distribution, Box-Muller on a counter-based generator; all integer arithmetic mod 2^64):
//   mix(z) = splitmix64's finaliser (common.h, mix64),  G = 0x9e3779b97f4a7c15 (kGolden64)
//   key    = mix(mix(mix(seed + G) ^ counter) ^ (s << 32 | p))
//   r      = mix(key + (c + 1) * G)
//   u1     = ((r >> 40) + 1) * 2^-24          in (0, 1]
//   u2     = ((r >> 16) & 0xFFFFFF) * 2^-24   in [0, 1)
//   g      = sqrt(-2 ln u1) * cos(2 pi u2)    fp32: logf, sqrtf, cospif(2 u2); u1, u2 and 2 u2 are exact in fp32
//   noise  = mu + clamp(sigma * g, -clip, clip)   (no clamp for clip <= 0);   value = x + noise
// sigma * g, mu + . and x + . are three fp32 roundings, never contracted.  sigma == 0: nothing is generated, mu is ignored and
// the value is x's bits.  The noise depends on (seed, counter, s, p, c) alone: not on b, the grid, the indices or the data, so
// data-parallel ranks that pass slot_offset = rank * local batch draw what one rank would have drawn for the whole batch.
//
// A thread owns one point, or -- in a call without noise, when n % 4 == 0 and every pointer is 16-byte aligned (rows are 12 n
// bytes, so only then does every row start on 16 bytes) -- four points through three 16-byte loads and stores per array, as
// rotate_y.  With noise the three draws of a point are the launch's critical path, not its bytes: at 50 x 2048 with noise,
// rotation and both outputs one point per thread took 4.2 us against 6.8 us for four (rocprofv3 kernel trace, MI355X), so the
// four-point form is kept for the copies and rotations.  Launch-bound at a batch's size; no LDS.  A source index outside
// [0, num_clouds) is never dereferenced; its slot stays unwritten.
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


constexpr int BG_THREADS = 256;
constexpr int BG_MAX_GRID_Y = 65535;

// the standard normal draw of (key, coordinate c): the file header's g
__device__ __forceinline__ float bg_normal(unsigned long long key, int c) {
    const unsigned long long r = mix64(key + (unsigned long long)(c + 1) * kGolden64);
    const float u1 = (float)((unsigned)(r >> 40) + 1u) * 0x1p-24f;
    const float u2x2 = (float)((unsigned)(r >> 16) & 0xFFFFFFu) * 0x1p-23f;
    return __fmul_rn(sqrtf(__fmul_rn(-2.f, logf(u1))), cospif(u2x2));
}

struct bg_params {
    unsigned long long seed, counter;
    int slot_offset;
    float mu, sigma, clip;
    int noise, rot_count, rotate_first;
};

__device__ __forceinline__ void bg_add_noise(const bg_params &P, unsigned long long slot, unsigned p, float &x, float &y, float &z) {
    const unsigned long long key = mix64(mix64(mix64(P.seed + kGolden64) ^ P.counter) ^ ((slot << 32) | (unsigned long long)p));
    float *v[3] = {&x, &y, &z};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float d = __fmul_rn(P.sigma, bg_normal(key, c));
        if (P.clip > 0.f) d = fminf(fmaxf(d, -P.clip), P.clip);
        *v[c] = __fadd_rn(*v[c], __fadd_rn(P.mu, d));
    }
}

// the row vector (x, y, z) times R (row-major): float64 products and sums, one rounding to fp32
__device__ __forceinline__ void bg_rotate(const double *R, float &x, float &y, float &z) {
    const double dx = x, dy = y, dz = z;
    x = (float)((dx * R[0] + dy * R[3]) + dz * R[6]);
    y = (float)((dx * R[1] + dy * R[4]) + dz * R[7]);
    z = (float)((dx * R[2] + dy * R[5]) + dz * R[8]);
}

template <bool NOISE>
__device__ __forceinline__ void bg_point(const bg_params &P, const double *R, unsigned long long slot, unsigned p, float &x, float &y, float &z) {
    if (P.rot_count && P.rotate_first) bg_rotate(R, x, y, z);
    if (NOISE && P.noise) bg_add_noise(P, slot, p, x, y, z);
    if (P.rot_count && !P.rotate_first) bg_rotate(R, x, y, z);
}

// grid: x over the point groups of a cloud (VEC: four points per thread, n % 4 == 0 and no noise; else one), y over the output clouds
template <bool VEC>
__global__ __launch_bounds__(BG_THREADS) void batch_gather_kernel(int b, int n, const float *data, long long num_clouds, const int *index,
                                                                  bg_params P, const double *rot, float *clean, float *feed) {
    const unsigned g = blockIdx.x * BG_THREADS + threadIdx.x;
    if (g >= (unsigned)(VEC ? n / 4 : n)) return;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const long long src_cloud = index ? (long long)index[i] : (long long)i;
        if (src_cloud < 0 || src_cloud >= num_clouds) continue;              // never dereferenced; the slot stays unwritten
        const float *src = data + (size_t)src_cloud * n * 3;
        const size_t row = (size_t)i * n * 3;
        const unsigned long long slot = (unsigned long long)(P.slot_offset + i);
        double R[9];
        if (P.rot_count) {
            const double *r = rot + (P.rot_count == 1 ? 0 : 9 * (size_t)i);
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = r[k];
        }
        if (VEC) {
            const float4 *s4 = reinterpret_cast<const float4 *>(src) + 3 * (size_t)g;
            float4 a = s4[0], c = s4[1], d = s4[2];
            if (clean) {
                float4 *c4 = reinterpret_cast<float4 *>(clean + row) + 3 * (size_t)g;
                c4[0] = a; c4[1] = c; c4[2] = d;
            }
            bg_point<false>(P, R, slot, 4 * g, a.x, a.y, a.z);
            bg_point<false>(P, R, slot, 4 * g + 1, a.w, c.x, c.y);
            bg_point<false>(P, R, slot, 4 * g + 2, c.z, c.w, d.x);
            bg_point<false>(P, R, slot, 4 * g + 3, d.y, d.z, d.w);
            float4 *f4 = reinterpret_cast<float4 *>(feed + row) + 3 * (size_t)g;
            f4[0] = a; f4[1] = c; f4[2] = d;
        } else {
            float x = src[3 * (size_t)g], y = src[3 * (size_t)g + 1], z = src[3 * (size_t)g + 2];
            if (clean) {
                float *cp = clean + row + 3 * (size_t)g;
                cp[0] = x; cp[1] = y; cp[2] = z;
            }
            bg_point<true>(P, R, slot, g, x, y, z);
            float *fp = feed + row + 3 * (size_t)g;
            fp[0] = x; fp[1] = y; fp[2] = z;
        }
    }
}

static inline bool bg_overlap(const float *a, size_t na, const float *b, size_t nb) {
    const size_t pa = reinterpret_cast<size_t>(a), pb = reinterpret_cast<size_t>(b);
    return pa < pb + 4 * nb && pb < pa + 4 * na;
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

extern "C" int geoadv_batch_gather(int b, int n, const float *data, long long num_clouds, const int *index, const geoadv_batch_augment *aug,
                                   const double *rot, float *clean, float *feed, void *stream) {
    GA_REQUIRE(b >= 1 && n >= 1 && num_clouds >= 1, "batch_gather: bad dimensions (b=%d, n=%d, num_clouds=%lld): all >= 1", b, n, num_clouds);
    GA_REQUIRE(data && feed, "batch_gather: null data or feed pointer");
    const size_t out_floats = (size_t)b * n * 3, data_floats = (size_t)num_clouds * n * 3;
    GA_REQUIRE(!bg_overlap(feed, out_floats, data, data_floats), "batch_gather: feed overlaps data");
    GA_REQUIRE(!clean || !bg_overlap(clean, out_floats, data, data_floats), "batch_gather: clean overlaps data");
    GA_REQUIRE(!clean || !bg_overlap(clean, out_floats, feed, out_floats), "batch_gather: clean overlaps feed");
    bg_params P = {};
    if (aug) {
        GA_REQUIRE(aug->rot_count == 0 || aug->rot_count == 1 || aug->rot_count == b,
                   "batch_gather: rot_count %d is neither 0, 1 nor the batch size %d", aug->rot_count, b);
        GA_REQUIRE(aug->rot_count == 0 || rot, "batch_gather: rot_count %d without rotation matrices", aug->rot_count);
        GA_REQUIRE(aug->slot_offset >= 0 && (long long)aug->slot_offset + b <= 0x7fffffffll, "batch_gather: slot_offset %d out of range", aug->slot_offset);
        GA_REQUIRE(aug->noise_sigma >= 0.f && aug->noise_sigma == aug->noise_sigma && aug->noise_mu == aug->noise_mu,
                   "batch_gather: noise_sigma must be >= 0 and noise_mu a number");
        P.seed = aug->seed; P.counter = aug->counter;
        P.slot_offset = aug->slot_offset;
        P.mu = aug->noise_mu; P.sigma = aug->noise_sigma; P.clip = aug->noise_clip;
        P.noise = aug->noise_sigma != 0.f;
        P.rot_count = aug->rot_count;
        P.rotate_first = aug->rotate_first ? 1 : 0;
    }
    const size_t align = reinterpret_cast<size_t>(data) | reinterpret_cast<size_t>(feed) | reinterpret_cast<size_t>(clean);
    const bool vec = !P.noise && n % 4 == 0 && (align & 15) == 0;
    const dim3 grid((unsigned)cdiv(vec ? n / 4 : n, BG_THREADS), (unsigned)std::min(b, BG_MAX_GRID_Y));
    if (vec)
        hipLaunchKernelGGL(batch_gather_kernel<true>, grid, dim3(BG_THREADS), 0, as_stream(stream), b, n, data, num_clouds, index, P, rot, clean, feed);
    else
        hipLaunchKernelGGL(batch_gather_kernel<false>, grid, dim3(BG_THREADS), 0, as_stream(stream), b, n, data, num_clouds, index, P, rot, clean, feed);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
