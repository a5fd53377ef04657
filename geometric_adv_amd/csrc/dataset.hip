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
//
// normalize_clouds: AtlasNet's Normalization (transfer/atlasnet/dataset/pointcloud_processor.py:160-233) to the unit ball or
// the bounding box, out = (x - c) * s per cloud.  One 256-thread workgroup per cloud, grid-stride, as sort_axes.  The mean is
// a float64 sum in a fixed order -- thread t adds points t, t + 256, ... in ascending order, the 64 lanes of a wave combine
// in a butterfly (commutative at every step, so all lanes hold the same bits), the four waves are added in ascending order
// out of LDS -- so c and s do not depend on the grid or the run.  The extrema are extreme<> / wave_extreme<> (a NaN wins);
// the unit ball's largest squared distance is a float64 maximum with the same rule.  The cloud is read again for every pass
// (unit ball: three, bounding box: two): 30 000 points are 360 KB and stay in L2; no LDS staging.  (x - c) * s is evaluated
// in float64 and rounded to fp32 once, as bg_rotate.
//
// augment_batch: AtlasNet's training batch in one launch -- gather by index, re-sampling with replacement
// (dataset_shapenet.py:213-215), then the Augmenter's operators in its order (dataset/augmenter.py): axial rotations, 3-D
// rotation, anisotropic scale, flips, translation.  Draws of output slot s = slot_offset + i, with mix and G as above:
//   r(q, k) = mix(mix(mix(mix(seed + G) ^ counter) ^ (s << 32 | q)) + k * G)      q = 0 for the operators; k = the stream
//   u(k)    = (r >> 40) * 2^-24                      in [0, 1), 24 bits as torch's fp32 rand
//   g(k)    = sqrt(-2 ln(((r >> 40) + 1) * 2^-24)) * cos(2 pi ((r >> 16) & 0xFFFFFF) * 2^-24)     float64
//   axial rotation about a   k = 16 + a   angle = u * 2K - K,  K = pi * range_rot / 360 (float64); with c, s its cosine and
//                                         sine and i < j the two other axes: M[a][a] = 1, M[i][i] = M[j][j] = c, M[i][j] = s,
//                                         M[j][i] = -s   (Operation.get_3D_rot_matrix)
//   3-D rotation             k = 19 + a   x = (g(19), g(20), g(21)) / sqrt(g(19)^2 + g(20)^2 + g(21)^2)
//                            k = 22       angle = u * 2 pi + pi, c and s its cosine and sine, XX = x x^T:
//                                         M[a][a] = c + XX[a][a] (1 - c);  M[0][1] = XX[0][1] (1 - c) - x[2] s,  M[1][0] = . + x[2] s;
//                                         M[0][2] = XX[0][2] (1 - c) + x[1] s,  M[2][0] = . - x[1] s;  M[1][2] = XX[1][2] (1 - c) - x[0] s,
//                                         M[2][1] = . + x[0] s     (DataAugmentation.get_random_rotation_matrix, lines 276-302)
//   scale of axis a          k = 23 + a   u * (scale_max - scale_min) + scale_min        fp32: subtract, multiply, add, each rounded
//   flip of axis a           k = 26 + a   +1 where bit 63 of r is set, else -1
//   translation of axis a    k = 29 + a   (u * 2) * translate_scale - translate_scale    fp32, each rounded
//   source point of point p  k = 32, q = p   j = ((r >> 32) * n_src) >> 32               integers only
// Angles, cos / sin, sqrt and ln are float64; every matrix entry is rounded to fp32 once, because the reference applies fp32
// operators (it casts even the double-built 3-D matrix with .type(self.type)).  The draws depend on (seed, counter, s, k, p)
// alone, not on b, the grid, the indices or the data.  The noise of batch_gather uses streams 1..3 of the same key; the
// operators start at 16.
// Per workgroup the record of a cloud is built once in LDS -- lanes 0..2 of wave 0 the axial matrices, lane 0 of wave 1 the
// 3-D matrix, lanes 0..2 of wave 2 scale, flip and translation, so the three kinds of float64 work run side by side and no
// other lane computes a transcendental -- and thread 0 composes the fp32 operators in float64 into one affine map x M + t.
// A thread owns one output point: x M + t in float64, rounded once.  With no operator enabled the point's bits are copied.
// Launch- and latency-bound at a batch's size (32 x 2048 points are 0.8 MB in and 0.8 MB out): the time is the launch and the
// one lane's chain of float64 transcendentals, not the bytes -- 12.2 us per call as a plain gather, 13.9 us with all five
// operators, output allocation and launch included (tools/atlas_loader_time.py, MI355X); not tuned beyond that.
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


constexpr int NC_MAX_N = 1 << 20;

// the float64 maximum / minimum with extreme<>'s rule: a NaN operand wins
template <bool MAX>
__device__ __forceinline__ double extreme(double a, double b) {
    return a != a ? a : (b != b ? b : (MAX ? fmax(a, b) : fmin(a, b)));
}

// the sum over the 64 lanes of a wave in float64: a butterfly, whose every step adds the same two values on both sides, so all
// lanes end with the same bits and the order is fixed
__device__ __forceinline__ double wave_sum64(double v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

__device__ __forceinline__ double wave_max64(double v) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) v = extreme<true>(v, __shfl_xor(v, m, kWave));
    return v;
}

__global__ __launch_bounds__(SA_THREADS) void normalize_clouds_kernel(int b, int n, int kind, const float *pc, float *out) {
    __shared__ double sum[SA_WAVES][3];     // the waves' coordinate sums, then (in [.][0]) their largest squared distance
    __shared__ float red[SA_WAVES][6];      // min x, y, z, max x, y, z
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int c = blockIdx.x; c < b; c += gridDim.x) {
        const float *cloud = pc + (size_t)c * n * 3;
        float *dst = out + (size_t)c * n * 3;
        if (kind == GEOADV_NORMALIZE_IDENTITY) {
            for (int p = t; p < 3 * n; p += SA_THREADS) dst[p] = cloud[p];
            continue;
        }
        double ctr[3], s;
        if (kind == GEOADV_NORMALIZE_UNIT_BALL) {
            double acc[3] = {0.0, 0.0, 0.0};
            for (int p = t; p < n; p += SA_THREADS) {
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] += (double)cloud[3 * (size_t)p + a];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                acc[a] = wave_sum64(acc[a]);
                if (lane == 0) sum[wave][a] = acc[a];
            }
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double v = sum[0][a];
#pragma unroll
                for (int w = 1; w < SA_WAVES; ++w) v += sum[w][a];
                ctr[a] = v / (double)n;
            }
            __syncthreads();        // sum[] is rewritten below
            double far = 0.0;       // squared distances are >= 0 or NaN
            for (int p = t; p < n; p += SA_THREADS) {
                const double dx = (double)cloud[3 * (size_t)p] - ctr[0], dy = (double)cloud[3 * (size_t)p + 1] - ctr[1],
                             dz = (double)cloud[3 * (size_t)p + 2] - ctr[2];
                far = extreme<true>(far, (dx * dx + dy * dy) + dz * dz);
            }
            far = wave_max64(far);
            if (lane == 0) sum[wave][0] = far;
            __syncthreads();
            double v = sum[0][0];
#pragma unroll
            for (int w = 1; w < SA_WAVES; ++w) v = extreme<true>(v, sum[w][0]);
            s = 1.0 / sqrt(v);
        } else {
            // lanes past the cloud's end keep point 0 (n >= 1): nothing outside [0, 3 n) is read
            float lo[3] = {cloud[0], cloud[1], cloud[2]};
            float hi[3] = {lo[0], lo[1], lo[2]};
            for (int p = t; p < n; p += SA_THREADS) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float v = cloud[3 * (size_t)p + a];
                    lo[a] = extreme<false>(lo[a], v);
                    hi[a] = extreme<true>(hi[a], v);
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lo[a] = wave_extreme<false>(lo[a]);
                hi[a] = wave_extreme<true>(hi[a]);
                if (lane == 0) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
            }
            __syncthreads();
            double half = 0.0;      // half extents are >= 0 or NaN
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                float l = red[0][a], h = red[0][3 + a];
#pragma unroll
                for (int w = 1; w < SA_WAVES; ++w) { l = extreme<false>(l, red[w][a]); h = extreme<true>(h, red[w][3 + a]); }
                ctr[a] = ((double)l + (double)h) / 2.0;
                half = extreme<true>(half, ((double)h - (double)l) / 2.0);
            }
            s = 1.0 / half;
        }
        for (int p = t; p < n; p += SA_THREADS) {
#pragma unroll
            for (int a = 0; a < 3; ++a) dst[3 * (size_t)p + a] = (float)(((double)cloud[3 * (size_t)p + a] - ctr[a]) * s);
        }
        __syncthreads();        // sum[] and red[] are rewritten by the next cloud of this workgroup
    }
}


constexpr int AB_THREADS = 256;
constexpr int AB_MAX_GRID_Y = 65535;
constexpr int AB_RECORD = GEOADV_AUGMENT_RECORD;
// the record's layout (include/geoadv.h) and the streams of the file header
constexpr int AB_AXIAL = 0, AB_ROT3D = 27, AB_SCALE = 36, AB_FLIP = 39, AB_TRANS = 42;
constexpr int AB_K_AXIAL = 16, AB_K_NORMAL = 19, AB_K_ANGLE = 22, AB_K_SCALE = 23, AB_K_FLIP = 26, AB_K_TRANS = 29, AB_K_SAMPLE = 32;

struct ab_params {
    unsigned long long seed, counter;
    int slot_offset, sample, rot_axes, rot_3d, scale, flip_axes, translate, any_op;
    float range_rot, scale_min, scale_max, translate_scale;
};

// the file header's r(q, k)
__device__ __forceinline__ unsigned long long ab_draw(const ab_params &P, unsigned long long slot, unsigned q, int k) {
    return mix64(mix64(mix64(mix64(P.seed + kGolden64) ^ P.counter) ^ ((slot << 32) | (unsigned long long)q)) + (unsigned long long)k * kGolden64);
}

// u: 24 bits, exact in fp32 and in float64
__device__ __forceinline__ float ab_uniform(unsigned long long r) { return (float)(unsigned)(r >> 40) * 0x1p-24f; }

__device__ __forceinline__ double ab_normal(unsigned long long r) {
    const double u1 = (double)((unsigned)(r >> 40) + 1u) * 0x1p-24;
    const double u2 = (double)((unsigned)(r >> 16) & 0xFFFFFFu) * 0x1p-24;
    return sqrt(-2.0 * log(u1)) * cos((2.0 * M_PI) * u2);
}

// what element e of a record holds where its operator is off
__device__ __forceinline__ float ab_identity(int e) { return e < AB_SCALE ? ((e % 9) % 4 == 0 ? 1.f : 0.f) : (e < AB_TRANS ? 1.f : 0.f); }

__device__ __forceinline__ bool ab_enabled(const ab_params &P, int e) {
    if (e < AB_ROT3D) return (P.rot_axes >> (e / 9)) & 1;
    if (e < AB_SCALE) return P.rot_3d != 0;
    if (e < AB_FLIP) return P.scale != 0;
    if (e < AB_TRANS) return (P.flip_axes >> (e - AB_FLIP)) & 1;
    return P.translate != 0;
}

// the drawn operators of `slot` into the record op[] (LDS, already holding the identities): three waves, one kind of work each
__device__ __forceinline__ void ab_draw_record(const ab_params &P, unsigned long long slot, float *op) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave == 0 && lane < 3 && ((P.rot_axes >> lane) & 1)) {
        const int a = lane, i = a == 0 ? 1 : 0, j = a == 2 ? 1 : 2;
        const double K = M_PI * (double)P.range_rot / 360.0;
        const double angle = (double)ab_uniform(ab_draw(P, slot, 0, AB_K_AXIAL + a)) * (2.0 * K) - K;
        const float c = (float)cos(angle), s = (float)sin(angle);
        float *M = op + AB_AXIAL + 9 * a;
        M[3 * i + i] = c; M[3 * i + j] = s;
        M[3 * j + i] = -s; M[3 * j + j] = c;
    } else if (wave == 1 && lane == 0 && P.rot_3d) {
        double x[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] = ab_normal(ab_draw(P, slot, 0, AB_K_NORMAL + a));
        const double norm = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a) x[a] /= norm;
        const double angle = (double)ab_uniform(ab_draw(P, slot, 0, AB_K_ANGLE)) * (2.0 * M_PI) + M_PI;
        const double c = cos(angle), s = sin(angle), v = 1.0 - c;
        float *M = op + AB_ROT3D;
        M[0] = (float)(c + (x[0] * x[0]) * v);
        M[4] = (float)(c + (x[1] * x[1]) * v);
        M[8] = (float)(c + (x[2] * x[2]) * v);
        M[1] = (float)((x[0] * x[1]) * v - x[2] * s);
        M[3] = (float)((x[0] * x[1]) * v + x[2] * s);
        M[2] = (float)((x[0] * x[2]) * v + x[1] * s);
        M[6] = (float)((x[0] * x[2]) * v - x[1] * s);
        M[5] = (float)((x[1] * x[2]) * v - x[0] * s);
        M[7] = (float)((x[1] * x[2]) * v + x[0] * s);
    } else if (wave == 2 && lane < 3) {
        const int a = lane;
        if (P.scale)
            op[AB_SCALE + a] = __fadd_rn(__fmul_rn(ab_uniform(ab_draw(P, slot, 0, AB_K_SCALE + a)), __fsub_rn(P.scale_max, P.scale_min)), P.scale_min);
        if ((P.flip_axes >> a) & 1) op[AB_FLIP + a] = (ab_draw(P, slot, 0, AB_K_FLIP + a) >> 63) ? 1.f : -1.f;
        if (P.translate)
            op[AB_TRANS + a] = __fsub_rn(__fmul_rn(__fmul_rn(ab_uniform(ab_draw(P, slot, 0, AB_K_TRANS + a)), 2.f), P.translate_scale), P.translate_scale);
    }
}

// the record's fp32 operators composed in float64: a point x (row vector) becomes x M + t, M = aff[0..9) row-major, t = aff[9..12)
__device__ __forceinline__ void ab_compose(const float *op, double *aff) {
    double M[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    for (int k = 0; k < 4; ++k) {           // the three axial matrices, then the 3-D one
        const float *R = op + 9 * k;
        double N[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                N[3 * r + c] = (M[3 * r] * (double)R[c] + M[3 * r + 1] * (double)R[3 + c]) + M[3 * r + 2] * (double)R[6 + c];
#pragma unroll
        for (int e = 0; e < 9; ++e) M[e] = N[e];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) aff[3 * r + c] = (M[3 * r + c] * (double)op[AB_SCALE + c]) * (double)op[AB_FLIP + c];
#pragma unroll
    for (int c = 0; c < 3; ++c) aff[9 + c] = (double)op[AB_TRANS + c];
}

// grid: x over the output points of a cloud, one per thread; y over the output clouds
__global__ __launch_bounds__(AB_THREADS) void augment_batch_kernel(int b, int n_out, const float *data, long long num_clouds, int n_src,
                                                                   const int *index, ab_params P, const float *params, float *params_out,
                                                                   float *out) {
    __shared__ float op[AB_RECORD];
    __shared__ double aff[12];
    const int t = threadIdx.x;
    const unsigned g = blockIdx.x * AB_THREADS + t;
    for (int i = blockIdx.y; i < b; i += gridDim.y) {
        const long long src_cloud = index ? (long long)index[i] : (long long)i;
        if (src_cloud < 0 || src_cloud >= num_clouds) continue;              // never dereferenced; the slot stays unwritten (uniform: no barrier is skipped by some)
        const unsigned long long slot = (unsigned long long)(P.slot_offset + i);
        if (P.any_op) {
            if (t < AB_RECORD) op[t] = (params && ab_enabled(P, t)) ? params[(size_t)i * AB_RECORD + t] : ab_identity(t);
            if (!params) {
                __syncthreads();
                ab_draw_record(P, slot, op);
            }
            __syncthreads();
            if (t == 0) ab_compose(op, aff);
            if (params_out && blockIdx.x == 0 && t < AB_RECORD) params_out[(size_t)i * AB_RECORD + t] = op[t];
            __syncthreads();
        } else if (params_out && blockIdx.x == 0 && t < AB_RECORD) {
            params_out[(size_t)i * AB_RECORD + t] = ab_identity(t);
        }
        if (g < (unsigned)n_out) {
            const unsigned long long j = P.sample ? ((ab_draw(P, slot, g, AB_K_SAMPLE) >> 32) * (unsigned long long)n_src) >> 32 : g;
            const float *src = data + ((size_t)src_cloud * n_src + j) * 3;
            float x = src[0], y = src[1], z = src[2];
            if (P.any_op) {
                const double dx = x, dy = y, dz = z;
                x = (float)(((dx * aff[0] + dy * aff[3]) + dz * aff[6]) + aff[9]);
                y = (float)(((dx * aff[1] + dy * aff[4]) + dz * aff[7]) + aff[10]);
                z = (float)(((dx * aff[2] + dy * aff[5]) + dz * aff[8]) + aff[11]);
            }
            float *dst = out + ((size_t)i * n_out + g) * 3;
            dst[0] = x; dst[1] = y; dst[2] = z;
        }
        if (P.any_op) __syncthreads();          // op[] and aff[] are rewritten by the next cloud of this workgroup
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
    const size_t align = reinterpret_cast<size_t>(data) | reinterpret_cast<size_t>(feed) | reinterpret_cast<size_t>(clean);    const bool vec = !P.noise && n % 4 == 0 && (align & 15) == 0;
    const dim3 grid((unsigned)cdiv(vec ? n / 4 : n, BG_THREADS), (unsigned)std::min(b, BG_MAX_GRID_Y));
    if (vec)
        hipLaunchKernelGGL(batch_gather_kernel<true>, grid, dim3(BG_THREADS), 0, as_stream(stream), b, n, data, num_clouds, index, P, rot, clean, feed);
    else
        hipLaunchKernelGGL(batch_gather_kernel<false>, grid, dim3(BG_THREADS), 0, as_stream(stream), b, n, data, num_clouds, index, P, rot, clean, feed);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

extern "C" int geoadv_normalize_clouds(int b, int n, int kind, const float *pc, float *out, void *stream) {
    GA_REQUIRE(b >= 1 && n >= 1 && n <= NC_MAX_N, "normalize_clouds: bad dimensions (b=%d, n=%d): b >= 1 and 1 <= n <= %d", b, n, NC_MAX_N);
    GA_REQUIRE(kind == GEOADV_NORMALIZE_IDENTITY || kind == GEOADV_NORMALIZE_UNIT_BALL || kind == GEOADV_NORMALIZE_BOUNDING_BOX,
               "normalize_clouds: kind %d is neither identity (0), unit ball (1) nor bounding box (2)", kind);
    GA_REQUIRE(pc && out, "normalize_clouds: null pointer");
    const size_t floats = (size_t)b * n * 3;
    GA_REQUIRE(!bg_overlap(pc, floats, out, floats), "normalize_clouds: in place is not supported (out overlaps pc)");
    normalize_clouds_kernel<<<std::min(b, SA_MAX_GRID), SA_THREADS, 0, as_stream(stream)>>>(b, n, kind, pc, out);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

extern "C" int geoadv_augment_batch(int b, int n_out, const float *data, long long num_clouds, int n_src, const int *index,
                                    const geoadv_cloud_augment *cfg, const float *params, float *params_out, float *out, void *stream) {
    GA_REQUIRE(b >= 1 && n_out >= 1 && n_out <= (1 << 30) && n_src >= 1 && num_clouds >= 1,
               "augment_batch: bad dimensions (b=%d, n_out=%d, n_src=%d, num_clouds=%lld): all >= 1, n_out <= 2^30", b, n_out, n_src, num_clouds);
    GA_REQUIRE(data && out, "augment_batch: null data or out pointer");
    const size_t out_floats = (size_t)b * n_out * 3, data_floats = (size_t)num_clouds * n_src * 3, rec_floats = (size_t)b * AB_RECORD;
    GA_REQUIRE(!bg_overlap(out, out_floats, data, data_floats), "augment_batch: out overlaps data");
    GA_REQUIRE(!params_out || (!bg_overlap(params_out, rec_floats, data, data_floats) && !bg_overlap(params_out, rec_floats, out, out_floats) &&
                               (!params || !bg_overlap(params_out, rec_floats, params, rec_floats))),
               "augment_batch: params_out overlaps data, out or params");
    GA_REQUIRE(!params || !bg_overlap(out, out_floats, params, rec_floats), "augment_batch: out overlaps params");
    ab_params P = {};
    if (cfg) {
        GA_REQUIRE(cfg->slot_offset >= 0 && (long long)cfg->slot_offset + b <= 0x7fffffffll, "augment_batch: slot_offset %d out of range", cfg->slot_offset);
        GA_REQUIRE(cfg->rot_axes >= 0 && cfg->rot_axes <= 7 && cfg->flip_axes >= 0 && cfg->flip_axes <= 7,
                   "augment_batch: rot_axes %d and flip_axes %d are bit sets of the axes 0..2", cfg->rot_axes, cfg->flip_axes);
        GA_REQUIRE(!cfg->rot_axes || (cfg->range_rot > 0.f && cfg->range_rot <= 360.f), "augment_batch: range_rot %g outside (0, 360]", (double)cfg->range_rot);
        GA_REQUIRE(!cfg->scale || (std::isfinite(cfg->scale_min) && std::isfinite(cfg->scale_max) && cfg->scale_min <= cfg->scale_max),
                   "augment_batch: scale_min %g > scale_max %g, or one of them is not finite", (double)cfg->scale_min, (double)cfg->scale_max);
        GA_REQUIRE(!cfg->translate || (std::isfinite(cfg->translate_scale) && cfg->translate_scale >= 0.f),
                   "augment_batch: translate_scale %g is negative or not finite", (double)cfg->translate_scale);
        P.seed = cfg->seed; P.counter = cfg->counter;
        P.slot_offset = cfg->slot_offset;
        P.sample = cfg->sample ? 1 : 0;
        P.rot_axes = cfg->rot_axes; P.range_rot = cfg->range_rot;
        P.rot_3d = cfg->rot_3d ? 1 : 0;
        P.scale = cfg->scale ? 1 : 0; P.scale_min = cfg->scale_min; P.scale_max = cfg->scale_max;
        P.flip_axes = cfg->flip_axes;
        P.translate = cfg->translate ? 1 : 0; P.translate_scale = cfg->translate_scale;
        P.any_op = (P.rot_axes || P.rot_3d || P.scale || P.flip_axes || P.translate) ? 1 : 0;
    }
    GA_REQUIRE(P.sample || n_out == n_src, "augment_batch: n_out %d != n_src %d without sampling", n_out, n_src);
    const dim3 grid((unsigned)cdiv(n_out, AB_THREADS), (unsigned)std::min(b, AB_MAX_GRID_Y));
    hipLaunchKernelGGL(augment_batch_kernel, grid, dim3(AB_THREADS), 0, as_stream(stream), b, n_out, data, num_clouds, n_src, index, P, params,
                       params_out, out);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
