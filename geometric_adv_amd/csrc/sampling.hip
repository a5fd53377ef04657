// Farthest point sampling (include/geoadv.h: geoadv_farthest_point_sample), gfx950.
//
// The chain is m picks long and every pick is an arg-max over the whole cloud, so a cloud never leaves its compute unit: its
// coordinates and the running squared distance t to the chosen set stay in registers from the first pick to the last, and one
// launch serves the whole batch.  Two forms of one kernel template, identical bits:
//   workgroup per cloud  NW waves (4, 8 or 16) share a cloud; per pick one LDS slot per wave and ONE barrier
//   wave per cloud       n <= 1024: a wave owns its cloud, four clouds share a workgroup, no LDS and no barrier in the loop
// Thread j of a cloud's T threads holds the points j, j + T, j + 2T, ...: ascending in its register block, so "first larger t
// wins" inside a thread and "larger t, then lower index" across lanes and waves give the lowest index among equals.
// The pick's coordinates are re-read from xyz by index at the top of the next step (a wave-uniform address, so one scalar-cache /
// L2 hit per wave): DESIGN.md "Farthest point sampling" says why they are not carried through the reduction.
#include <cmath>
#include "common.h"

namespace geoadv {

constexpr int FPS_MAX_N = 16384;
constexpr int FPS_WAVE_MAX_N = 1024;    // the largest cloud one wave holds (16 points per lane)
constexpr int FPS_WAVE_AUTO_N = 256;    // form 0 (auto): clouds up to here go to the wave-per-cloud form
constexpr int FPS_WAVE_CLOUDS = 4;      // clouds (= waves) per workgroup in the wave-per-cloud form
constexpr int FPS_MAX_WAVES = 16;

// The reduction operator "larger t, then lower index" in two 32-bit passes, each four DPP steps that fuse into the v_max / v_min
// itself: the largest t, then the lowest index among the lanes that hold it.  t is never NaN and is -1 or >= +0, so its bits
// order as a SIGNED integer the way the floats do.
constexpr int FPS_T_NONE = (int)0x80000000, FPS_INDEX_NONE = 0x7fffffff;    // a lane that holds nothing: below / above every value

#define FPS_ROW_REDUCE(OP, v)                                                          \
    do {                                                                               \
        v = OP(v, __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true));  /* quad_perm [1,0,3,2] */ \
        v = OP(v, __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true));  /* quad_perm [2,3,0,1] */ \
        v = OP(v, __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true)); /* row_half_mirror */     \
        v = OP(v, __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true)); /* row_mirror */          \
    } while (0)

// over a row of 16 lanes; every lane of the row ends up with the row's (largest t bits, lowest index that holds them)
__device__ __forceinline__ void row_best(int &tb, int &index) {
    int top = tb;
    FPS_ROW_REDUCE(max, top);
    index = tb == top ? index : FPS_INDEX_NONE;
    FPS_ROW_REDUCE(min, index);
    tb = top;
}

// over the 64 lanes of a wave: the four rows by DPP, v_readlane collects them (wave-uniform results)
__device__ __forceinline__ void wave_best(int &tb, int &index) {
    int top = tb;
    FPS_ROW_REDUCE(max, top);
    top = max(max(__builtin_amdgcn_readlane(top, 0), __builtin_amdgcn_readlane(top, 16)),
              max(__builtin_amdgcn_readlane(top, 32), __builtin_amdgcn_readlane(top, 48)));
    index = tb == top ? index : FPS_INDEX_NONE;
    FPS_ROW_REDUCE(min, index);
    index = min(min(__builtin_amdgcn_readlane(index, 0), __builtin_amdgcn_readlane(index, 16)),
                min(__builtin_amdgcn_readlane(index, 32), __builtin_amdgcn_readlane(index, 48)));
    tb = top;
}
#undef FPS_ROW_REDUCE

// NW waves per cloud, PPT points per thread, CPW clouds per workgroup (CPW > 1 only with NW == 1).  n <= NW * 64 * PPT.
template <int NW, int PPT, int CPW>
__global__ void __launch_bounds__(NW * kWave * CPW)
fps_kernel(int b, int n, const float *__restrict__ xyz, int m, const int *__restrict__ start, int *__restrict__ idx,
           float *__restrict__ sampled, float *__restrict__ mindist) {
    static_assert(NW == 1 || CPW == 1, "several clouds per workgroup only in the wave-per-cloud form");
    static_assert(NW <= FPS_MAX_WAVES, "one row of 16 lanes reduces the per-wave slots");
    constexpr int T = NW * kWave;                   // threads of one cloud
    const int j = threadIdx.x % T;
    const int cloud = CPW == 1 ? (int)blockIdx.x : (int)blockIdx.x * CPW + __builtin_amdgcn_readfirstlane(threadIdx.x / T);
    if (cloud >= b) return;                         // whole waves, and only where the loop has no barrier
    const float *X = xyz + (size_t)cloud * n * 3;

    // the cloud: a point with a non-finite coordinate, and a slot past the cloud's end, carry t = -1 and can never win
    float x[PPT], y[PPT], z[PPT], t[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int i = k * T + j;
        x[k] = y[k] = z[k] = 0.f;
        if (i < n) {
            x[k] = X[3 * (size_t)i];
            y[k] = X[3 * (size_t)i + 1];
            z[k] = X[3 * (size_t)i + 2];
        }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k)                   // after the loads, so that they are all in flight together
        t[k] = k * T + j < n && std::isfinite(x[k]) && std::isfinite(y[k]) && std::isfinite(z[k]) ? INFINITY : -1.f;

    int cur = start ? __builtin_amdgcn_readfirstlane(start[cloud]) : 0;
    if (cur < 0 || cur >= n) cur = 0;
    __shared__ int2 slot[2][FPS_MAX_WAVES];         // (t bits, index) per wave; two sets, by the step's parity: one barrier per step

    for (int s = 0; s < m; ++s) {
        const float cx = X[3 * (size_t)cur], cy = X[3 * (size_t)cur + 1], cz = X[3 * (size_t)cur + 2];
        if (j == 0) {
            idx[(size_t)cloud * m + s] = cur;
            if (sampled) {
                float *o = sampled + ((size_t)cloud * m + s) * 3;
                o[0] = cx; o[1] = cy; o[2] = cz;
            }
        }
        // t = min(t, squared distance to the pick); d is +inf or NaN next to a non-finite coordinate and then replaces nothing
        // (a compare and a select: fminf is two instructions as well, a canonicalising v_max before its v_min, and measured the same)
        float bt = 0.f;
        int bk = 0;
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float dx = x[k] - cx, dy = y[k] - cy, dz = z[k] - cz;
            const float d = (dx * dx + dy * dy) + dz * dz;
            t[k] = d < t[k] ? d : t[k];
            const bool up = k == 0 || t[k] > bt;
            bt = up ? t[k] : bt;
            bk = up ? k : bk;
        }
        int tb = __float_as_int(bt), bi = bk * T + j;
        wave_best(tb, bi);
        if (NW > 1) {
            const int p = s & 1;
            if (j % kWave == 0) slot[p][j / kWave] = make_int2(tb, bi);
            __syncthreads();
            const int l = j & 15;                   // every row of every wave reduces the NW slots for itself
            const int2 c = l < NW ? slot[p][l] : make_int2(FPS_T_NONE, FPS_INDEX_NONE);
            tb = c.x;
            bi = c.y;
            row_best(tb, bi);
        }
        // the next pick; < n, because a slot past the cloud's end ties with t = -1 at best and has the higher index.  The
        // reduction after the last pick is wasted once per call and keeps the loop free of an exit in its middle.
        cur = __builtin_amdgcn_readfirstlane(bi);
    }

    if (mindist) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const int i = k * T + j;
            if (i < n) mindist[(size_t)cloud * n + i] = t[k];
        }
    }
}

struct fps_plan {
    int form, waves, ppt;   // form 1 = workgroup per cloud, 2 = wave per cloud; the cloud's waves; points per thread
};

// The instance that answers a cloud of n points: the fewest registers that hold it, and in the workgroup form more waves
// before more points per thread (the per-thread loop is the serial part of a pick).
static bool fps_choose(int n, int form, fps_plan *p) {
    if (n < 1 || n > FPS_MAX_N || form < 0 || form > 2) return false;
    if (form == 0) form = n <= FPS_WAVE_AUTO_N ? 2 : 1;
    if (form == 2) {
        if (n > FPS_WAVE_MAX_N) return false;
        *p = {2, 1, n <= 64 ? 1 : n <= 256 ? 4 : 16};
    } else if (n <= 256) *p = {1, 4, 1};
    else if (n <= 1024) *p = {1, 4, 4};
    else if (n <= 2048) *p = {1, 8, 4};
    else if (n <= 4096) *p = {1, 16, 4};
    else if (n <= 8192) *p = {1, 16, 8};
    else *p = {1, 16, 16};
    return true;
}

template <int NW, int PPT, int CPW>
static void fps_launch(int b, int n, const float *xyz, int m, const int *start, int *idx, float *sampled, float *mindist, hipStream_t st) {
    hipLaunchKernelGGL((fps_kernel<NW, PPT, CPW>), dim3((unsigned)cdiv(b, CPW)), dim3(NW * kWave * CPW), 0, st, b, n, xyz, m, start, idx, sampled,
                       mindist);
}

static inline bool fps_overlap(const void *a, size_t bytes_a, const void *b, size_t bytes_b) {
    const size_t pa = reinterpret_cast<size_t>(a), pb = reinterpret_cast<size_t>(b);
    return pa < pb + bytes_b && pb < pa + bytes_a;
}

}  // namespace geoadv

using namespace geoadv;

extern "C" int geoadv_farthest_point_sample_plan(int n, int form, int *form_out, int *waves, int *points_per_thread) {
    fps_plan p;
    GA_REQUIRE(fps_choose(n, form, &p), "farthest_point_sample: no kernel for n=%d, form=%d: 1 <= n <= %d, form 0 (auto), 1 (workgroup per cloud) "
               "or 2 (wave per cloud, n <= %d)", n, form, FPS_MAX_N, FPS_WAVE_MAX_N);
    if (form_out) *form_out = p.form;
    if (waves) *waves = p.waves;
    if (points_per_thread) *points_per_thread = p.ppt;
    return GEOADV_OK;
}

extern "C" int geoadv_farthest_point_sample(int b, int n, const float *xyz, int m, const int *start, int form, int *idx, float *sampled,
                                            float *mindist, void *stream) {
    GA_REQUIRE(b >= 1 && n >= 1 && n <= FPS_MAX_N && m >= 1 && m <= n,
               "farthest_point_sample: bad dimensions (b=%d, n=%d, m=%d): b >= 1, 1 <= n <= %d, 1 <= m <= n", b, n, m, FPS_MAX_N);
    GA_REQUIRE(xyz && idx, "farthest_point_sample: null xyz or idx pointer");
    const size_t xyz_bytes = (size_t)b * n * 12;
    GA_REQUIRE(!sampled || !fps_overlap(sampled, (size_t)b * m * 12, xyz, xyz_bytes), "farthest_point_sample: sampled overlaps xyz");
    GA_REQUIRE(!mindist || !fps_overlap(mindist, (size_t)b * n * 4, xyz, xyz_bytes), "farthest_point_sample: mindist overlaps xyz");
    fps_plan p;
    GA_REQUIRE(fps_choose(n, form, &p), "farthest_point_sample: form %d is neither 0 (auto), 1 (workgroup per cloud) nor 2 (wave per cloud, "
               "n <= %d; got n=%d)", form, FPS_WAVE_MAX_N, n);
    const hipStream_t st = as_stream(stream);
#define FPS_CASE(F, NW, PPT, CPW) \
    if (p.form == F && p.waves == NW && p.ppt == PPT) fps_launch<NW, PPT, CPW>(b, n, xyz, m, start, idx, sampled, mindist, st)
    FPS_CASE(2, 1, 1, FPS_WAVE_CLOUDS);
    else FPS_CASE(2, 1, 4, FPS_WAVE_CLOUDS);
    else FPS_CASE(2, 1, 16, FPS_WAVE_CLOUDS);
    else FPS_CASE(1, 4, 1, 1);
    else FPS_CASE(1, 4, 4, 1);
    else FPS_CASE(1, 8, 4, 1);
    else FPS_CASE(1, 16, 4, 1);
    else FPS_CASE(1, 16, 8, 1);
    else FPS_CASE(1, 16, 16, 1);
    else GA_REQUIRE(false, "farthest_point_sample: no kernel instance for form %d, %d waves, %d points per thread", p.form, p.waves, p.ppt);
#undef FPS_CASE
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
