// Exact neighbour lists for nn_distance(P, Q) of a fixed Q and a slowly moving P: the build pass, the query kernel and the
// operator entry point (chamfer_lists.h has the idea; DESIGN 4 "Neighbour lists" the certificate and its margin).
#include "chamfer_lists.h"
#include "chamfer_sym.h"
#include <math.h>

#pragma clang fp contract(off)

namespace geoadv {

struct ListBuildArgs { ReconLists L; ListBuild in; int cslices, span; };

// grid = (row tiles of 256 x column slices, clouds).  A thread owns one row and walks the slice's columns out of LDS: ONE
// evaluation per pair serves the row's list (D < tau_row) and the column's (D < tau_col), as in the symmetric scan.  Entries are
// appended through counters; their order inside a list is not defined and does not matter (the query takes a lexicographic
// minimum), the counter's final value -- listed or overflowed -- is.
__global__ __launch_bounds__(RL_THREADS) void recon_lists_build_kernel(ListBuildArgs a) {
    __shared__ float4 sq[RL_THREADS];
    const ReconLists &L = a.L;
    const int c = blockIdx.y, n = L.n, m = L.m, cap = L.cap, t = threadIdx.x, lane = t & 63;
    const int rt = blockIdx.x / a.cslices, cs = blockIdx.x % a.cslices;
    const float *P = a.in.P + (size_t)c * n * 3, *Q = a.in.Q + (size_t)c * m * 3;
    float skin;
    if (a.in.skin) skin = a.in.skin[c];
    else {
        const float seen = L.dmax[c];
        skin = seen > 0.f ? fminf(fmaxf(a.in.factor * seen, a.in.lo), a.in.hi) : a.in.first;     // (a NaN history: `first`; a cloud handed back: hi)
    }
    unsigned *crow = L.cnt_row + (size_t)c * n, *ccol = L.cnt_col + (size_t)c * m;
    const int i = rt * RL_THREADS + t;
    const bool rv = i < n;
    float px = 0.f, py = 0.f, pz = 0.f, ti = -1.f;
    if (rv) {
        px = P[3 * i]; py = P[3 * i + 1]; pz = P[3 * i + 2];
        const float d1 = a.in.row64 ? __uint_as_float((unsigned)(a.in.row64[(size_t)c * n + i] >> 32)) : a.in.dist1[(size_t)c * n + i];
        ti = rl_tau(d1, skin);
        if (cs == 0) {
            L.tau_row[(size_t)c * n + i] = ti;
            if (L.anchor != a.in.P) {
                float *A = L.anchor + ((size_t)c * n + i) * 3;
                A[0] = px; A[1] = py; A[2] = pz;
            }
        }
    }
    if (blockIdx.x == 0 && t == 0) {
        L.skin[c] = skin;
        if (a.in.hint && c == 0) {       // what the queries since the last build counted, for a host that reads it without waiting
            for (int k = 0; k < 4; ++k) a.in.hint[k] = L.stats[k];
            __threadfence_system();
            a.in.hint[4] = a.in.serial;
        }
    }
    unsigned short *lrow = L.list_row + (size_t)c * cap * n, *lcol = L.list_col + (size_t)c * cap * m;
    const int k0 = cs * a.span, k1 = min(m, k0 + a.span);
    for (int kb = k0; kb < k1; kb += RL_THREADS) {
        __syncthreads();
        {
            const int k = kb + t;
            float4 v = make_float4(INFINITY, INFINITY, INFINITY, -1.f);          // padding: never below any threshold
            if (k < k1) {
                v.x = Q[3 * (size_t)k]; v.y = Q[3 * (size_t)k + 1]; v.z = Q[3 * (size_t)k + 2];
                v.w = rl_tau(a.in.dist2[(size_t)c * m + k], skin);
                if (rt == 0) L.tau_col[(size_t)c * m + k] = v.w;
                // a column whose list has overflowed already (another workgroup's rows: a far column sees a whole dense cloud
                // inside its skin) stays unlisted whatever is added: it leaves the comparison, its counter stays beyond cap
                if (__hip_atomic_load(&ccol[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned)cap) v.w = -1.f;
            }
            sq[t] = v;
        }
        __syncthreads();
        const int cnt = min(RL_THREADS, k1 - kb), cnt4 = (cnt + 3) & ~3;
        for (int u = 0; u < cnt4; u += 4) {
            float4 q[4];
            float d[4];
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                q[j] = sq[u + j];
                d[j] = rl_sqdist(q[j].x, q[j].y, q[j].z, px, py, pz);
                any = any | (d[j] < ti) | (rv & (d[j] < q[j].w));
            }
            if (!__any(any)) continue;                                           // (uniform) almost every group of four
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = kb + u + j;
                if (d[j] < ti) {
                    const unsigned slot = atomicAdd(&crow[i], 1u);
                    if (slot < (unsigned)cap) lrow[(size_t)i * cap + slot] = (unsigned short)k;
                }
                const bool hc = rv && d[j] < q[j].w;
                const unsigned long long mk = __ballot(hc);                     // one counter update per wave and column
                if (mk) {
                    const int leader = __ffsll((long long)mk) - 1;
                    unsigned base = 0;
                    if (lane == leader) {
                        base = atomicAdd(&ccol[k], (unsigned)__popcll(mk));
                        if (base + (unsigned)__popcll(mk) > (unsigned)cap) sq[u + j].w = -1.f;      // overflowed: see above (a late reader of the old value only counts on)
                    }
                    base = (unsigned)__shfl((int)base, leader);
                    if (hc) {
                        const unsigned slot = base + (unsigned)__popcll(mk & ((1ull << lane) - 1ull));
                        if (slot < (unsigned)cap) lcol[(size_t)k * cap + slot] = (unsigned short)i;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(RL_THREADS) void recon_lists_query_kernel(ListQueryArgs a) {
    __shared__ unsigned lds[RL_THREADS + 16];
    recon_lists_query_block<RL_THREADS>(a, blockIdx.x, blockIdx.y, lds);
}

// the operator's read-out: out[0..3] = the counters, flags[c] = cloud c raised its flag
__global__ void recon_lists_state_kernel(ReconLists L, const int *need, unsigned long long *out, int *flags) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < 4) out[c] = L.stats[c];
    if (c < L.b) flags[c] = sym_needed(need, c) ? 1 : 0;
}

size_t carve_recon_lists(ReconLists &L, void *base, int b, int n, int m, int cap, bool own_anchor) {
    Carver cv(base);
    const size_t B = (size_t)b;
    L.b = b; L.n = n; L.m = m; L.cap = cap;
    L.anchor = own_anchor ? cv.take<float>(B * n * 3) : nullptr;
    L.tau_row = cv.take<float>(B * n); L.tau_col = cv.take<float>(B * m);
    char *clr = cv.take<char>(sizeof(int) * (16 * B + B * n + B * m));          // one block: one clear per build
    L.clear = clr; L.clear_bytes = sizeof(int) * (16 * B + B * n + B * m);
    L.need[0] = reinterpret_cast<int *>(clr); L.need[1] = L.need[0] + 8 * B;     // (32 bytes per cloud: 16-byte aligned)
    L.cnt_row = reinterpret_cast<unsigned *>(L.need[1] + 8 * B); L.cnt_col = L.cnt_row + B * n;
    L.list_row = cv.take<unsigned short>(B * cap * n); L.list_col = cv.take<unsigned short>(B * cap * m);
    L.dmax = cv.take<float>(B); L.skin = cv.take<float>(B);
    L.stats = cv.take<unsigned long long>(4);
    return cv.bytes();
}

int launch_recon_lists_build(const ReconLists &L, const ListBuild &in, hipStream_t st) {
    GA_HIP(hipMemsetAsync(L.clear, 0, L.clear_bytes, st));
    ListBuildArgs a;
    a.L = L; a.in = in;
    if (!a.L.anchor) a.L.anchor = const_cast<float *>(in.P);
    // column slices: enough workgroups for four per CU, whole stages of 256 columns each
    const int rtiles = cdiv(L.n, RL_THREADS), stages = cdiv(L.m, RL_THREADS);
    int cslices = 1;
    while (cslices < stages && (long)rtiles * cslices * L.b < 4L * kCUs) cslices *= 2;
    cslices = std::min(cslices, stages);
    a.span = cdiv(stages, cslices) * RL_THREADS;
    a.cslices = cdiv(L.m, a.span);
    recon_lists_build_kernel<<<dim3(rtiles * a.cslices, L.b), RL_THREADS, 0, st>>>(a);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

ListRider recon_lists_rider(const ReconLists &L, const ListQuery &q, int threads) {
    ListRider r;
    r.a.L = L; r.a.q = q;
    r.a.need_prev = L.need[q.call & 1]; r.a.need_next = L.need[(q.call + 1) & 1];
    r.per_cloud = cdiv(L.n, threads) + cdiv(L.m, threads);
    r.first_block = 0; r.blocks = r.per_cloud * L.b;
    return r;
}

int launch_recon_lists_query(const ReconLists &L, const ListQuery &q, hipStream_t st) {
    const ListQueryArgs a = recon_lists_rider(L, q, RL_THREADS).a;
    recon_lists_query_kernel<<<dim3(cdiv(L.n, RL_THREADS) + cdiv(L.m, RL_THREADS), L.b), RL_THREADS, 0, st>>>(a);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}

}  // namespace geoadv

using namespace geoadv;

extern "C" size_t geoadv_nn_distance_lists_workspace_bytes(int b, int n, int m, int capacity) {
    if (b <= 0 || n <= 0 || m <= 0 || capacity <= 0) return 256;
    ReconLists L;
    return carve_recon_lists(L, nullptr, b, n, m, capacity, false) + 256;
}

extern "C" int geoadv_nn_distance_lists(int b, int n, int m, const float *xyz1_anchor, const float *xyz2, const float *dist1_anchor,
                                        const float *dist2_anchor, const float *skin, int capacity, const float *xyz1, float *dist1,
                                        int *idx1, float *dist2, int *idx2, unsigned long long *state, int *flags, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    GA_REQUIRE(b >= 0 && n >= 1 && m >= 1 && n <= RL_MAX_POINTS && m <= RL_MAX_POINTS,
               "nn_distance_lists: bad dimensions (b=%d n=%d m=%d; clouds of at most %d points)", b, n, m, RL_MAX_POINTS);
    GA_REQUIRE(capacity >= 1 && capacity <= RL_CAP_MAX, "nn_distance_lists: capacity=%d must be in [1, %d]", capacity, RL_CAP_MAX);
    if (b == 0) return GEOADV_OK;
    GA_REQUIRE(b <= 65535, "nn_distance_lists: at most 65535 clouds (got %d)", b);
    GA_REQUIRE(xyz1_anchor && xyz2 && dist1_anchor && dist2_anchor && skin && xyz1 && dist1 && idx1 && dist2 && idx2 && state && flags && workspace,
               "nn_distance_lists: null pointer");
    GA_REQUIRE(workspace_bytes >= geoadv_nn_distance_lists_workspace_bytes(b, n, m, capacity),
               "nn_distance_lists: workspace too small (%zu bytes, need %zu)", workspace_bytes,
               geoadv_nn_distance_lists_workspace_bytes(b, n, m, capacity));
    hipStream_t st = as_stream(stream);
    ReconLists L;
    carve_recon_lists(L, workspace, b, n, m, capacity, false);
    GA_HIP(hipMemsetAsync(L.stats, 0, sizeof(unsigned long long) * 4, st));
    ListBuild in{};
    in.P = xyz1_anchor; in.Q = xyz2; in.dist1 = dist1_anchor; in.dist2 = dist2_anchor; in.skin = skin;
    if (int rc = launch_recon_lists_build(L, in, st)) return rc;
    L.anchor = const_cast<float *>(xyz1_anchor);
    ListQuery q{};
    q.P = xyz1; q.Q = xyz2; q.dist1 = dist1; q.idx1 = idx1; q.dist2 = dist2; q.idx2 = idx2; q.call = 0; q.answer_all = true;
    if (int rc = launch_recon_lists_query(L, q, st)) return rc;
    recon_lists_state_kernel<<<cdiv(std::max(b, 4), 256), 256, 0, st>>>(L, L.need[1], state, flags);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
