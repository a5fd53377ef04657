// Exact neighbour lists for nn_distance(P, Q) with a fixed Q and a slowly moving P (chamfer_lists.hip; DESIGN 4, "Neighbour lists").
// The Verlet list of molecular dynamics with an exactness certificate: at an ANCHOR the all-pairs scan has the exact minima; a
// compare-only pass then stores, for every row and every column, all partners closer than tau = (sqrt(minimum) + skin)^2.  While
// P has moved by less than the skin, a query only evaluates its list -- with the scan's own arithmetic and tie rule -- and
// certifies that no partner outside the list can reach the list's best; what it cannot certify it answers by brute force in the
// same launch.  The results are the scan's, bit for bit.
#pragma once
#include "common.h"
#include "chamfer_sym.h"

namespace geoadv {

constexpr int RL_CAP_MAX = 32;          // list entries per query at most (the capacity is a run-time value, 16 by default)
constexpr int RL_MAX_POINTS = 2048;     // rows / columns per cloud the lists are built for (entries are 16-bit)
constexpr int RL_THREADS = 256;         // one query per thread

struct ReconLists {
    int b, n, m, cap;
    float *anchor;                      // [b][n][3] P at the anchor
    float *tau_row, *tau_col;           // [b][n], [b][m] list thresholds (squared distances)
    int *need[2];                       // [8 b] each: clouds handed back to the scan until the next anchor; the query of call k reads
                                        // [k & 1] and writes [(k + 1) & 1] (the paired search's pattern, chamfer_grid.h)
    unsigned *cnt_row, *cnt_col;        // [b][n], [b][m] partners found below tau (0 or more than cap: the query is unlisted)
    unsigned short *list_row;           // [b][n][cap] column indices
    unsigned short *list_col;           // [b][m][cap] row indices
    float *dmax;                        // [b] largest displacement |P - anchor| the last query saw (0: no history)
    float *skin;                        // [b] the skin of the current lists
    unsigned long long *stats;          // [4] certified, listed but refused, unlisted queries; cloud-iterations handed back to the scan
    void *clear; size_t clear_bytes;    // need[0], need[1], cnt_row, cnt_col: zeroed before every build
};
// Carves the buffers above from `base` (null: measures only); own_anchor: with a copy of P (the loop; the operator reads the caller's)
size_t carve_recon_lists(ReconLists &L, void *base, int b, int n, int m, int cap, bool own_anchor);

struct ListBuild {
    const float *P, *Q;                 // [b][n][3] rows at the anchor, [b][m][3] columns
    const float *dist1;                 // [b][n] exact row minima, or ...
    const unsigned long long *row64;    // ... the scan's packed (distance, index) words (chamfer_sym.h)
    const float *dist2;                 // [b][m] exact column minima
    const float *skin;                  // [b] given, or null: factor * dmax clamped to [lo, hi], `first` without history
    float first, factor, lo, hi;
    unsigned long long *hint;           // host-visible [5] or null: stats[0..3] and a serial, stored by the build (no synchronisation)
    unsigned long long serial;
};
// zeroes the counters and flags, then builds the lists of every cloud (and copies P to L.anchor when it is not P itself)
int launch_recon_lists_build(const ReconLists &L, const ListBuild &in, hipStream_t st);

struct ListQuery {
    const float *P, *Q;                 // the moved rows, the columns
    float *dist1; int *idx1;            // [b][n] row minima, or ...
    unsigned long long *row64;          // ... one packed word per row (plain store)
    float *dist2; int *idx2;            // [b][m]
    int call;                           // calls since the build: selects the flag arrays
    bool answer_all;                    // the operator: flagged clouds are answered too (nothing else would)
};
int launch_recon_lists_query(const ReconLists &L, const ListQuery &q, hipStream_t st);

struct ListQueryArgs { ReconLists L; ListQuery q; const int *need_prev; int *need_next; };
// the query's workgroups as riders of the symmetric scan's launch (chamfer_sym.hip), the LAST blocks of its grid: on a list iteration
// the scan's own workgroups of that pair leave at once, and these run beside the paired search and the pool Jacobian
struct ListRider { ListQueryArgs a; int first_block, blocks, per_cloud; };
ListRider recon_lists_rider(const ReconLists &L, const ListQuery &q, int threads);

#ifdef __HIPCC__
// the scan's own arithmetic (chamfer_sym.hip: sqdist_s), every product and sum rounded on its own: the bits of a pair's distance
// do not depend on which kernel evaluates it, nor on which point is subtracted from which
__device__ __forceinline__ float rl_sqdist(float tx, float ty, float tz, float qx, float qy, float qz) {
    const float dx = tx - qx, dy = ty - qy, dz = tz - qz;
    const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz;
}
__device__ __forceinline__ float rl_sqrt(float v) { return __builtin_amdgcn_sqrtf(v); }   // v_sqrt_f32: 1 ulp, covered by the margin
// tau = (sqrt(minimum) + skin)^2.  Whatever its rounding: the list is DEFINED by the stored value (every pair with D < tau)
__device__ __forceinline__ float rl_tau(float dmin, float skin) {
    const float t = rl_sqrt(dmin) + skin;
    return t * t;
}
constexpr float RL_MARGIN = 0x1p-18f;       // relative to sqrt(tau): 64 units of fp32 round-off against the <= 17 the bound needs
constexpr float RL_TAU_MIN = 0x1p-80f;      // below: no certificate (the relative error model of the distances needs normal terms)


// grid = (row blocks + column blocks, clouds), one query per thread.  Certificate: a partner outside the list was at
// least sqrt(tau) away at the anchor; rows have moved by at most `move` since (a row query: its own displacement; a column query:
// the cloud's largest), so it is still sqrt(tau) - move away, and the list's best d* is the answer when
//     sqrt(d*) + move + margin < sqrt(tau).
// Every other query -- unlisted, refused, or poisoned by a NaN (all comparisons false) -- goes to a queue in LDS and is answered
// by a whole wave over all partners, same arithmetic, lowest index on equal bits.
// `blk`: the workgroup's index among its cloud's (row blocks first); lds: THREADS + 16 words.
template <int THREADS>
__device__ __forceinline__ void recon_lists_query_block(const ListQueryArgs &a, int blk, int c, unsigned *lds) {
    constexpr int RL_THREADS = THREADS;
    unsigned *red = lds, &qn = lds[8], &unl = lds[9];
    int *queue = reinterpret_cast<int *>(lds + 16);
    const ReconLists &L = a.L;
    const int n = L.n, m = L.m, cap = L.cap, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (!a.q.answer_all && sym_needed(a.need_prev, c)) {       // handed back earlier in this period: the scan answers this cloud
        if (t == 0) {
            a.need_next[8 * c + (blk & 7)] = 1;         // ... until the next anchor
            if (blk == 0) {
                atomicAdd(&L.stats[3], 1ull);
                L.dmax[c] = INFINITY;                       // it moved past its skin: the next build gives it the widest one
            }
        }
        return;
    }
    const int rblocks = (n + RL_THREADS - 1) / RL_THREADS;
    const bool is_row = blk < rblocks;
    const int N = is_row ? n : m, M = is_row ? m : n;          // queries of this side, partners
    const int q = (is_row ? blk : blk - rblocks) * RL_THREADS + t;
    const bool valid = q < N;
    const float *P = a.q.P + (size_t)c * n * 3, *Q = a.q.Q + (size_t)c * m * 3, *A = L.anchor + (size_t)c * n * 3;
    const float *own = is_row ? P : Q, *oth = is_row ? Q : P;
    if (t == 0) { qn = 0; unl = 0; }
    float move = 0.f;
    if (is_row) {
        if (valid) move = rl_sqrt(rl_sqdist(P[3 * q], P[3 * q + 1], P[3 * q + 2], A[3 * q], A[3 * q + 1], A[3 * q + 2]));
    } else {
        // squared displacements are >= +0 or NaN: as unsigned integers their order is the floats', with every NaN on top
        unsigned mx = 0;
        for (int j0 = t; j0 < n; j0 += 8 * RL_THREADS) {       // one round trip for eight rows per thread (rows past the end repeat the last)
            float v[8][6];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int j = min(j0 + u * RL_THREADS, n - 1);
#pragma unroll
                for (int e = 0; e < 3; ++e) { v[u][e] = P[3 * j + e]; v[u][3 + e] = A[3 * j + e]; }
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) mx = max(mx, __float_as_uint(rl_sqdist(v[u][0], v[u][1], v[u][2], v[u][3], v[u][4], v[u][5])));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off));
        if (lane == 0) red[wave] = mx;
    }
    __syncthreads();
    if (!is_row) {
        unsigned mx = red[0];
#pragma unroll
        for (int w = 1; w < RL_THREADS / 64; ++w) mx = max(mx, red[w]);
        move = rl_sqrt(__uint_as_float(mx));                   // (NaN stays NaN: nothing is certified)
        if (blk == rblocks && t == 0) L.dmax[c] = move;
    }
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (valid) { ox = own[3 * (size_t)q]; oy = own[3 * (size_t)q + 1]; oz = own[3 * (size_t)q + 2]; }
    if (valid) {
        const unsigned cnt = (is_row ? L.cnt_row : L.cnt_col)[(size_t)c * N + q];
        const float tau = (is_row ? L.tau_row : L.tau_col)[(size_t)c * N + q];
        const unsigned short *lst = (is_row ? L.list_row : L.list_col) + ((size_t)c * N + q) * cap;
        const bool listed = cnt >= 1u && cnt <= (unsigned)cap;
        float best = INFINITY;
        int bi = 0;
        if (listed) {
            bi = 0x7fffffff;
            // eight entries at a time, their indices and then their coordinates all in flight together: a thread's walk is a chain
            // of dependent loads, and one entry per round trip made the launch three times as long as the scan it replaces
            for (unsigned s0 = 0; s0 < cnt; s0 += 8) {
                int k[8];
                float x[8], y[8], z[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) k[u] = s0 + u < cnt ? min((int)lst[s0 + u], M - 1) : -1;
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const size_t o = 3 * (size_t)max(k[u], 0);
                    x[u] = oth[o]; y[u] = oth[o + 1]; z[u] = oth[o + 2];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float d = rl_sqdist(x[u], y[u], z[u], ox, oy, oz);
                    if (k[u] >= 0 && (d < best || (d == best && k[u] < bi))) { best = d; bi = k[u]; }
                }
            }
        }
        const float sd = rl_sqrt(best), st = rl_sqrt(tau);
        const bool ok = listed && bi != 0x7fffffff && tau >= RL_TAU_MIN && (sd + move) + RL_MARGIN * st < st;
        if (ok) {
            if (!is_row) { a.q.dist2[(size_t)c * m + q] = best; a.q.idx2[(size_t)c * m + q] = bi; }
            else if (a.q.row64) a.q.row64[(size_t)c * n + q] = sym_pack(best, bi);
            else { a.q.dist1[(size_t)c * n + q] = best; a.q.idx1[(size_t)c * n + q] = bi; }
        } else {
            queue[atomicAdd(&qn, 1u)] = q;
            if (!listed) atomicAdd(&unl, 1u);
        }
    }
    __syncthreads();
    const int nq = (int)qn;
    for (int e = wave; e < nq; e += RL_THREADS / 64) {         // (uniform per wave)
        const int qq = queue[e];
        const float qx = own[3 * (size_t)qq], qy = own[3 * (size_t)qq + 1], qz = own[3 * (size_t)qq + 2];
        float best = INFINITY;
        int bi = 0;
        for (int k0 = lane; k0 < M; k0 += 4 * 64) {            // ascending per lane: the first minimum kept is the lane's lowest index
            float x[4], y[4], z[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t o = 3 * (size_t)min(k0 + 64 * u, M - 1);
                x[u] = oth[o]; y[u] = oth[o + 1]; z[u] = oth[o + 2];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float d = rl_sqdist(x[u], y[u], z[u], qx, qy, qz);
                if (k0 + 64 * u < M && d < best) { best = d; bi = k0 + 64 * u; }
            }
        }
        wave_lexmin(best, bi);
        if (lane == 0) {
            if (!is_row) { a.q.dist2[(size_t)c * m + qq] = best; a.q.idx2[(size_t)c * m + qq] = bi; }
            else if (a.q.row64) a.q.row64[(size_t)c * n + qq] = sym_pack(best, bi);
            else { a.q.dist1[(size_t)c * n + qq] = best; a.q.idx1[(size_t)c * n + qq] = bi; }
        }
    }
    if (t == 0) {
        const int mine = min(RL_THREADS, N - (q - t));
        if (mine > nq) atomicAdd(&L.stats[0], (unsigned long long)(mine - nq));
        if (nq > (int)unl) atomicAdd(&L.stats[1], (unsigned long long)(nq - (int)unl));
        if (unl) atomicAdd(&L.stats[2], (unsigned long long)unl);
        if (nq > THREADS / 4) a.need_next[8 * c + (blk & 7)] = 1;      // too stale to pay: the scan takes the cloud over
    }
}


template <int THREADS>
__device__ __forceinline__ bool list_rider_block(const ListRider &r, unsigned *lds) {
    if (r.blocks == 0 || (int)blockIdx.x < r.first_block) return false;
    const int lin = (int)blockIdx.x - r.first_block;
    recon_lists_query_block<THREADS>(r.a, lin % r.per_cloud, lin / r.per_cloud, lds);
    return true;
}
#endif

}  // namespace geoadv
