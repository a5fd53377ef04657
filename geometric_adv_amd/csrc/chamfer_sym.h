// Interface of the symmetric Chamfer scan (chamfer_sym.hip) shared with its callers (attack.hip, train.hip).
#pragma once
#include "common.h"

namespace geoadv {

struct ChamferPair {
    const float *p, *q;        // [b][n][3] rows, [b][m][3] columns
    float *dist1; int *idx1;   // [b][n]  row minima  (nn_distance outputs 0,1)
    float *dist2; int *idx2;   // [b][m]  column minima (outputs 2,3)
};

// How the row minima leave a planned launch of the scan -- a read-only view for whoever reads them next (SymPlan::rows):
// FINAL / MERGE_LAUNCH: dist1 / idx1 are final in the pairs' own arrays (one slice, or the merge launch ran): deferred == false.
// PARTIALS: one (distance, index) partial per column slice -- [pair][cloud][slice][n] -- whose lexicographic minimum is dist1 / idx1.
// PACKED (8 or more partials per row -- a merge launch or a heavy consumer, 8 loads per row at the least -- i.e. batches up to
// 63 clouds of 2048 points): the scan folds every (row, slice) into ONE packed word per row -- (distance bits << 32) | index, 64-bit unsigned atomic
// minimum: squared distances are >= +0, so the order of the words is the lexicographic order of (distance, index) -- in
// row64[pair][cloud][n], which must hold all ones when the scan starts (the loop's FC2 launch fills it on its way); slices == 0.
constexpr int SYM_PACK_FROM = 8;
// (Kernel arguments carry this view: `clouds` and the trailing slot keep the arguments' offsets where they were before the launch was
// planned on the host -- with the view shrunk to what is read, the loop measured 0.25 us per iteration slower, profiles/r11_sym_plan_ab.txt.)
struct SymRows { const float *rowpart_d; const int *rowpart_i; int slices, clouds; bool deferred; const unsigned long long *row64; int unused_ = 0; };

// What a caller asks of one launch of the scan.  Plain values only: chamfer_sym_plan() reads nothing else.
struct SymRequest {
    int np, b, n, m;                 // 1 or 2 problems of b clouds, n rows x m columns each
    bool loop = false;               // the attack loop's launch rule (riders may share the launch)
    bool need1 = false;              // the second pair is gated by per-cloud flags: it usually has no work and does not count as live
    bool search = false, jac = false, loss = false;   // riders asked for: the paired grid search, the pool Jacobian, the loss + gradient workgroups
    int loss_rows = 0;               // ... workgroups per cloud of the loss riders
    bool loss_force = false;         // ... hosted wherever the launch CAN (the parity tests; the default hosts them where it pays)
    bool defer = false;              // the caller's next launch takes the row minima as partials
    bool packed = false;             // ... and has a packed buffer (SymRows::row64)
    int pack_from = SYM_PACK_FROM;   // the fewest partials per row that are folded into the packed words
    int q_clouds = 0, pair_base = 0; // q_clouds > 0: cloud c is the pair (P cloud (pair_base + c) / q_clouds, Q cloud (pair_base + c) % q_clouds)
    bool screen = true;              // the process-wide screen switch (chamfer_sym_screen_on), read ONCE by whoever builds the request
};
// Launch shape of the symmetric scan: how the 8 waves of a workgroup are laid over rows and columns, and how many
// columns a workgroup takes so that the grid fills the chip (the plain kernel: 256 / 128 / 64 per stage; the screened one: always 256;
// `groups` = live (pair, cloud) groups).
struct SymShape { int rw, cw, rtiles, C, S, cslices; bool mx; };
struct SymBlocks { int first, count; };
// Every decision of one launch, made once by chamfer_sym_plan() -- a pure host function: no device, no global -- read by the
// caller (the loop's forward prepares its other launches from it) and executed by launch_chamfer_sym().
struct SymPlan {
    SymRequest req;
    SymShape shape;
    int kernel;                      // 0: the plain kernel; 8: the screened one (8 column tiles = 256 columns per stage, its only form)
    int rslices;                     // row partials per row (column slices x column waves)
    int rows;                        // how the row minima leave the launch: GEOADV_PLAN_ROWS_* (include/geoadv.h)
    SymBlocks search, scan, jac, loss;   // block ranges in grid order (count 0: absent); grid = their sum
    unsigned grid;
    size_t lds_bytes;                // dynamic LDS of the launch
    unsigned loss_arrivals;          // what every cloud's arrival counter gains in this launch (0 unless the loss riders are hosted)
    int raise_prio;                  // JacRider::raise_prio
    size_t group_floats;             // scratch floats per (pair, cloud) group
    size_t part_off[4];              // offsets in the workspace, in floats: row distances, row indices, column distances, column indices
};
SymPlan chamfer_sym_plan(const SymRequest &r);
bool chamfer_sym_screen_on();
SymRows chamfer_sym_rows(const SymPlan &p, const float *workspace, const unsigned long long *row64);

#ifdef __HIPCC__
__device__ __forceinline__ bool sym_needed(const int *need, int c) {
    if (!need) return true;
    const int4 lo = reinterpret_cast<const int4 *>(need)[2 * c], hi = reinterpret_cast<const int4 *>(need)[2 * c + 1];
    return (lo.x | lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) != 0;
}

// Lexicographic (distance, index) minimum over `slices` partials `stride` elements apart.  The slices are column ranges in
// ascending order, so the lowest slice attaining the minimal distance holds the lowest index: only the DISTANCES are compared
// (eight loads in flight per step) and the winner's index is one further load.
__device__ __forceinline__ float sym_merge_pick(const float *d, int slices, size_t stride, int &slice) {
    float bd = d[0];
    int bs = 0;
    for (int s0 = 1; s0 < slices; s0 += 8) {
        float vd[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) vd[u] = d[(size_t)(s0 + u < slices ? s0 + u : 0) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s0 + u < slices && vd[u] < bd) { bd = vd[u]; bs = s0 + u; }
    }
    slice = bs;
    return bd;
}
__device__ __forceinline__ void sym_merge_slices(const float *d, const int *i, int slices, size_t stride, float &od, int &oi) {
    int s;
    od = sym_merge_pick(d, slices, stride, s);
    oi = i[(size_t)s * stride];
}
__device__ __forceinline__ unsigned long long sym_pack(float d, int i) {
    return ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)i;
}
// the distance alone
__device__ __forceinline__ float sym_merge_min(const float *d, int slices, size_t stride) {
    float bd = d[0];
    for (int s0 = 1; s0 < slices; s0 += 8) {
        float vd[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) vd[u] = d[(size_t)(s0 + u < slices ? s0 + u : 0) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) bd = fminf(bd, vd[u]);
    }
    return bd;
}
#endif

// Chamfer gradient w.r.t. the FIRST cloud of a problem (attack.hip: chamfer_grad_attack_*_kernel; shared with train.hip)
struct CGradProblem {
    const float *p, *q;          // [B][n][3] own / other cloud
    const int *idx1, *idx2;      // [B][n] own->other matches, other->own matches
    float *g;                    // [B][n][3]
    const float *w;              // [B] or null: upstream factor (dist_weight)
    const int *jstar;            // [B] or null: point receiving the extra max-term
    float extra_w;               // max_point_dist_weight (0 = none)
    // idx1 still as the symmetric scan's (distance, index) partials per column slice (null: idx1 is final); this kernel then
    // takes their lexicographic minimum on its way in and leaves it in idx1_out.  part_need: only the clouds flagged there.
    const float *part_d; const int *part_i; int part_slices; const int *part_need; int *idx1_out;
    const unsigned long long *part_w;      // ... or as packed (distance, index) words [B][n] (SymRows::row64): the index is the low half
};
int launch_chamfer_grad(const CGradProblem *pr, int np, int B, int n, hipStream_t st);

// One direction of the two-scan kernel (chamfer.hip): up to four scans share a launch
struct ChamferScan {
    const float *query;   // [b, nq, 3]
    const float *target;  // [b, nt, 3]
    float *dist;          // [b, nq]
    int *idx;             // [b, nq]
    int nq, nt;
    const int *need;      // null = every cloud; else int[8 * b] (16-byte aligned): cloud c is scanned only if one of its 8
                          // flags is set (a workgroup of the paired grid search, chamfer_grid.hip, gave up on it)
};
int launch_chamfer_scans(const ChamferScan *scans, int nscan, int b, hipStream_t stream);

// the reference's rule for a NaN distance to candidate 0, applied to finished nn_distance outputs (chamfer.hip)
int launch_nn_nonfinite_fix(int b, int n, const float *xyz1, int m, const float *xyz2, float *dist1, int *idx1, float *dist2,
                            int *idx2, hipStream_t stream);

size_t chamfer_sym_workspace_floats(int pairs, int b, int n, int m);
struct GridArgs;
struct JacRider;
struct LossRider;
struct ListRider;
// Executes a plan.  need1: per-cloud flags (int[8 * b], 16-byte aligned) restricting the SECOND pair to the clouds that still need the
// all-pairs kernel; rider / jac / loss: the riders the plan has block ranges for (their first_block / blocks / clouds / raise_prio
// come from the plan; loss->target already counts plan.loss_arrivals); row64: the packed buffer when plan.rows is PACKED.
// need0: the same kind of flags for the FIRST pair (the loop's neighbour lists answer the other clouds, chamfer_lists.h); null = every cloud.
int launch_chamfer_sym(const SymPlan &p, const ChamferPair *pairs, float *workspace, const int *need1, const GridArgs *rider,
                       const JacRider *jac, const LossRider *loss, unsigned long long *row64, hipStream_t stream, const int *need0 = nullptr,
                       const ListRider *lists = nullptr);      // lists: the list queries as further workgroups of the launch (plain kernel, no hosted loss riders)
// the operator form: every cloud live, no rider, rows final on return
int launch_chamfer_sym(const ChamferPair *pairs, int np, int b, int n, int m, float *workspace, hipStream_t stream);

}  // namespace geoadv
