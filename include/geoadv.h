/*
 * geoadv.h -- C ABI of libgeoadv.so, the MI355X (gfx950) implementation of the geometric
 * adversarial attack hot path of itailang/geometric_adv.
 *
 * This header is the drop-in boundary.  Every entry point below replaces one native launcher
 * (or one session-level Python method) of the reference; the reference file:line is cited at
 * each declaration.  Conventions, all entry points:
 *   - plain C linkage, plain pointers and ints; no torch / TF types,
 *   - every data pointer is a DEVICE pointer (HBM) unless the parameter name starts with host_,
 *   - row-major contiguous fp32 / int32 tensors in the reference's layouts,
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); calls only ENQUEUE
 *     work (no allocation, no host synchronisation) unless stated otherwise, so they are
 *     capturable into a hipGraph,
 *   - return value: 0 on success, non-zero on error; geoadv_last_error() gives the message
 *     (thread-local).  Shape violations that the reference reports through OP_REQUIRES /
 *     errors::InvalidArgument (tf_nndistance.cpp:51-58, tf_grouping.cpp:70-74) return
 *     GEOADV_EINVAL here,
 *   - the caller owns every buffer; the library owns only what lives behind the opaque
 *     geoadv_ae / geoadv_attack handles.
 */
#ifndef GEOADV_H
#define GEOADV_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GEOADV_OK      0
#define GEOADV_EINVAL  1   /* bad shape / argument                      */
#define GEOADV_EHIP    2   /* a HIP runtime call or kernel launch failed */
#define GEOADV_ENOMEM  3
#define GEOADV_ERANGE  4   /* a value left the range an arithmetic was set up for (geoadv_ae_status) */

int         geoadv_version(void);                /* 1000*major + minor */
const char *geoadv_last_error(void);

/* ------------------------------------------------------------------------------------------
 * Structural losses: external/structural_losses
 * ---------------------------------------------------------------------------------------- */

/* NmDistanceKernelLauncher(b,n,xyz,m,xyz2,result,result_i,result2,result2_i)
 * (tf_nndistance.cpp:168, kernel tf_nndistance_g.cu:5-131).  dist1[b,n], idx1[b,n] = squared
 * distance / index of the nearest xyz2 point for every xyz1 point; dist2/idx2 the converse.
 * Results are bit-identical to the reference CPU op (tf_nndistance.cpp:21-43): unfused fp32
 * arithmetic, lowest index on ties.  n == 0 or m == 0 is accepted (m == 0 gives dist 0 / idx 0,
 * like the CPU loop).  Non-finite coordinates follow the CPU loop too (`k==0 || d<best`, :33): a
 * query whose distance to candidate 0 is NaN returns (NaN, 0), a NaN distance to a later
 * candidate never wins, an infinite minimum returns its lowest index (the payload of a returned
 * NaN is not specified): a cloud pair with a non-finite coordinate is recomputed by that loop, a
 * thread per query, in a closing launch of the operator.  The same holds for geoadv_nn_distance_sym
 * and geoadv_nn_distance_paired (tests/golden/nn_distance_nonfinite.npz). */
int geoadv_nn_distance(int b, int n, const float *xyz1, int m, const float *xyz2,
                       float *dist1, int *idx1, float *dist2, int *idx2, void *stream);

/* The same outputs, bit for bit, from ONE evaluation of every pair distance for both directions (the attack loop's kernel,
 * csrc/chamfer_sym.hip: the distance matrix is symmetric in the two clouds' roles down to the last bit).  n, m >= 1.  workspace:
 * geoadv_nn_distance_sym_workspace_floats(b,n,m) floats of caller-owned scratch (row minima per column slice; the caller
 * allocates, as with the temp tensor of tf_approxmatch.cpp:164-170). */
size_t geoadv_nn_distance_sym_workspace_floats(int b, int n, int m);
/* 1 if this shape is answered by the matrix-pipe-screened form of the scan (csrc/chamfer_mx.h: approximate distances from one fp16
 * MFMA per 32 x 32 pairs select, with a rigorous error bound, the few pairs that are then evaluated with the reference's
 * arithmetic -- same bits out), 0 if by the unscreened scan.  geoadv_set_chamfer_screen(0) turns the screened kernel off for the
 * whole process (operators, scorer, attack and training loops; returns the previous setting): the tests' second opinion. */
int geoadv_nn_distance_sym_is_screened(int b, int n, int m);
int geoadv_set_chamfer_screen(int on);
int geoadv_nn_distance_sym(int b, int n, const float *xyz1, int m, const float *xyz2,
                           float *dist1, int *idx1, float *dist2, int *idx2,
                           float *workspace, size_t workspace_floats, void *stream);

/* nn_distance(xyz1, xyz2) from exact neighbour lists (csrc/chamfer_lists.hip; the attack loop answers nn_distance(recon, target)
 * this way between two all-pairs scans): xyz2 is fixed and xyz1 has moved a little since an ANCHOR at which the exact minima are
 * known.  The call builds, for every row and every column, the list of partners whose ANCHOR distance D(xyz1_anchor, xyz2) is below
 * tau = (sqrt(minimum) + skin[cloud])^2 -- at most `capacity` (1 ... 32) entries; a query with more is unlisted -- and then answers
 * every query for the moved xyz1: from its list where the certificate holds (no partner outside the list can reach the list's
 * best: sqrt(best) + displacement + margin < sqrt(tau), the displacement being the row's own for a row query and the cloud's
 * largest for a column query), by brute force over all partners otherwise.  Either way the four outputs are those of
 * geoadv_nn_distance(xyz1, xyz2) bit for bit for finite inputs, ties to the lowest index.  dist1_anchor / dist2_anchor [b,n] / [b,m]
 * must be the exact minima of nn_distance(xyz1_anchor, xyz2); n, m <= 2048.  state (device, 4 words): queries certified, listed but
 * refused, unlisted; 0.  flags (device, [b]): 1 for a cloud in which a workgroup refused more than a quarter of its 256 queries
 * (the loop hands such a cloud back to the scan until its next anchor).  Non-finite coordinates: every query they touch is
 * refused and answered by brute force with an in-range index.  workspace: geoadv_nn_distance_lists_workspace_bytes bytes. */
size_t geoadv_nn_distance_lists_workspace_bytes(int b, int n, int m, int capacity);
int geoadv_nn_distance_lists(int b, int n, int m, const float *xyz1_anchor, const float *xyz2, const float *dist1_anchor,
                             const float *dist2_anchor, const float *skin, int capacity, const float *xyz1, float *dist1,
                             int *idx1, float *dist2, int *idx2, unsigned long long *state, int *flags, void *workspace,
                             size_t workspace_bytes, void *stream);

/* chamfer_dist[b] = reduce_mean(dist1[b,:]) + reduce_mean(dist2[b,:]) -- the scalar every caller of nn_distance forms next
 * (adv_ae.py:121,132; get_dists_per_point.py:75; prepare_indices_for_attack.py:114) -- in the summation order of the
 * attack loop's own metrics, so that a Chamfer distance recomputed from saved clouds equals adversarial_metrics[:,:,2]
 * bit for bit (the np.array_equal sanity check of get_dists_per_point.py:114-115). */
int geoadv_chamfer_per_pc(int b, int n, int m, const float *dist1, const float *dist2, float *out, void *stream);

/* Same results as geoadv_nn_distance for n == m <= 8192, from an exact grid search that uses xyz2[j] as the first guess
 * for the neighbour of xyz1[j] (and vice versa): fast when the clouds are paired like the attack's (adv, x), never wrong
 * otherwise (a query whose guess is poor is scanned against all points). */
int geoadv_nn_distance_paired(int b, int n, const float *xyz1, const float *xyz2,
                              float *dist1, int *idx1, float *dist2, int *idx2, void *stream);

/* NmDistanceGradKernelLauncher(b,n,xyz1,m,xyz2,grad_dist1,idx1,grad_dist2,idx2,grad_xyz1,grad_xyz2)
 * (tf_nndistance.cpp:208, kernel tf_nndistance_g.cu:132-157).  Outputs are fully overwritten
 * (the reference memsets them).  Unlike the reference GPU kernel (float atomicAdd) the
 * accumulation order is the CPU op's (tf_nndistance.cpp:126-163), so results are deterministic
 * and bit-identical to it.  Requires n, m <= 32768. */
int geoadv_nn_distance_grad(int b, int n, const float *xyz1, int m, const float *xyz2,
                            const float *grad_dist1, const int *idx1,
                            const float *grad_dist2, const int *idx2,
                            float *grad_xyz1, float *grad_xyz2, void *stream);

/* Bulk Chamfer scorer: the graph of attacker/prepare_indices_for_attack.py:110-114 evaluated for
 * EVERY pair of clouds, out[i*nb + j] = mean_p dist1 + mean_q dist2 of nn_distance(A[i], B[j]), without the
 * np.tile'd (na, nb, n, 3) copies the script feeds in 10 x 10 batches (:121-139).  A (na,n,3), B (nb,m,3).
 * workspace: geoadv_chamfer_matrix_workspace_floats(na,nb,n,m) floats (any larger or smaller size >= one pair's
 * worth works: pairs are processed in chunks that fit). */
size_t geoadv_chamfer_matrix_workspace_floats(int na, int nb, int n, int m);
int geoadv_chamfer_matrix(int na, int nb, int n, int m, const float *A, const float *B, float *out,
                          float *workspace, size_t workspace_floats, void *stream);

/* approxmatchLauncher(b,n,m,xyz1,xyz2,match,temp) (tf_approxmatch.cpp:141, kernel
 * tf_approxmatch_g.cu:1-181).  match is (b,m,n) like the reference GPU op: match[b,l,k] couples
 * xyz2 point l with xyz1 point k.  temp: scratch of geoadv_approx_match_temp_floats(b,n,m) floats
 * (the reference allocates b*(n+m)*2, tf_approxmatch.cpp:168).  The level schedule is the CPU
 * op's (11 levels, tf_approxmatch.cpp:31). */
size_t geoadv_approx_match_temp_floats(int b, int n, int m);
int geoadv_approx_match(int b, int n, int m, const float *xyz1, const float *xyz2,
                        float *match, float *temp, void *stream);
/* How the pair weight expf(level * |p - q|^2) (tf_approxmatch.cpp:46) is evaluated; the rest of the algorithm (fp64
 * capacities, factors and sums) is the same in both modes (csrc/emd.hip header):
 *   FAST       fp32 distance, v_exp_f32.  Plan entries typically within 1e-6 relative of the CPU op; on clouds of
 *              thousands of points a few entries per million reach ~1e-4 (the algorithm amplifies the weight rounding).
 *   REFERENCE  the CPU op's own weights bit for bit (double distance, float expf argument, glibc's expf algorithm in fp64)
 *              and double level terms: every entry within ~2 float ulps of the CPU op; ~3.7x the time.
 * geoadv_approx_match / geoadv_emd_cost_grad1 are the FAST mode. */
#define GEOADV_EMD_FAST 0
#define GEOADV_EMD_REFERENCE 1
/* OR-ed into a `mode` argument (and into geoadv_attack_config.emd_weight_mode): every sweep of THIS call in its dense form -- the
 * first three levels' sweeps (level = -4^8, -4^7, -4^6: weights exactly 0 beyond 0.04 / 0.08 / 0.16) otherwise walk a cell grid
 * instead of every pair (csrc/emd.hip, "Sparse levels").  The results differ only in the order of fp64 additions. */
#define GEOADV_EMD_DENSE_LEVELS 0x100
int geoadv_approx_match_mode(int mode, int b, int n, int m, const float *xyz1, const float *xyz2,
                             float *match, float *temp, void *stream);
/* TEST / MEASUREMENT ONLY: the process default of calls whose mode carries no GEOADV_EMD_DENSE_LEVELS flag (on != 0, the default:
 * sparse first levels; 0: every sweep dense).  An atomic word read at launch time -- a process that wants one behaviour for one
 * call or handle passes the flag instead; this setter is not meant to be flipped while other threads launch. */
int geoadv_emd_sparse_levels(int on);
/* matchcostLauncher (tf_approxmatch.cpp:142; tf_approxmatch_g.cu:183-227): out[b].  The reference's launcher has no scratch
 * argument: this form takes stream-ordered scratch of its own (hipMallocAsync on `stream`); geoadv_match_cost_ws is the same op on
 * caller-owned scratch of geoadv_match_cost_workspace_floats(b,n,m) floats. */
int geoadv_match_cost(int b, int n, int m, const float *xyz1, const float *xyz2,
                      const float *match, float *out, void *stream);
size_t geoadv_match_cost_workspace_floats(int b, int n, int m);
int geoadv_match_cost_ws(int b, int n, int m, const float *xyz1, const float *xyz2, const float *match, float *out,
                         float *workspace, size_t workspace_floats, void *stream);
/* match_cost and match_cost_grad w.r.t. xyz1 of the plan approx_match(xyz1, xyz2) WITHOUT materialising the plan: what a
 * caller that treats the plan as a constant (ApproxMatch is NoGradient, tf_approxmatch.py:19) and differentiates w.r.t.
 * xyz1 only needs -- the attack loop's Chamfer+EMD loss.  cost[b], grad1[b,n,3]; temp: scratch of
 * geoadv_emd_cost_grad1_temp_floats(b,n,m) floats.  Equal to the three separate ops up to the order of the fp32 sums. */
size_t geoadv_emd_cost_grad1_temp_floats(int b, int n, int m);
int geoadv_emd_cost_grad1(int b, int n, int m, const float *xyz1, const float *xyz2, float *cost, float *grad1,
                          float *temp, void *stream);
int geoadv_emd_cost_grad1_mode(int mode, int b, int n, int m, const float *xyz1, const float *xyz2, float *cost,
                               float *grad1, float *temp, void *stream);
/* matchcostgradLauncher (tf_approxmatch.cpp:143; tf_approxmatch_g.cu:229-295).  grad2 may be NULL (only grad1 wanted). */
int geoadv_match_cost_grad(int b, int n, int m, const float *xyz1, const float *xyz2,
                           const float *match, float *grad1, float *grad2, void *stream);

/* ------------------------------------------------------------------------------------------
 * Grouping: external/grouping
 * ---------------------------------------------------------------------------------------- */

/* queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt) (tf_grouping.cpp:66;
 * tf_grouping_g.cu:3-36,125-128). */
int geoadv_query_ball_point(int b, int n, int m, float radius, int nsample,
                            const float *xyz1, const float *xyz2, int *idx, int *pts_cnt, void *stream);
/* selectionSortLauncher(b,n,m,k,dist,outi,out) (tf_grouping.cpp:108; tf_grouping_g.cu:83-131).
 * dist, outi, out are (b,m,n).  The first k entries of every row equal the reference's; the
 * remaining n-k entries hold the unselected elements in the reference's (swap) order too. */
int geoadv_selection_sort(int b, int n, int m, int k, const float *dist, int *outi, float *out, void *stream);
/* groupPointLauncher(b,n,c,m,nsample,points,idx,out) (tf_grouping.cpp:142; tf_grouping_g.cu:40-57). */
int geoadv_group_point(int b, int n, int c, int m, int nsample, const float *points, const int *idx,
                       float *out, void *stream);
/* groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points) (tf_grouping.cpp:173;
 * tf_grouping_g.cu:61-78).  grad_points is zeroed here (the reference op memsets it,
 * tf_grouping.cpp:204) and accumulated in a fixed order (no float atomics). */
int geoadv_group_point_grad(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                            float *grad_points, void *stream);
/* ... on caller-owned scratch (geoadv_group_point_grad_workspace_bytes bytes) instead of the stream-ordered allocation the
 * reference-shaped form above makes (its launcher prototype has no scratch argument). */
size_t geoadv_group_point_grad_workspace_bytes(int b, int n, int c, int m, int nsample);
int geoadv_group_point_grad_ws(int b, int n, int c, int m, int nsample, const float *grad_out, const int *idx,
                               float *grad_points, void *workspace, size_t workspace_bytes, void *stream);
/* knn_point(k, xyz1, xyz2) (tf_grouping.py:48-75) fused: squared distances + the k smallest per
 * query in the order SelectionSort produces (incl. its swap tie rule), without the (b,m,n)
 * matrix or the two tiled (b,m,n,3) operands.  val, idx are (b,m,k).  1 <= k <= 64. */
int geoadv_knn_point(int b, int n, int m, int k, const float *xyz1, const float *xyz2,
                     float *val, int *idx, void *stream);
/* defender/get_knn_dists_per_point.py:78-81 fused: knn_point(k+1, pc, pc), drop the first column,
 * gather, euclidean distance.  out is (b,n,k). */
int geoadv_knn_dists(int b, int n, int k, const float *pc, float *out, void *stream);
/* Which kernel answers a k-NN call with k <= 16 (same results, bit for bit): */
#define GEOADV_KNN_AUTO        0   /* by size: datasets of >= 512 points the exact grid search, smaller ones the all-points kernel */
#define GEOADV_KNN_ALL_POINTS  1
#define GEOADV_KNN_GRID        2   /* the grid search at every size                                                               */
#define GEOADV_KNN_GRID_SHELLS 3   /* as GRID without the lane-private first pass (every query by the wave-uniform shell walk)     */
/* The two ops with the kernel selected PER CALL (`kernel` = GEOADV_KNN_*) on caller-owned scratch of
 * geoadv_knn_workspace_bytes(b,n,m,k) bytes (knn_dists: m = n and k + 1 neighbours) -- no allocation, nothing process-wide: what
 * concurrent host threads call.  The reference-shaped forms above (tf_grouping.py:48-75 has no scratch argument) allocate
 * stream-ordered scratch per call and follow the process default below. */
size_t geoadv_knn_workspace_bytes(int b, int n, int m, int k);
int geoadv_knn_point_ws(int kernel, int b, int n, int m, int k, const float *xyz1, const float *xyz2,
                        float *val, int *idx, void *workspace, size_t workspace_bytes, void *stream);
int geoadv_knn_dists_ws(int kernel, int b, int n, int k, const float *pc, float *out,
                        void *workspace, size_t workspace_bytes, void *stream);
/* TEST / MEASUREMENT ONLY: the process default (GEOADV_KNN_*) of geoadv_knn_point / geoadv_knn_dists; an atomic word read at
 * launch time, not meant to be flipped while other threads launch -- those pass `kernel` to the _ws forms. */
int geoadv_knn_grid_mode(int mode);

/* Farthest point sampling: per cloud of xyz[b,n,3], m indices into the cloud, each the point farthest from those chosen before
 * it -- the sibling of the grouping operators above (PointNet++'s sampling layer; not part of the reference).  One launch for the
 * batch, one workgroup or one wave per cloud, the cloud and its distances in registers throughout (csrc/sampling.hip).
 * The rule, all fp32, every product and sum rounded on its own (no fused multiply-add):
 *   t[i] = +inf where point i is finite, -1 where one of its coordinates is NaN or an infinity;   cur = start
 *   for s = 0 .. m-1:   idx[s] = cur
 *                       d[i] = ((x[i]-x[cur])^2 + (y[i]-y[cur])^2) + (z[i]-z[cur])^2;   t[i] = d[i] where d[i] < t[i]
 *                       cur = the index of the largest t, the LOWEST index among equals
 * so: t is never NaN (a NaN d replaces nothing); a non-finite point is never chosen, except as the given start, which is
 * emitted as given; once every finite point has t = 0 (duplicates, or more picks than distinct points) the lowest such index
 * repeats; with no finite point every pick after the first is 0; a start outside [0, n) reads as 0; m == n on distinct finite
 * points yields a permutation, the cloud in farthest-point order.  There is no skip of points near the origin (the PointNet++
 * CUDA kernel's |p|^2 <= 1e-3 test is not reproduced).
 * start: device [b] or NULL = 0.  idx[b,m].  sampled (may be NULL) [b,m,3]: the bits of the chosen points.  mindist (may be
 * NULL) [b,n]: the final t, the squared distance of every point to the chosen set (-1 for a non-finite point).
 * form: which kernel answers the call, same bits -- GEOADV_FPS_AUTO (n <= 256: a wave per cloud, else a workgroup per cloud),
 * GEOADV_FPS_WORKGROUP (every n), GEOADV_FPS_WAVE (n <= 1024).
 * Enqueues on `stream` only.  GEOADV_EINVAL: b < 1, n < 1, n > 16384, m < 1, m > n, xyz or idx NULL, sampled or mindist
 * overlapping xyz, an unknown form, GEOADV_FPS_WAVE with n > 1024. */
#define GEOADV_FPS_AUTO      0
#define GEOADV_FPS_WORKGROUP 1
#define GEOADV_FPS_WAVE      2
int geoadv_farthest_point_sample(int b, int n, const float *xyz /* [b,n,3] */, int m,
                                 const int *start /* device [b] or NULL = 0 */, int form, int *idx /* [b,m] */,
                                 float *sampled /* [b,m,3] or NULL */, float *mindist /* [b,n] or NULL: the final t */, void *stream);
/* The kernel instance that answers a cloud of n points under `form`, without a launch (tests pin every boundary of the dispatch):
 * *form_out = GEOADV_FPS_WORKGROUP or GEOADV_FPS_WAVE, *waves = the waves that share a cloud, *points_per_thread.  Any of the
 * three may be NULL.  GEOADV_EINVAL where geoadv_farthest_point_sample refuses (n, form). */
int geoadv_farthest_point_sample_plan(int n, int form, int *form_out, int *waves, int *points_per_thread);

/* get_outlier_pc_inlier_pc (src/adversary_utils.py:149-178) on the device, fused with the score its caller forms
 * (defender/run_defense_surface.py:187-191: the mean of the first top_k kNN distances of a point): a point is an outlier if
 * mean(knn_dists[b,p,0:top_k]) > thresh, an inlier if <= thresh (a NaN score is neither, as with np.where).  knn_dists is
 * (b,n,knn_stride), 1 <= top_k <= min(knn_stride, 7); with knn_stride = top_k = 1 it is the reference function's own
 * per-point scalar.  Outputs as the reference's: inlier_pc / outlier_pc (b,n,3) packed in point order and padded with the last
 * packed point (zeros if none), outlier_idx (b,n) int16 zero-padded, outlier_num (b) int16.  outlier_pc / outlier_idx /
 * outlier_num may be NULL. */
int geoadv_outlier_filter(int b, int n, const float *pc, const float *knn_dists, int knn_stride, int top_k, float thresh,
                          float *outlier_pc, short *outlier_idx, short *outlier_num, float *inlier_pc, void *stream);

/* Statistical outlier removal (SOR; the baseline defense of DUP-Net and IF-Defense; not part of the reference): the scale-free
 * form of geoadv_outlier_filter, with a per-cloud threshold mean + alpha * std of the kNN score in place of one absolute
 * threshold.  One 1024-thread workgroup per cloud (csrc/stat_defense.hip).  The rule, all float64, every product and sum
 * rounded on its own (no fused multiply-add):
 *   s_p = (((double)knn_dists[p][0] + (double)knn_dists[p][1]) + ... + (double)knn_dists[p][k-1]) / (double)k
 *   a non-finite s_p (NaN, +-inf) stays out of the statistics and makes p an outlier;  m = the number of finite scores
 *   mu  = SUM(s_p) / m                    (0 for m = 0)
 *   var = SUM((s_p - mu) * (s_p - mu)) / (m - 1)      (0 for m < 2)
 *   p is an INLIER iff s_p is finite and (s_p <= mu or (s_p - mu) * (s_p - mu) <= (alpha * alpha) * var)
 * which is s_p <= mu + alpha * sigma without a square root, so that the outcome does not hang on how a device rounds sqrt.
 * SUM runs over ALL points, a non-finite score adding +0.0, in a FIXED order that is part of the rule, with T = 1024:
 *   1. thread t of T starts at +0.0 and adds the terms of points t, t + T, t + 2T, ... in ascending order,
 *   2. the 64 threads 64w .. 64w+63 of wave w combine in the xor butterfly v += v[lane ^ mask], mask = 1, 2, 4, 8, 16, 32,
 *   3. the T / 64 = 16 wave sums are added in ascending order of w, starting from wave 0's.
 * knn_dists is (b,n,knn_stride); any per-point array serves (squared distances give IF-Defense's variant).
 * Outputs as geoadv_outlier_filter's: inlier_pc / outlier_pc (b,n,3) packed in point order and padded with the last packed
 * point (zeros if none), outlier_idx (b,n) int16 zero-padded, outlier_num (b) int16; outlier_pc / outlier_idx / outlier_num
 * may be NULL.  stats (may be NULL) [b,3] = (mu, var, (double)m) per cloud.
 * Enqueues on `stream` only.  GEOADV_EINVAL, before any launch: alpha < 0 or not finite, k < 1, k > knn_stride,
 * knn_stride > 64, n < 1, n > 32767 (int16 never wraps), b < 0, pc, knn_dists or inlier_pc NULL with b > 0.  b == 0 is a no-op. */
int geoadv_sor_filter(int b, int n, const float *pc /* [b,n,3] */, const float *knn_dists /* [b,n,knn_stride] */, int knn_stride,
                      int k, double alpha, float *outlier_pc, short *outlier_idx, short *outlier_num, float *inlier_pc,
                      double *stats /* [b,3] or NULL */, void *stream);

/* Simple random sampling (SRS; the other baseline defense of the point-cloud attack literature; not part of the reference):
 * every cloud loses `drop` points chosen by a counter-based draw.  mix = splitmix64's finaliser, G = 0x9e3779b97f4a7c15,
 * 64-bit wrap-around; for the cloud slot s = slot_offset + i of cloud i and point p
 *   r(p) = mix(mix(mix(mix(seed + G) ^ counter) ^ (s << 32 | p)) + 48 * G)
 * (the key of geoadv_batch_gather, stream 48: batch_gather uses streams 1..3 and augment_batch 16..32).  The dropped points are
 * the `drop` points with the smallest (r(p), p) in lexicographic order (r is a bijection of p within a slot, so the draws
 * of a cloud never tie).  kept_pc (b,n,3): the other n - drop points in point order (the bits of pc), padded with the last
 * kept point.  dropped_idx (may be NULL) [b,drop]: the dropped points, ascending.  drop == 0 copies the bits of pc.
 * The result depends on (seed, counter, s, p) alone -- not on b, the grid or the data: ranks that pass slot_offset = rank *
 * local batch draw what one rank would have drawn.
 * One 1024-thread workgroup per cloud (csrc/stat_defense.hip): the drop-th smallest draw is found by an 8-bit radix select
 * over the 64-bit words on an LDS histogram (8 passes, O(n) each; no all-pairs form at any size), then two stable packings.
 * Enqueues on `stream` only.  GEOADV_EINVAL, before any launch: b < 0, n < 1, n > 32767, drop < 0, drop >= n,
 * slot_offset + b > 2^32, pc or kept_pc NULL with b > 0, kept_pc overlapping pc.  b == 0 is a no-op. */
int geoadv_random_drop(int b, int n, const float *pc /* [b,n,3] */, int drop, unsigned long long seed, unsigned long long counter,
                       unsigned long long slot_offset, float *kept_pc /* [b,n,3] */, int *dropped_idx /* [b,drop] or NULL */,
                       void *stream);

/* The kNN outlier loss of the kNN attack (Tsai, Yang, Chen: Robust Adversarial Objects against Deep Learning Models, AAAI 2020;
 * not part of the reference) and its gradient: the term that penalises exactly the points geoadv_sor_filter would remove, so that
 * a perturbation stays on the surface and survives the filter.  The search (geoadv_knn_point_ws) and ONE further launch, one
 * 1024-thread workgroup per cloud (csrc/knn_loss.hip).  The rule, for one cloud x[n,3] (fp32), k and alpha:
 *   neighbours  (val, N) = knn_point(k + 1, x, x) with the first column dropped (as geoadv_knn_dists drops it), in knn_point's tie
 *               order: N[p][0..k-1] the indices, val[p][c] = ((dx*dx + dy*dy) + dz*dz) of x_p - x_N[p][c] in fp32, every product
 *               and sum rounded on its own (no fused multiply-add), recomputed from the coordinates
 *   score       s_p, m, mu, var and SUM: the SOR rule above, word for word, applied to val (squared distances: IF-Defense's
 *               variant), all float64, SUM in its fixed T = 1024 order (a NaN score is a NaN; its sign and payload are no part
 *               of the rule)
 *   mask        w_p = 1 iff s_p is finite and s_p > mu and (s_p - mu) * (s_p - mu) > (alpha * alpha) * var
 *               -- among finite scores exactly the complement of SOR's inlier test; a non-finite score gives w_p = 0.  The mask
 *               is a CONSTANT of the differentiation: no gradient flows through mu or var (as in the published implementations)
 *   loss        K = SUM(w_p ? s_p : +0.0) / (double)n, float64
 *   gradient    accumulated in float64, per component, in an order that is part of the rule:
 *                 G_i = +0.0
 *                 if w_i:  for c = 0 .. k-1 ascending:  G_i += (double)x_i - (double)x_N[i][c]
 *                 for p = 0 .. n-1 ascending with w_p = 1, within p for c ascending with N[p][c] == i:
 *                                                        G_i += (double)x_i - (double)x_p
 *                 grad_i = (float)(G_i * (2.0 / ((double)n * (double)k)))        one rounding to fp32
 *               a point that no masked point lists and that is not masked itself gets +0.0.  This is the float64 gradient of K
 *               with the mask held constant.  No float atomics: two calls give the same bits; a point's in-degree is unbounded
 *               (ties can make many masked points name one neighbour) and nothing is truncated.
 * Outputs: loss [b]; grad [b,n,3] or NULL (then the loss alone is formed); score [b,n] (s_p), mask [b,n] (w_p as 0 / 1),
 * idx [b,n,k] (N), stats [b,4] = (mu, var, (double)m, the number of masked points) -- each may be NULL.
 * workspace: geoadv_knn_outlier_loss_workspace_bytes(b,n,k) bytes of device memory, caller-owned, nothing process-wide; 256
 * bytes for shapes the call refuses.  kernel: GEOADV_KNN_* for the search (same bits).
 * Enqueues on `stream` only.  GEOADV_EINVAL, before any launch: b < 0, b > 65535, k < 1, k > 15, n < k + 2, n > 32767 -- and,
 * for as long as the search keeps a row of the cloud in LDS, n > 16384 --, alpha < 0 or not finite, xyz or loss NULL with b > 0,
 * a workspace that is too small, an unknown kernel, grad overlapping xyz.  b == 0 is a no-op.
 *
 * The SURFACE rule (GEOADV_KNN_LOSS_SURFACE OR-ed into `kernel`, as GEOADV_EMD_DENSE_LEVELS is OR-ed into a mode): the same call
 * with the mask of the paper's off-surface defense -- exactly the points geoadv_outlier_filter(x, geoadv_knn_dists(x, k), thr,
 * top_k = k) removes -- and a hinge on it.  `alpha` is then the threshold, used as thr = (float)alpha.  Without the flag nothing
 * above changes.  For one cloud x[n,3] (fp32), k and thr:
 *   neighbours  N and val as above (knn_point(k + 1), first column dropped, tie order kept; val recomputed in fp32, every product
 *               and sum rounded on its own)
 *   distance    d[p][c] = sqrtf(val[p][c]), correctly rounded fp32: the bits geoadv_knn_dists writes
 *   score       s_p = ((d[p][0] + d[p][1]) + ... + d[p][k-1]) / (float)k, all fp32, left to right, no division for k = 1: knn_score
 *               of csrc/defense.hip, i.e. numpy's float32 mean of fewer than 8 elements -- hence 1 <= k <= 7, geoadv_outlier_filter's limit
 *   mask        w_p = 1 iff s_p > thr in fp32: geoadv_outlier_filter's outlier test.  A NaN score gives 0, +inf gives 1.  A constant
 *               of the differentiation
 *   loss        K = SUM(w_p ? (double)s_p - (double)thr : +0.0) / (double)n, float64, SUM in the SOR rule's fixed T = 1024 order; no
 *               point over the threshold gives +0.0
 *   gradient    float64 per component, in the order above (the gather over a masked point's own neighbours with c ascending, then
 *               the scatter over p ascending and within p over c ascending); an edge (p, c) with j = N[p][c] adds to its endpoint i
 *                 ((double)x_i - (double)x_other) / (double)d[p][c]       a float64 division, rounded once
 *               where x_other is the edge's other endpoint and d[p][c] is recomputed from the two coordinates (the fp32 squared
 *               distance has the same bits from either end); an edge with d[p][c] == 0 adds nothing (subgradient 0);
 *                 grad_i = (float)(G_i * (1.0 / ((double)n * (double)k)))
 * Outputs: score [b,n] = (double)s_p; mask and idx as above; stats [b,4] = ((double)thr, +0.0, the number of scores that are not
 * NaN, the number of masked points).  The workspace size is unchanged.  GEOADV_EINVAL, before any launch, under the flag: k > 7,
 * alpha negative, not finite or above FLT_MAX; with or without it: bits of `kernel` other than the flag and a GEOADV_KNN_* value;
 * everything refused above.  (geoadv_debug_knn_outlier_loss_launch has no `kernel` argument: it launches the SOR rule only.) */
#define GEOADV_KNN_LOSS_SURFACE 0x100
size_t geoadv_knn_outlier_loss_workspace_bytes(int b, int n, int k);
int geoadv_knn_outlier_loss(int kernel /* GEOADV_KNN_* for the search */, int b, int n, int k, double alpha,
                            const float *xyz /* [b,n,3] */, double *loss /* [b] */, float *grad /* [b,n,3] or NULL */,
                            double *score /* [b,n] or NULL */, unsigned char *mask /* [b,n] or NULL */,
                            int *idx /* [b,n,k] or NULL */, double *stats /* [b,4] or NULL: mu, var, m, number masked */,
                            void *workspace, size_t workspace_bytes, void *stream);
/* TEST / MEASUREMENT ONLY: the launch after the search alone, on a workspace in which a geoadv_knn_outlier_loss call of the same
 * (b, n, k) on the same xyz left its neighbours (tools/knn_loss_time.py times it).  Refuses what that call refuses. */
int geoadv_debug_knn_outlier_loss_launch(int b, int n, int k, double alpha, const float *xyz, double *loss, float *grad /* or NULL */,
                                         void *workspace, size_t workspace_bytes, void *stream);

/* get_critical_points + get_critical_pc_non_critical_pc (src/ae_utils.py:12-80) on the device, from (max_val, max_idx) =
 * (np.max, np.argmax)(pre_symmetry, axis=1) as geoadv_ae_critical returns them: (b,c) each.  critical_points (b,c,3) /
 * critical_idx (b,c) int16: the distinct arg-max points of the channels with max_val > 0, the point owning most channels first,
 * zero-padded; critical_num (b) int16; critical_pc (b,n,3): those points padded with the last of them; non_critical_pc (b,n,3):
 * every other point in point order, padded with the last.  Points owning EQUALLY many channels come in descending point
 * index (what a stable sort makes of the reference's np.argsort(counts)[::-1]; numpy's default sort leaves that order to the
 * build).  Any output may be NULL.  c <= 1024, n <= 32768. */
int geoadv_critical_split(int b, int n, int c, const float *pc, const float *max_val, const int *max_idx,
                          float *critical_points, short *critical_idx, short *critical_num, float *critical_pc,
                          float *non_critical_pc, void *stream);

/* sort_axes (src/shift_rotate_util.py:22-62) on the device: per cloud of pc[b,n,3] the longer of the x and y extents
 * (max - min, fp32) becomes x; z stays.  axes_idx[b,3] (may be NULL) is the reference's np.argsort([ex, ey, 0])[::-1]:
 * {0,1,2} for ex > ey, {1,0,2} for ex < ey AND for ex == ey (the reference swaps on a tie).  Only where ex < ey strictly is
 * axis (neg_rot ? 1 : 0) of the result negated (the swap becomes a rotation about z).  out[b,n,3] holds copies and sign
 * flips of the input only: the reference's bits.  Where an x or y extent is exactly 0 the reference's own assertion fails;
 * the rule above goes on holding here.  A NaN extent orders as the largest, as in numpy.  out must not be pc.
 * 1 <= n <= 16384, b >= 1, else GEOADV_EINVAL. */
int geoadv_sort_axes(int b, int n, const float *pc, float *out, int *axes_idx /* [b][3], may be NULL */, int neg_rot,
                     void *stream);

/* One training batch built on the device in one launch: clean[i] = the bits of data[index[i]] (data[num_clouds,n,3] resident,
 * index device [b] or NULL = 0..b-1), feed[i] = that cloud with Gaussian noise and / or a rotation.  aug == NULL: feed holds the
 * gathered bits.  Rotation: every point as a row vector times R (the reference's batch.dot(R), src/general_utils.py:142),
 * float64 products and sums rounded once to fp32.  Noise of output slot s = slot_offset + i, point p, coordinate c (mix =
 * splitmix64's finaliser, G = 0x9e3779b97f4a7c15, 64-bit wrap-around):
 *   key = mix(mix(mix(seed + G) ^ counter) ^ (s << 32 | p));  r = mix(key + (c + 1) * G)
 *   u1 = ((r >> 40) + 1) * 2^-24;  u2 = ((r >> 16) & 0xFFFFFF) * 2^-24;  g = sqrt(-2 ln u1) * cos(2 pi u2)   (fp32)
 *   value = x + (mu + clamp(sigma * g, -clip, clip))   (three fp32 roundings)
 * so it depends on (seed, counter, s, p, c) alone.  GEOADV_EINVAL: b, n or num_clouds < 1, rot_count not in {0, 1, b},
 * rot == NULL with rot_count > 0, data or feed NULL, feed or clean overlapping data or each other, slot_offset < 0, sigma < 0.
 * An index outside [0, num_clouds) is never dereferenced: that slot of clean and feed is left unwritten. */
typedef struct geoadv_batch_augment {
    unsigned long long seed, counter;  /* generator key; counter = the caller's global step ordinal */
    int   slot_offset;                 /* slot of output cloud 0 (data-parallel ranks: rank * local batch) */
    float noise_mu, noise_sigma;       /* sigma == 0: no noise is generated and mu is ignored */
    float noise_clip;                  /* > 0: sigma * g is clamped to [-clip, clip]; <= 0: no clamp */
    int   rot_count;                   /* 0: none; 1: one matrix for the batch; b: one per cloud */
    int   rotate_first;                /* 0: noise then rotation (AE order); 1: rotation then noise (classifier order) */
} geoadv_batch_augment;
int geoadv_batch_gather(int b, int n, const float *data, long long num_clouds, const int *index /* device [b] or NULL = 0..b-1 */,
                        const geoadv_batch_augment *aug /* NULL = plain gather */, const double *rot /* device [rot_count][9], row-major */,
                        float *clean /* device [b,n,3] or NULL */, float *feed /* device [b,n,3] */, void *stream);

/* Normalization (transfer/atlasnet/dataset/pointcloud_processor.py:160-233) on the device: out[b,n,3] = (pc - c) * s per cloud.
 *   GEOADV_NORMALIZE_IDENTITY      the bits of pc
 *   GEOADV_NORMALIZE_UNIT_BALL     c = the cloud's mean, s = 1 / sqrt(max_p ||p - c||^2)
 *   GEOADV_NORMALIZE_BOUNDING_BOX  c = (min + max) / 2 per axis, s = 1 / max_axis((max - min) / 2)   (the reference's isotropic form)
 * c and s are float64 (sums in a fixed order: bitwise reproducible, whatever the grid), (x - c) * s is evaluated in float64
 * and rounded to fp32 once.  A NaN coordinate wins every extremum, so its cloud comes out all NaN; a cloud whose points all
 * coincide (n = 1 included) comes out all NaN as well (0 * 1/0), as in the reference; other clouds are unaffected.
 * out must not be pc.  b >= 1, 1 <= n <= 2^20, else GEOADV_EINVAL. */
#define GEOADV_NORMALIZE_IDENTITY 0
#define GEOADV_NORMALIZE_UNIT_BALL 1
#define GEOADV_NORMALIZE_BOUNDING_BOX 2
int geoadv_normalize_clouds(int b, int n, int kind, const float *pc, float *out, void *stream);

/* One AtlasNet training batch in one launch: gather by index out of data[num_clouds,n_src,3], optional re-sampling of n_out
 * points with replacement, then the Augmenter's operators (transfer/atlasnet/dataset/augmenter.py) in its order: axial
 * rotations (ascending axis), 3-D rotation, anisotropic scale, flips, translation.  A point is a row vector times a matrix.
 *
 * The operators of an output cloud are one record of GEOADV_AUGMENT_RECORD fp32 values:
 *   [0, 27)   the axial rotation about axis 0, 1, 2: three row-major 3x3 matrices (Operation.get_3D_rot_matrix)
 *   [27, 36)  the 3-D rotation, row-major (DataAugmentation.get_random_rotation_matrix)
 *   [36, 39)  scale per axis      [39, 42)  flip per axis (+1 / -1)      [42, 45)  translation per axis
 * An operator that the configuration does not enable holds its identity (unit matrix, 1, 1, 0) and is not applied.
 * params != NULL: device [b][GEOADV_AUGMENT_RECORD], the enabled operators are taken from it and nothing is drawn.
 * params_out != NULL: device [b][GEOADV_AUGMENT_RECORD], receives the record that was applied, drawn or given.
 * The fp32 operators are composed into one affine map in float64; every point is evaluated in float64 and rounded once.
 * With no operator enabled the output holds the source points' bits.
 *
 * Draws of output slot s = slot_offset + i (mix = splitmix64's finaliser, G = 0x9e3779b97f4a7c15, 64-bit wrap-around):
 *   r(q, k) = mix(mix(mix(mix(seed + G) ^ counter) ^ (s << 32 | q)) + k * G)       q = 0 for the operators, k the stream
 *   u(k)  = (r >> 40) * 2^-24 in [0, 1);   normal g(k) = sqrt(-2 ln(((r >> 40) + 1) * 2^-24)) * cos(2 pi ((r >> 16) & 0xFFFFFF) * 2^-24)
 *   axial, axis a      k = 16 + a   angle = u * 2K - K, K = pi * range_rot / 360 (float64); cos / sin in float64
 *   3-D rotation       k = 19 + a   axis = (g(19), g(20), g(21)) / its norm;   k = 22   angle = u * 2 pi + pi (float64)
 *   scale, axis a      k = 23 + a   u * (scale_max - scale_min) + scale_min           (fp32, every operation rounded)
 *   flip, axis a       k = 26 + a   +1 where r >> 63 is set, else -1
 *   translation, a     k = 29 + a   (u * 2) * translate_scale - translate_scale       (fp32, every operation rounded)
 *   sample, point p    k = 32, q = p   source point j = ((r >> 32) * n_src) >> 32       (integers only)
 * Matrix entries are computed in float64 and rounded to fp32 once.  The draws depend on (seed, counter, s, k, p) alone.
 *
 * GEOADV_EINVAL: a dimension < 1, out overlapping data (or params_out), n_out != n_src without sample, rot_axes or flip_axes
 * outside [0, 7], range_rot outside (0, 360] with rot_axes, scale_min > scale_max or either not finite with scale, a
 * translate_scale that is negative or not finite with translate, slot_offset < 0.  An index outside [0, num_clouds) is never
 * dereferenced: that slot of out and params_out is left unwritten. */
#define GEOADV_AUGMENT_RECORD 45
typedef struct geoadv_cloud_augment {
    unsigned long long seed, counter;  /* generator key; counter = the caller's global step ordinal */
    int   slot_offset;                 /* slot of output cloud 0 (data-parallel ranks: rank * local batch) */
    int   sample;                      /* 0: n_out == n_src, points in order; 1: n_out points drawn with replacement */
    int   rot_axes;                    /* bit a: random rotation about axis a */
    float range_rot;                   /* degrees, in (0, 360]; the reference's default is 360 */
    int   rot_3d;                      /* 1: random 3-D rotation */
    int   scale;                       /* 1: anisotropic scale in [scale_min, scale_max) */
    float scale_min, scale_max;        /* the reference's defaults are 0.75 and 1.25 */
    int   flip_axes;                   /* bit a: random flip of axis a */
    int   translate;                   /* 1: translation in [-translate_scale, translate_scale) per axis */
    float translate_scale;             /* the reference's default is 0.03 */
} geoadv_cloud_augment;
int geoadv_augment_batch(int b, int n_out, const float *data, long long num_clouds, int n_src,
                         const int *index /* device [b] or NULL = 0..b-1 */, const geoadv_cloud_augment *cfg /* NULL = plain gather */,
                         const float *params /* device [b][45] or NULL */, float *params_out /* device [b][45] or NULL */,
                         float *out /* device [b,n_out,3] */, void *stream);

/* get_dist_mat (src/general_utils.py:94-106) on the device: out[na,nb], out[i][j] = || a[i] - b[j] ||_2 of the fp32 row-major
 * a[na,d] and b[nb,d] -- the latent distance matrix of attacker/prepare_indices_for_attack.py:89-101.  Bit for bit numpy's
 * np.linalg.norm(s - t, axis=-1): fp32 differences, squares rounded on their own, numpy's pairwise summation order of a
 * contiguous run of d <= 128 elements (eight accumulators, combined as a tree, the last d mod 8 elements added one by one),
 * a correctly rounded square root, denormals kept.  With b == a the matrix is exactly symmetric and its diagonal is +0.
 * 1 <= d <= 128 and na, nb >= 0, else GEOADV_EINVAL; na == 0 or nb == 0 is a no-op. */
int geoadv_latent_dist_matrix(int na, int nb, int d, const float *a, const float *b, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Victim auto-encoder: src/encoders_decoders.py:19-147 with the architecture of
 * src/ae_templates.py:11-39 (5 x [conv1d k=1, BN(inference), ReLU], max over points,
 * FC-ReLU, FC-ReLU, FC).
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_ae geoadv_ae;

#define GEOADV_ENC_LAYERS 5
#define GEOADV_DEC_LAYERS 3

/* Host-side description of the weights, in the reference's variable layout
 * (adversary_autoencoder.py:42-51 restores exactly these variables):
 *   enc_w[i]  : [C_i, C_{i+1}]   (tflearn conv_1d W[1,1,Cin,Cout] squeezed), enc_b[i] : [C_{i+1}]
 *   bn_*[i]   : [C_{i+1}]         gamma, beta, moving_mean, moving_variance (eps = 1e-5)
 *   dec_w[k]  : [D_k, D_{k+1}], dec_b[k] : [D_{k+1}]
 * enc_dims = {3, 64, 128, 128, 256, bneck}; dec_dims = {bneck, 256, 256, 3*n_points}.
 * This build supports the template's widths (every C_i, i>=1, a multiple of 32; bneck = 128). */
typedef struct geoadv_ae_weights {
    int n_points;
    int enc_dims[GEOADV_ENC_LAYERS + 1];
    int dec_dims[GEOADV_DEC_LAYERS + 1];
    const float *enc_w[GEOADV_ENC_LAYERS], *enc_b[GEOADV_ENC_LAYERS];
    const float *bn_gamma[GEOADV_ENC_LAYERS], *bn_beta[GEOADV_ENC_LAYERS];
    const float *bn_mean[GEOADV_ENC_LAYERS], *bn_var[GEOADV_ENC_LAYERS];
    const float *dec_w[GEOADV_DEC_LAYERS], *dec_b[GEOADV_DEC_LAYERS];
} geoadv_ae_weights;

/* Uploads (and re-packs for MFMA) the HOST weights.  Allocates device memory; synchronous. */
int  geoadv_ae_create(geoadv_ae **out, const geoadv_ae_weights *host_weights);
void geoadv_ae_destroy(geoadv_ae *ae);

/* Arithmetic of the encoder's four wide layers (the path's dominant kernel; 180 kFLOP per point).
 *   F32    : v_mfma_f32_32x32x2_f32 -- fp32 products, fp32 accumulate (bounded by the 157 TFLOP/s fp32 matrix peak).
 *   BF16X3 : every operand as three bf16 pieces (8 + 8 + 8 bits = the fp32's 24), a product as its six piece products of
 *            weight >= 2^-16, each exact in the fp32 accumulator, on v_mfma_f32_32x32x16_bf16 (csrc/encoder_x3.h).  Error
 *            against float64 = that of an fp32 accumulation in another order (profiles/r05_bf16x3_probe.jsonl); not the
 *            bits of F32.  Non-finite coordinates give NaN activations (inf - inf in the split) where F32 gives inf.
 *   F16X2  : every operand as TWO fp16 pieces (11 + 11 bits; remainder < 2^-23) of power-of-two-scaled values, a product as its
 *            three piece products of weight >= 2^-11, each exact in the fp32 accumulator, on v_mfma_f32_32x32x16_f16: half of
 *            BF16X3's matrix instructions, the same error against float64 (profiles/r06_f16x2_probe.jsonl: 0.44-0.52 units of
 *            2^-24 |a|.|w| rms, the fp32 chain's).  A layer's activations are carried times a power of two s_j -- 2^6 for a
 *            layer whose batch norm has gamma^2 + beta^2 = 1 on average, moved with that magnitude otherwise (what
 *            relu(gamma z + beta) puts out) --, its weights times the power of two that puts the largest in [2^13, 2^14);
 *            RANGE: an activation of 1023.5 x that magnitude or more does not fit (clouds far outside what the victim's
 *            batch norms were made for) -- the kernels check every activation they split, and a cloud that has one gets
 *            +inf latents (so that nothing downstream looks sane) and raises the model's sticky flag: geoadv_ae_status /
 *            geoadv_attack_status then return GEOADV_ERANGE.  Such clouds run under BF16X3.  Not available (set refuses, the
 *            default falls back to BF16X3) for a model with a non-finite weight or a folded constant outside the normal fp32
 *            range.
 * All reproduce themselves bit for bit (forward, recomputing backward, any batch).  The default of handles created from
 * now on (AUTO, the initial setting: F16X2 where available, else BF16X3) / of one handle (set before it is shared with attack
 * handles or threads). */
#define GEOADV_ENC_ARITH_AUTO  (-1)
#define GEOADV_ENC_ARITH_F32    0
#define GEOADV_ENC_ARITH_BF16X3 1
#define GEOADV_ENC_ARITH_F16X2  2
int  geoadv_set_default_encoder_arith(int arith);
int  geoadv_ae_set_encoder_arith(geoadv_ae *ae, int arith);
int  geoadv_ae_encoder_arith(const geoadv_ae *ae);
/* Synchronises `stream`; GEOADV_ERANGE (message in geoadv_last_error; the flag is cleared) if an F16X2 forward of this model since
 * the last call met an activation outside its range, else GEOADV_OK.  Callers that synchronise anyway (to read results) call it.
 * The flag is read behind everything queued on `stream` and cleared ON `stream`: a forward queued on that stream directly after
 * the call keeps the flag it raises.  Forwards of the model in flight on OTHER streams are not waited for: a caller that runs one
 * model on several streams synchronises those itself before it trusts GEOADV_OK. */
int  geoadv_ae_status(const geoadv_ae *ae, void *stream);

/* AdversaryAutoEncoder.reconstruct / AutoEncoder.transform (adversary_autoencoder.py:75-91):
 * pc[b,n,3] -> latent[b,bneck] (may be NULL) and recon[b,n,3] (may be NULL).
 * workspace: geoadv_ae_workspace_bytes(ae,b) bytes of device scratch. */
size_t geoadv_ae_workspace_bytes(const geoadv_ae *ae, int b);
/* Encoder only, with the arg-max of the symmetric pool (what src/ae_utils.py:19-20 derives from
 * get_pre_symmetry_data): latent[b,bneck] = max over points of the last encoder layer, arg_idx[b,bneck] = the
 * LOWEST point index attaining it (np.argmax semantics).  Same workspace as geoadv_ae_forward. */
int geoadv_ae_critical(const geoadv_ae *ae, int b, const float *pc, float *latent, int *arg_idx,
                       void *workspace, void *stream);
int geoadv_ae_forward(const geoadv_ae *ae, int b, const float *pc, float *latent, float *recon,
                      void *workspace, void *stream);
/* AutoEncoder.decode (src/autoencoder.py:191-194; used by interpolate, :178-189): latent[b,bneck] -> recon[b,n,3].
 * Same arithmetic as the decoder half of geoadv_ae_forward: decode(transform(x)) == reconstruct(x) bit for bit.
 * Same workspace as geoadv_ae_forward. */
int geoadv_ae_decode(const geoadv_ae *ae, int b, const float *latent, float *recon, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * PointNet classifier of the semantic evaluation: classifier/pointnet_cls.py:30-84 (get_model) with the
 * T-Nets of classifier/transform_nets.py, inference only (is_training = False: batch norm from the moving
 * statistics with eps 1e-3, dropout the identity), fp32.  csrc/classifier.hip.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_cls geoadv_cls;

/* The 20 weight layers, in this order.  Every w is [fan_in, fan_out] row-major (conv2d's W[1,kw,Cin,Cout] squeezed:
 * conv1 / transform_net1's tconv1 are [3,64]), b is [fan_out].  gamma / beta / mean / var (the batch norm's variables and
 * moving statistics, [fan_out]) are given for every layer but TXYZ, TFEAT and FC3, whose BN pointers must be NULL.
 * TXYZ / TFEAT take the variables as stored: the identity (transform_nets.py) is added by the library. */
#define GEOADV_CLS_LAYERS    20
#define GEOADV_CLS_T1_CONV1   0   /* transform_net1/tconv1   3 -> 64    */
#define GEOADV_CLS_T1_CONV2   1   /* transform_net1/tconv2  64 -> 128   */
#define GEOADV_CLS_T1_CONV3   2   /* transform_net1/tconv3 128 -> 1024  */
#define GEOADV_CLS_T1_FC1     3   /* transform_net1/tfc1  1024 -> 512   */
#define GEOADV_CLS_T1_FC2     4   /* transform_net1/tfc2   512 -> 256   */
#define GEOADV_CLS_TXYZ       5   /* transform_net1/transform_XYZ 256 -> 9 (+I) */
#define GEOADV_CLS_CONV1      6   /* conv1   3 -> 64  */
#define GEOADV_CLS_CONV2      7   /* conv2  64 -> 64  */
#define GEOADV_CLS_T2_CONV1   8   /* transform_net2/tconv1  64 -> 64    */
#define GEOADV_CLS_T2_CONV2   9   /* transform_net2/tconv2  64 -> 128   */
#define GEOADV_CLS_T2_CONV3  10   /* transform_net2/tconv3 128 -> 1024  */
#define GEOADV_CLS_T2_FC1    11   /* transform_net2/tfc1  1024 -> 512   */
#define GEOADV_CLS_T2_FC2    12   /* transform_net2/tfc2   512 -> 256   */
#define GEOADV_CLS_TFEAT     13   /* transform_net2/transform_feat 256 -> 4096 (+I) */
#define GEOADV_CLS_CONV3     14   /* conv3  64 -> 64   */
#define GEOADV_CLS_CONV4     15   /* conv4  64 -> 128  */
#define GEOADV_CLS_CONV5     16   /* conv5 128 -> 1024 */
#define GEOADV_CLS_FC1       17   /* fc1  1024 -> 512  */
#define GEOADV_CLS_FC2       18   /* fc2   512 -> 256  */
#define GEOADV_CLS_FC3       19   /* fc3   256 -> num_classes, linear */
typedef struct geoadv_cls_weights {
    int num_classes;                              /* 1 ... 1024 (13 in the reference's scripts) */
    const float *w[GEOADV_CLS_LAYERS], *b[GEOADV_CLS_LAYERS];
    const float *gamma[GEOADV_CLS_LAYERS], *beta[GEOADV_CLS_LAYERS];
    const float *mean[GEOADV_CLS_LAYERS], *var[GEOADV_CLS_LAYERS];
} geoadv_cls_weights;

/* Uploads the HOST weights (batch norm folded into a per-channel scale / shift, the per-point layers packed for MFMA).
 * Allocates device memory; synchronous.  The handle is immutable afterwards (any number of threads / streams may use it). */
int  geoadv_cls_create(geoadv_cls **out, const geoadv_cls_weights *host_weights);
void geoadv_cls_destroy(geoadv_cls *cls);
/* Device scratch of geoadv_cls_forward for a batch of b clouds of n points. */
size_t geoadv_cls_workspace_bytes(const geoadv_cls *cls, int b, int n);
/* PointNetClassifier.classify (classifier/pointnet_classifier.py:62-82) without its batch-size restriction:
 * pc[b,n,3] -> logits[b,num_classes] and labels[b] (int32, np.argmax: the first maximum).  transform_in[b,3,3] (T1) and
 * transform_feat[b,64,64] (T2) return the two T-Nets' matrices.  Any of the four outputs may be NULL.  1 <= n <= 16384,
 * b >= 1, else GEOADV_EINVAL.  A cloud with non-finite coordinates affects no other cloud's results. */
int geoadv_cls_forward(const geoadv_cls *cls, int b, int n, const float *pc, float *logits, int *labels,
                       float *transform_in, float *transform_feat, void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * The classifier's INPUT GRADIENT: d loss / d pc through exactly the graph of geoadv_cls_forward (is_training = False),
 * both T-Nets included -- T1 and T2 are differentiated as functions of the points.  Not in the reference: the primitive of
 * the white-box classifier attacks (cls_attack.py), of saliency maps and of point dropping.  csrc/cls_grad.hip.
 * ---------------------------------------------------------------------------------------- */
#define GEOADV_CLS_LOSS_XENT           0   /* softmax cross entropy of labels[c], per cloud (no batch mean): dZ = softmax - onehot */
#define GEOADV_CLS_LOSS_CW_TARGETED    1   /* labels[c] = target t: max(max_{i != t} Z_i - Z_t, -kappa)                        */
#define GEOADV_CLS_LOSS_CW_UNTARGETED  2   /* labels[c] = true class y: max(Z_y - max_{i != y} Z_i, -kappa)                    */
/* Device scratch of geoadv_cls_input_grad for a batch of b clouds of n points. */
size_t geoadv_cls_input_grad_workspace_bytes(const geoadv_cls *cls, int b, int n);
/* pc[b,n,3], labels[b] (DEVICE int32) -> grad[b,n,3] = d loss[c] / d pc[c], with loss[b] (per cloud), logits[b,C] (bit-equal
 * to geoadv_cls_forward's) and winners[b,3,1024] on request (each may be NULL).
 * Rules (csrc/cls_train.hip's): the ReLU gradient is [output > 0]; a max pool passes its gradient to ONE row per (cloud,
 * column), the lowest point index among equal maxima; a pooled value of +0 passes none.  winners[c][p][k] is the row pool p
 * chose for column k (p = 0: T-Net1's pool, 1: T-Net2's, 2: the classifier's), 0 where the pooled value is +0.  A point
 * that wins no column of any pool gets a gradient of exactly zero.
 * The loss is computed in float64 from the fp32 logits Z and rounded once.  The CW kinds take the FIRST maximum over the
 * other classes, at j: if the unclamped value is > -kappa (strictly), dZ is +1 / -1 at (j, t) (targeted) or (y, j)
 * (untargeted); otherwise the cloud's gradient is exactly zero.  They need num_classes >= 2.
 * 1 <= n <= 16384, b >= 1, kappa >= 0 and finite, a known loss_kind, else GEOADV_EINVAL and nothing is written.  A label
 * outside [0, C) makes that cloud's loss and gradient NaN, reads nothing out of bounds and touches no other cloud; a cloud
 * with non-finite coordinates affects no other cloud.  All on `stream`, no host synchronisation; two calls on the same
 * input give the same bits; a cloud's outputs do not depend on its batch neighbours or on b. */
int geoadv_cls_input_grad(const geoadv_cls *cls, int b, int n, const float *pc, const int *labels, int loss_kind, float kappa,
                          float *loss, float *logits, int *winners, float *grad, void *ws, void *stream);

/* ------------------------------------------------------------------------------------------
 * Voted evaluation of the classifier (classifier/tst_classifier.py eval_one_epoch, one batch) and the rotation it votes
 * over (classifier/provider.py rotate_point_cloud_by_angle).  csrc/cls_eval.hip.
 * ---------------------------------------------------------------------------------------- */
/* out[b,n,3] = pc[b,n,3] @ [[c,0,s],[0,1,0],[-s,0,c]] with c = cos_angle, s = sin_angle computed by the caller: float32
 * points times the float64 matrix, products and sums in float64, rounded to float32 once.  out may be pc.  b == 0 or
 * n == 0 is a no-op; negative shapes return GEOADV_EINVAL. */
int geoadv_rotate_y(int b, int n, const float *pc, double cos_angle, double sin_angle, float *out, void *stream);
/* Device scratch of geoadv_cls_evaluate for a batch of b clouds of n points (any number of votes). */
size_t geoadv_cls_evaluate_workspace_bytes(const geoadv_cls *cls, int b, int n);
/* For vote v = 0 .. num_votes - 1: pc rotated by v / num_votes * 2 pi (or by the HOST array cos_sin[num_votes][2] =
 * (cos, sin) of every vote's angle when it is not NULL, read before the call returns), geoadv_cls_forward on it, and
 *   loss[v]              float32: mean_b(softmax cross entropy against labels) + 0.001 * sum_b(0.5 ||T2 T2^T - I||_F^2),
 *   pred_sum[b,C]        float64: the logits summed over the votes in vote order,
 *   vote_counts[b,C]     int32: how many votes had their arg-max at each class,
 *   pred[b]              int32: the first maximum of pred_sum after the last vote.
 * labels[b] is a DEVICE int32 array; NULL (or loss NULL) computes no loss.  A label outside [0, C) makes every loss[v] of
 * the call NaN and reads nothing out of bounds; the other outputs do not depend on the labels.  Any output may be NULL.
 * All on `stream`, no host synchronisation; two calls on the same input give the same bits.  1 <= n <= 16384, b >= 1,
 * 1 <= num_votes <= 64, else GEOADV_EINVAL. */
int geoadv_cls_evaluate(const geoadv_cls *cls, int b, int n, const float *pc, const int *labels, int num_votes,
                        const double *cos_sin, float *loss, int *pred, double *pred_sum, int *vote_counts,
                        void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * PointNet classifier TRAINING step (classifier/train_classifier.py train_one_epoch: sess.run([train_op, loss, pred]) at
 * is_training = True): batch norm from the batch's moments, differentiated through; dropout keep 0.7 after fc1 and fc2;
 * loss = mean softmax cross entropy + 0.001 * l2_loss(T2 T2^T - I); AdamOptimizer or MomentumOptimizer with the
 * staircase learning-rate and bn_decay schedules of the global step `batch`.  csrc/cls_train.hip (which states the
 * dropout generator exactly).  One handle = one model with a fixed batch and point count; no process-wide state.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_cls_trainer geoadv_cls_trainer;
#define GEOADV_CLS_OPT_ADAM     0
#define GEOADV_CLS_OPT_MOMENTUM 1
typedef struct geoadv_cls_train_config {
    int   batch;            /* BATCH_SIZE (32)                                                     */
    int   n_points;         /* NUM_POINT (2048); 1 ... 16384, batch * n_points <= 2^20            */
    int   optimizer;        /* GEOADV_CLS_OPT_ADAM / _MOMENTUM                                     */
    float learning_rate;    /* BASE_LEARNING_RATE (0.001)                                          */
    float momentum;         /* MOMENTUM (0.9), momentum only                                       */
    int   decay_step;       /* DECAY_STEP (200000), in samples                                     */
    float decay_rate;       /* DECAY_RATE (0.7)                                                    */
    int   initial_step;     /* the step counter `batch` to start from (0, or a restored value)      */
    int   dropout_seed;     /* key of the dropout generator                                        */
} geoadv_cls_train_config;
/* init: HOST values of every variable (mean / var = the moving averages).  Optimizer slots start at zero and the beta
 * powers at 0.9 / 0.999; geoadv_cls_trainer_set_slots restores them (flat, in the parameter layout). */
int  geoadv_cls_trainer_create(geoadv_cls_trainer **out, const geoadv_cls_weights *init, const geoadv_cls_train_config *cfg);
void geoadv_cls_trainer_destroy(geoadv_cls_trainer *t);
/* set_slots takes no stream: a synchronous copy from HOST memory (hipMemcpy), complete on return.  It does not wait for a step in
 * flight: the caller must have synchronised every stream on which a step of this handle was queued. */
int  geoadv_cls_trainer_set_slots(geoadv_cls_trainer *t, const float *slot1, const float *slot2, float beta1_power, float beta2_power);
/* x: device [batch][n][3], labels: device int32 [batch]; loss (device float, of the PRE-update variables) and pred (device
 * int32 [batch], argmax of the logits) may be NULL.  Updates the variables, slots, moving averages and the step counter. */
int geoadv_cls_trainer_step(geoadv_cls_trainer *t, const float *x, const int *labels, float *loss, int *pred, void *stream);
/* Device pointers of the flat parameter / gradient buffers (`count` floats each); offsets80[4 l + f] = where layer l's
 * weights [in][out] (f 0), biases (1), bn/gamma (2), bn/beta (3) sit ((size_t)-1: none); moving_offsets20[l] = where its
 * moving statistics sit in the MOVING_MEAN / MOVING_VAR arenas (may be NULL). */
int geoadv_cls_trainer_buffers(geoadv_cls_trainer *t, float **params, float **grads, size_t *count);
int geoadv_cls_trainer_layout(const geoadv_cls_trainer *t, size_t *offsets80, size_t *moving_offsets20);
/* The step counter and Adam's beta powers as they stand (after the last step). */
int geoadv_cls_trainer_counters(const geoadv_cls_trainer *t, long long *step, float *beta1_power, float *beta2_power);
/* Read-only TEST / export view of the device state: *ptr and its element count.
 *   BN_MEAN / BN_VAR / MOVING_MEAN / MOVING_VAR  float [C_layer]  batch statistics of the last step / moving averages
 *   DROPOUT_MASK   float [batch][512 | 256]   layer 0 = fc1, 1 = fc2 (0 / 1)
 *   POOL_ARGMAX    int [batch][1024]          pool 0 = T-Net1, 1 = T-Net2, 2 = conv5: the point of the first maximum
 *   T1 / T2 float [batch][9 | 4096], LOGITS float [batch][num_classes]   of the last step's forward
 *   SLOT1 / SLOT2  float [count]              Adam m / v, or Momentum's accumulator (SLOT1), in the parameter layout
 *   PRE_BN         float [rows][C_layer]      the stored pre-BN activation a of a BN layer; rows = batch * n_points for a
 *                                             per-point layer, batch for an fc layer
 *   BN_INV / BN_SHIFT  float [C_layer]        the folded constants of a BN layer: the step's ReLU input is
 *                                             a * inv + shift, two fp32 roundings (no contraction) */
#define GEOADV_CLS_STATE_BN_MEAN       0
#define GEOADV_CLS_STATE_BN_VAR        1
#define GEOADV_CLS_STATE_MOVING_MEAN   2
#define GEOADV_CLS_STATE_MOVING_VAR    3
#define GEOADV_CLS_STATE_DROPOUT_MASK  4
#define GEOADV_CLS_STATE_POOL_ARGMAX   5
#define GEOADV_CLS_STATE_T1            6
#define GEOADV_CLS_STATE_T2            7
#define GEOADV_CLS_STATE_LOGITS        8
#define GEOADV_CLS_STATE_SLOT1         9
#define GEOADV_CLS_STATE_SLOT2        10
#define GEOADV_CLS_STATE_PRE_BN       11
#define GEOADV_CLS_STATE_BN_INV       12
#define GEOADV_CLS_STATE_BN_SHIFT     13
int geoadv_cls_trainer_state(const geoadv_cls_trainer *t, int what, int layer, const void **ptr, size_t *count);

/* ------------------------------------------------------------------------------------------
 * AtlasNet auto-encoder of the transfer experiment: transfer/atlasnet/model/model_blocks.py (PointNet encoder :28-60,
 * Mapping2Dto3D decoder :63-105) in eval mode (atlasnet.py:45-67, train=False: the fixed template points), batch norm
 * from the running statistics with eps 1e-5, fp32.  csrc/atlasnet.hip.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_atlas geoadv_atlas;

#define GEOADV_ATLAS_ENC_LAYERS      5   /* conv1 3->64, conv2 64->128, conv3 128->1024 (BN, no ReLU), lin1, lin2 1024->1024 */
#define GEOADV_ATLAS_MAX_DEC_LAYERS  7   /* per primitive: conv1 dim->1024, conv2 1024->512, num_layers x 512->512, last_conv 512->3 */
typedef struct geoadv_atlas_config {
    int nb_primitives;          /* 1 ... 128 */
    int points_per_primitive;   /* template points per primitive (g * g for the SQUARE template), 1 ... 65536 */
    int dim_template;           /* 2 or 3 */
    int bottleneck_size;        /* 1024 */
    int hidden_neurons;         /* 512 */
    int num_layers;             /* 0 ... 4 */
    int activation;             /* 0 = relu (the only one supported) */
    int decoder_bn;             /* 1: the decoder has its batch norms; 0: remove_all_batchNorms (the encoder keeps its own) */
} geoadv_atlas_config;
/* Every w is [fan_in, fan_out] row-major (torch's Conv1d / Linear weight [out, in(, 1)] transposed), b is [fan_out].  The
 * encoder's five layers all have batch norm.  Decoder layer l of primitive p lives at dec_*[l] + p * (size of one primitive's
 * array), layers in the order conv1, conv2, conv_list[0 .. num_layers), last_conv (index 2 + num_layers).  The decoder's BN
 * pointers are given for every layer but last_conv when decoder_bn = 1, and must all be NULL otherwise. */
typedef struct geoadv_atlas_weights {
    const float *enc_w[GEOADV_ATLAS_ENC_LAYERS], *enc_b[GEOADV_ATLAS_ENC_LAYERS];
    const float *enc_gamma[GEOADV_ATLAS_ENC_LAYERS], *enc_beta[GEOADV_ATLAS_ENC_LAYERS];
    const float *enc_mean[GEOADV_ATLAS_ENC_LAYERS], *enc_var[GEOADV_ATLAS_ENC_LAYERS];
    const float *dec_w[GEOADV_ATLAS_MAX_DEC_LAYERS], *dec_b[GEOADV_ATLAS_MAX_DEC_LAYERS];
    const float *dec_gamma[GEOADV_ATLAS_MAX_DEC_LAYERS], *dec_beta[GEOADV_ATLAS_MAX_DEC_LAYERS];
    const float *dec_mean[GEOADV_ATLAS_MAX_DEC_LAYERS], *dec_var[GEOADV_ATLAS_MAX_DEC_LAYERS];
} geoadv_atlas_weights;

/* Uploads the HOST weights and the HOST template points host_template[nb_primitives, points_per_primitive, dim_template]
 * (batch norm folded into a per-channel scale / shift, the per-point layers packed for MFMA).  Allocates device memory;
 * synchronous.  The handle is immutable afterwards.  Unsupported configurations return GEOADV_EINVAL. */
int  geoadv_atlas_create(geoadv_atlas **out, const geoadv_atlas_config *config, const geoadv_atlas_weights *host_weights,
                         const float *host_template);
void geoadv_atlas_destroy(geoadv_atlas *atlas);
/* Device scratch of geoadv_atlas_forward for a batch of b clouds of n points. */
size_t geoadv_atlas_workspace_bytes(const geoadv_atlas *atlas, int b, int n);
/* EncoderDecoder.forward(x, train=False) followed by fuse_primitives (training/trainer_loss.py:36-45): pc[b,n,3] ->
 * recon[b, nb_primitives * points_per_primitive, 3], primitive-major; latent[b,1024] (may be NULL) returns the encoder's
 * output.  1 <= n <= 16384, b >= 1, else GEOADV_EINVAL.  A cloud's results do not depend on b, on its position in the
 * batch or on the order of its points; a cloud with non-finite coordinates affects no other cloud. */
int geoadv_atlas_forward(const geoadv_atlas *atlas, int b, int n, const float *pc, float *latent, float *recon,
                         void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * FoldingNet auto-encoder of the transfer experiment: transfer/foldingnet/foldingnet.py (FoldingNetEnc_with_graph :57-104,
 * Graph_Pooling :14-54, FoldingNetDec :107-189) with the graph of prepare_graph.py:24-73 (16 neighbours, covariance,
 * symmetric adjacency), eval mode, batch norm from the running statistics with eps 1e-5, fp32.  csrc/foldingnet.hip.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_fold geoadv_fold;

#define GEOADV_FOLD_ENC_LAYERS  7   /* conv1 12->64, conv2 64->64, conv3 64->64, conv4 64->128, conv5 128->1024, fc1 1024->512
                                       (batch norms bn1 .. bn6), fc2 512->512 (no batch norm)                                 */
#define GEOADV_FOLD_DEC_LAYERS  6   /* fold1.conv1 514->512, fold1.conv2 512->512, fold1.conv3 512->3, the same for fold2 (515) */
#define GEOADV_FOLD_PICKS_GIVEN  0  /* the 16 neighbour positions of every point and pool layer come from the caller           */
#define GEOADV_FOLD_PICKS_DEVICE 1  /* drawn on the device from (seed, cloud ordinal, pool layer, point): csrc/foldingnet.hip   */
/* Every w is [fan_in, fan_out] row-major (torch's weight [out, in(, 1)] transposed), b is [fan_out].  The first 512 rows of
 * a fold's conv1 act on the code, the last 2 (fold1: grid x, y) or 3 (fold2: p1) on the point.  fc2's batch-norm pointers
 * must be NULL, all others given. */
typedef struct geoadv_fold_weights {
    const float *enc_w[GEOADV_FOLD_ENC_LAYERS], *enc_b[GEOADV_FOLD_ENC_LAYERS];
    const float *enc_gamma[GEOADV_FOLD_ENC_LAYERS], *enc_beta[GEOADV_FOLD_ENC_LAYERS];
    const float *enc_mean[GEOADV_FOLD_ENC_LAYERS], *enc_var[GEOADV_FOLD_ENC_LAYERS];
    const float *dec_w[GEOADV_FOLD_DEC_LAYERS], *dec_b[GEOADV_FOLD_DEC_LAYERS];
} geoadv_fold_weights;

/* Uploads the HOST weights (batch norm folded, the per-point layers packed for MFMA).  Allocates device memory;
 * synchronous.  The handle is immutable afterwards. */
int  geoadv_fold_create(geoadv_fold **out, const geoadv_fold_weights *host_weights);
void geoadv_fold_destroy(geoadv_fold *fold);
/* Device scratch of geoadv_fold_graph / geoadv_fold_forward for a batch of b clouds of n points. */
size_t geoadv_fold_workspace_bytes(const geoadv_fold *fold, int b, int n);
/* build_graph (prepare_graph.py:45-104) of pc[b,n,3]: degree[b,n] (the symmetric adjacency's row lengths, >= 16),
 * knn[b,n,16] (the 17 nearest neighbours by squared distance, the existing kNN kernel's order and tie rule, column 0
 * dropped) and cov[b,n,9] (np.cov of those 16 neighbours, ddof 1, row-major 3x3).  Any output may be NULL.
 * 17 <= n <= 16384, b >= 1, else GEOADV_EINVAL. */
int geoadv_fold_graph(const geoadv_fold *fold, int b, int n, const float *pc, int *degree, int *knn, float *cov,
                      void *workspace, void *stream);
/* FoldingNet_graph.forward of pc[b,n,3] (the graph is rebuilt here).  picks[2,b,n,16] are positions in each point's
 * sorted adjacency row, pool layer major: read with GEOADV_FOLD_PICKS_GIVEN (required; a position outside [0, degree)
 * is clamped into the row, never read outside it), written with GEOADV_FOLD_PICKS_DEVICE (may be NULL), where cloud k of
 * the batch draws with ordinal cloud_offset + k.  cols[2,b,n,16] returns the neighbour indices the picks resolve to,
 * code[b,512] the encoder's output, p1[b,2025,3] fold1's output and recon[b,2025,3] the reconstruction; each may be NULL.
 * 17 <= n <= 16384, b >= 1, cloud_offset >= 0, else GEOADV_EINVAL.  A cloud with non-finite coordinates affects no
 * other cloud. */
int geoadv_fold_forward(const geoadv_fold *fold, int b, int n, const float *pc, int sampling, unsigned long long seed,
                        long long cloud_offset, int *picks, int *cols, float *code, float *p1, float *recon,
                        void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * FoldingNet training: one step of transfer/foldingnet/train_foldingnet.py:76-117 -- FoldingNet_graph in train mode (batch
 * statistics, eps 1e-5, running statistics 0.9 / 0.1 with the unbiased variance), loss = ChamferLoss(points, recon) (batch
 * mean of mean_j min_k d + mean_k min_j d, squared distances; its gradient reaches recon only), torch.optim.Adam with
 * weight decay on every parameter.  csrc/fold_train.hip states the pool backward's rule and the optimizer exactly.  One
 * handle = one model with a fixed batch and point count; no process-wide state; a step is bitwise reproducible.  A handle
 * keeps about 12 KB of device memory per decoder row (batch * 2025) and 15 KB per point: 1.8 GB at 32 x 2048, and about
 * 27 GB at batch 1024 (with 17 ... 128 points).
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_fold_trainer geoadv_fold_trainer;
typedef struct geoadv_fold_train_config {
    int   batch;            /* 2 ... 1024 (bn6 takes its statistics over the clouds of the batch), batch * n_points <= 2^17 */
    int   n_points;         /* 17 ... 16384, as geoadv_fold_forward                               */
    float learning_rate;    /* 1e-4                                                                */
    float weight_decay;     /* 1e-6, added to the gradient of every parameter                      */
    long long seed;         /* key of the device neighbour sampler (taken modulo 2^64)             */
    long long initial_step; /* optimizer steps taken so far (0, or a restored value)               */
    long long initial_ordinal; /* clouds seen so far: the device sampler's next cloud ordinal      */
} geoadv_fold_train_config;
/* init: HOST values of every parameter (mean / var = the running statistics), in geoadv_fold_weights' layout.  Adam's
 * slots start at zero; geoadv_fold_trainer_set_slots restores exp_avg / exp_avg_sq (flat, in the parameter layout). */
int  geoadv_fold_trainer_create(geoadv_fold_trainer **out, const geoadv_fold_weights *init, const geoadv_fold_train_config *cfg);
void geoadv_fold_trainer_destroy(geoadv_fold_trainer *t);
/* set_slots takes no stream: a synchronous copy from HOST memory (hipMemcpy), complete on return.  It does not wait for a step in
 * flight: the caller must have synchronised every stream on which a step of this handle was queued. */
int  geoadv_fold_trainer_set_slots(geoadv_fold_trainer *t, const float *slot1, const float *slot2);
/* x: device [batch][n][3].  sampling / picks (device int32 [2][batch][n][16]) as geoadv_fold_forward: read with
 * GEOADV_FOLD_PICKS_GIVEN, written (may be NULL) with GEOADV_FOLD_PICKS_DEVICE, where cloud k draws with ordinal
 * (clouds seen so far) + k.  loss / mid_loss (device floats, of the PRE-update parameters: ChamferLoss against recon and
 * against fold1's output) may be NULL.  Updates the parameters, slots, running statistics, step and ordinal counters. */
int geoadv_fold_trainer_step(geoadv_fold_trainer *t, const float *x, int sampling, int *picks, float *loss, float *mid_loss,
                             void *stream);
/* Device pointers of the flat parameter / gradient buffers (`count` floats each); offsets52[4 l + f] = where layer l's
 * weights [in][out] (f 0), biases (1), BN weight (2), BN bias (3) sit ((size_t)-1: none), layers in the order conv1 .. conv5,
 * fc1, fc2, fold1.conv1 .. 3, fold2.conv1 .. 3; moving_offsets13[l] = where its statistics sit in the BN arenas (may be NULL). */
int geoadv_fold_trainer_buffers(geoadv_fold_trainer *t, float **params, float **grads, size_t *count);
int geoadv_fold_trainer_layout(const geoadv_fold_trainer *t, size_t *offsets52, size_t *moving_offsets13);
int geoadv_fold_trainer_counters(const geoadv_fold_trainer *t, long long *step, long long *ordinal);
/* Read-only TEST / export view of what the last step kept: *ptr and its element count.
 *   BN_MEAN / BN_VAR / RUNNING_MEAN / RUNNING_VAR / BN_INV / BN_SHIFT  float [C_layer], layer 0 .. 5 (bn1 .. bn6): the batch's
 *                  mean and biased variance, the running statistics, the folded constants (the step's BN output is
 *                  a * inv + shift, two fp32 roundings)
 *   PRE_BN         float [rows][C_layer]   the stored pre-BN activation; rows = batch * n (layers 0 .. 4) or batch (5)
 *   POOL_WINNER    int [batch * n][64 | 128]  pool 0 / 1: the row (in its cloud) whose value each (point, channel) took, -1
 *                  where the maximum is not positive
 *   GMAX_ROW       int [batch][1024]       the first maximal row of bn5's output
 *   HIDDEN         float [batch * 2025][512]  the ReLU outputs of fold1.conv1, fold1.conv2, fold2.conv1, fold2.conv2 (0 .. 3)
 *   PICKS / COLS   int [2][batch][n][16]; COV float [batch][n][9]; CODE [batch][512]; MID / RECON [batch][2025][3]
 *   CHAMFER_IDX    int: 0 = nearest recon point of every input point [batch][n], 1 = nearest input point [batch][2025]
 *   SLOT1 / SLOT2  float [count]           Adam's exp_avg / exp_avg_sq in the parameter layout */
#define GEOADV_FOLD_STATE_BN_MEAN       0
#define GEOADV_FOLD_STATE_BN_VAR        1
#define GEOADV_FOLD_STATE_RUNNING_MEAN  2
#define GEOADV_FOLD_STATE_RUNNING_VAR   3
#define GEOADV_FOLD_STATE_BN_INV        4
#define GEOADV_FOLD_STATE_BN_SHIFT      5
#define GEOADV_FOLD_STATE_PRE_BN        6
#define GEOADV_FOLD_STATE_POOL_WINNER   7
#define GEOADV_FOLD_STATE_GMAX_ROW      8
#define GEOADV_FOLD_STATE_HIDDEN        9
#define GEOADV_FOLD_STATE_PICKS        10
#define GEOADV_FOLD_STATE_COLS         11
#define GEOADV_FOLD_STATE_COV          12
#define GEOADV_FOLD_STATE_CODE         13
#define GEOADV_FOLD_STATE_MID          14
#define GEOADV_FOLD_STATE_RECON        15
#define GEOADV_FOLD_STATE_CHAMFER_IDX  16
#define GEOADV_FOLD_STATE_SLOT1        17
#define GEOADV_FOLD_STATE_SLOT2        18
int geoadv_fold_trainer_state(const geoadv_fold_trainer *t, int what, int layer, const void **ptr, size_t *count);

/* TESTS / TOOLS: three kernels of the FoldingNet training step on caller-supplied DEVICE buffers, each through the launch the step
 * itself uses (csrc/fold_train.hip).  b in 1 ... 1024, n >= 1, b * n <= 2^17, c in 1 ... 65536; no pointer may be NULL.
 * pool: the graph pool and its ReLU.  h [b n][c]; cols [b n][16] rows of the point's own cloud, each in [0, n).
 *   g [b n][c] = the maximum over (the point itself, its 16 columns) where that is positive, else +0; win [b n][c] = the row that
 *   attained it -- the point itself first, then the lowest slot -- or -1.
 * pool_grad: the pool's backward, gathered by destination.  dg, win as above; off / deg [b n] and col [b][32 n]: the sorted row of
 *   point i of cloud k is col[k * 32 n + off[k n + i] ...], deg[k n + i] entries (csrc/fold_graph.h), which must hold every i' != i
 *   with win[i'][.] == i.  dh [b n][c] = [win[i] == i] dg[i] + the dg[i'] of those i', added in the row's order.
 * gmax: pooled [b][c] = the maximum over the n rows of each cloud of a * inv + shift (a [b n][c]; inv, shift [c]; two rounded
 *   operations), arg [b][c] = its first row. */
int geoadv_fold_train_pool(int b, int n, int c, const float *h, const int *cols, float *g, int *win, void *stream);
int geoadv_fold_train_pool_grad(int b, int n, int c, const float *dg, const int *win, const int *off, const int *deg, const int *col,
                                float *dh, void *stream);
int geoadv_fold_train_gmax(int b, int n, int c, const float *a, const float *inv, const float *shift, float *pooled, int *arg,
                           void *stream);

/* ------------------------------------------------------------------------------------------
 * AtlasNet training: one step of transfer/atlasnet/training/trainer.py's train_iteration for the point-cloud
 * auto-encoder -- EncoderDecoder.forward(x, train=True) (batch statistics, eps 1e-5, running statistics 0.9 / 0.1 with the
 * unbiased variance; template points uniform in [0, 1)^2, one draw per primitive shared by the batch), fuse_primitives,
 * loss = mean(dist1) + mean(dist2) over the whole batch (squared distances; the gradient reaches the reconstruction only),
 * torch.optim.Adam without weight decay.  csrc/atlas_train.hip states the template generator and the optimizer exactly.
 * One handle = one model with a fixed batch, point count and template size; no process-wide state; a step is bitwise
 * reproducible.  A handle keeps about (14 + 4 num_layers) KB of device memory per decoder row
 * (nb_primitives * batch * points_per_primitive) and 6 KB per input point: 2.3 GB at 32 x 2048 with 25 x 100, num_layers 2.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_atlas_trainer geoadv_atlas_trainer;
typedef struct geoadv_atlas_train_config {
    int   batch;                  /* 2 ... 1024 (bn4 / bn5 take their statistics over the clouds of the batch)            */
    int   n_points;               /* 1 ... 16384, batch * n_points <= 2^17                                                */
    int   points_per_primitive;   /* template points per primitive in TRAIN mode (number_points / nb_primitives), >= 1;
                                     nb_primitives * batch * points_per_primitive <= 2^18 and
                                     nb_primitives * points_per_primitive <= 16384                                        */
    float learning_rate;          /* 1e-3                                                                                  */
    long long seed;               /* key of the device template generator (taken modulo 2^64)                             */
    long long initial_step;       /* Adam steps taken so far by the CURRENT optimizer (0, or a restored value)            */
    long long initial_tracked;    /* training steps the model has taken in all (num_batches_tracked): the generator's counter */
} geoadv_atlas_train_config;
/* config: as geoadv_atlas_create (points_per_primitive there is ignored here: the train config's holds).  init: HOST values
 * of every parameter (mean / var = the running statistics).  Adam's slots start at zero; set_slots restores exp_avg /
 * exp_avg_sq (flat, in the parameter layout).  Sizes the handle cannot hold return GEOADV_EINVAL here, never later. */
int  geoadv_atlas_trainer_create(geoadv_atlas_trainer **out, const geoadv_atlas_config *config, const geoadv_atlas_weights *init,
                                 const geoadv_atlas_train_config *cfg);
void geoadv_atlas_trainer_destroy(geoadv_atlas_trainer *t);
/* set_slots takes no stream: a synchronous copy from HOST memory (hipMemcpy), complete on return.  It does not wait for a step in
 * flight: the caller must have synchronised every stream on which a step of this handle was queued. */
int  geoadv_atlas_trainer_set_slots(geoadv_atlas_trainer *t, const float *slot1, const float *slot2);
/* The reference builds a NEW Adam with lrate / 10 at its decay epochs: reset_optimizer != 0 zeroes both slots and the
 * Adam step count as well (num_batches_tracked goes on).  No stream: with reset_optimizer the call synchronises the DEVICE (every
 * step in flight on any stream finishes first), clears the slots and returns once the clear is complete, so the caller has
 * nothing to synchronise; without it only host state changes, which the next step reads when it is queued. */
int  geoadv_atlas_trainer_set_learning_rate(geoadv_atlas_trainer *t, float learning_rate, int reset_optimizer);
/* x: device [batch][n_points][3].  template_points: device [nb_primitives][points_per_primitive][2], read if
 * given_template != 0, else written with the step's draw (may then be NULL).  loss (a device float, of the PRE-update
 * parameters) may be NULL.  Updates the parameters, slots, running statistics and both counters. */
int geoadv_atlas_trainer_step(geoadv_atlas_trainer *t, const float *x, int given_template, float *template_points, float *loss,
                              void *stream);
/* Device pointers of the flat parameter / gradient buffers (`count` floats each); offsets[4 l + f] = where layer l's
 * weights [in][out] (f 0), biases (1), BN weight (2), BN bias (3) sit ((size_t)-1: none); layers 0 .. 4 = the encoder's
 * conv1, conv2, conv3, lin1, lin2, then the decoder's conv1, conv2, conv_list[0 .. num_layers), last_conv (8 + num_layers
 * layers in all; offsets holds 4 * 12 entries).  A decoder entry is primitive 0's; primitive p follows at p * (size of one
 * primitive's array).  moving_offsets[l] (12 entries, may be NULL) = where the layer's statistics sit in the BN arenas. */
int geoadv_atlas_trainer_buffers(geoadv_atlas_trainer *t, float **params, float **grads, size_t *count);
int geoadv_atlas_trainer_layout(const geoadv_atlas_trainer *t, size_t *offsets48, size_t *moving_offsets12);
int geoadv_atlas_trainer_counters(const geoadv_atlas_trainer *t, long long *step, long long *tracked);
/* Read-only TEST / export view of what the last step kept: *ptr and its element count.  A decoder layer's arrays hold all
 * primitives, primitive-major; rows of a primitive are (cloud, template point), cloud-major.
 *   BN_MEAN / BN_VAR / RUNNING_MEAN / RUNNING_VAR / BN_INV / BN_SHIFT  float [C] (encoder) or [nb][C] (decoder) of a layer
 *                  with batch norm: the batch's mean and biased variance, the running statistics, the folded constants (the
 *                  step's BN output is a * inv + shift, two fp32 roundings).  A decoder without batch norm has inv 1, shift 0.
 *   PRE_BN         float: the stored pre-BN activation: [batch * n][C] (layers 0 .. 2), [batch][1024] (3, 4),
 *                  [nb][batch * p][512] (6 ...).  Layer 5 (the decoder's conv1) returns t1 = conv1(template) [nb][p][1024]:
 *                  its pre-BN activation is t1[j] + latent[b] and is never stored.
 *   GMAX_ROW       int [batch][1024]   the first maximal row of bn3's output
 *   TEMPLATE       float [nb][p][2]; LATENT [batch][1024]; RECON [batch][nb * p][3]
 *   CHAMFER_IDX    int: 0 = nearest recon point of every input point [batch][n], 1 = nearest input point [batch][nb * p]
 *   SLOT1 / SLOT2  float [count]       Adam's exp_avg / exp_avg_sq in the parameter layout */
#define GEOADV_ATLAS_STATE_BN_MEAN       0
#define GEOADV_ATLAS_STATE_BN_VAR        1
#define GEOADV_ATLAS_STATE_RUNNING_MEAN  2
#define GEOADV_ATLAS_STATE_RUNNING_VAR   3
#define GEOADV_ATLAS_STATE_BN_INV        4
#define GEOADV_ATLAS_STATE_BN_SHIFT      5
#define GEOADV_ATLAS_STATE_PRE_BN        6
#define GEOADV_ATLAS_STATE_GMAX_ROW      7
#define GEOADV_ATLAS_STATE_TEMPLATE      8
#define GEOADV_ATLAS_STATE_LATENT        9
#define GEOADV_ATLAS_STATE_RECON        10
#define GEOADV_ATLAS_STATE_CHAMFER_IDX  11
#define GEOADV_ATLAS_STATE_SLOT1        12
#define GEOADV_ATLAS_STATE_SLOT2        13
int geoadv_atlas_trainer_state(const geoadv_atlas_trainer *t, int what, int layer, const void **ptr, size_t *count);

/* TESTS / TOOLS: one fp32 GEMM of the training steps on caller-supplied DEVICE buffers, through the launch the trainers use.
 *   C[z][i * ldc + j] = sum_k A[z * sAz + i * sAi + k * sAk] * B[z * sBz + k * sBk + j * sBj] + bias[z * sBiasZ + j]
 * for z < batch, i < M, j < N, k < K (strides in floats; bias may be NULL).
 * kernel 0: the 64-tile kernel with its fixed-order split-K (csrc/train_tile.h); the split follows from the shape alone and is
 *   written to *ksplit_out (may be NULL).  It has ONE bias for all groups: sBiasZ != 0 with batch > 1 returns GEOADV_EINVAL.
 *   partials: device scratch of at least geoadv_train_gemm_partial_floats() floats (partial_floats = its size).
 * kernel 1: the batched 128-tile kernel of the AtlasNet step (csrc/atlas_train.hip); partials is not used, *ksplit_out = 1.
 * M, N in 1 ... 2^20, K >= 1, batch in 1 ... 1024, ldc >= N. */
size_t geoadv_train_gemm_partial_floats(void);
int geoadv_train_gemm(int kernel, const float *A, long long sAi, long long sAk, long long sAz, const float *B, long long sBk,
                      long long sBj, long long sBz, float *C, long long ldc, long long sCz, const float *bias, long long sBiasZ,
                      int M, int N, int K, int batch, float *partials, size_t partial_floats, int *ksplit_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * The attack loop: AdvAE (src/adv_ae.py:30-251) + Adversary (src/adversary.py:9-57).
 * One handle = one batch slot of `batch` clouds with device-resident state
 * (pert, Adam m/v/beta powers, best-so-far outputs).
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_attack geoadv_attack;

#define GEOADV_LOSS_ADV_CHAMFER 0   /* loss_adv_type 'chamfer' (output space), adv_ae.py:88   */
#define GEOADV_LOSS_ADV_LATENT  1   /* loss_adv_type 'latent',  adv_ae.py:85-86,107-116      */
#define GEOADV_LOSS_DIST_CHAMFER 0  /* loss_dist_type 'chamfer', adv_ae.py:98-102            */
#define GEOADV_LOSS_DIST_PERT    1  /* loss_dist_type 'pert',    adv_ae.py:93-97             */

typedef struct geoadv_attack_config {
    int   batch;                    /* conf.batch_size                                        */
    int   loss_adv_type;            /* GEOADV_LOSS_ADV_*                                      */
    int   loss_dist_type;           /* GEOADV_LOSS_DIST_*                                     */
    float max_point_pert_weight;    /* conf.max_point_pert_weight (adv_ae.py:94-95)           */
    float max_point_dist_weight;    /* conf.max_point_dist_weight (adv_ae.py:99-100)          */
    float learning_rate;            /* conf.learning_rate (adv_ae.py:146,152)                 */
    float emd_weight;               /* build-defined: loss_adv += emd_weight*match_cost/N; 0 = off */
    int   all_pairs_source_dist;    /* 0 (default): nn_distance(adv, x) by the exact paired grid search, falling back per
                                     * cloud to the all-pairs kernel, except for tiny batches -- batch * n_points < 10240, i.e.
                                     * up to 4 clouds of 2048 points (GEOADV_SMALL_BATCH_POINTS) -- where the all-pairs kernel alone
                                     * is as fast; 1: always the all-pairs kernel; 2: the grid search at every size.  Same results. */
    int   emd_weight_mode;          /* GEOADV_EMD_FAST (0, default) or GEOADV_EMD_REFERENCE for the EMD term's plan,
                                     * optionally | GEOADV_EMD_DENSE_LEVELS (this handle's EMD sweeps all dense)            */
    /* Alternative code paths with the same results, selected explicitly (never by the environment); all 0 = defaults.
     * The parity tests run every one of them against the default path.                                                */
    int   recompute_backward;       /* 1: the sparse encoder backward re-runs the forward for the critical rows instead
                                     * of reading the ReLU masks the forward kept (the path tied clouds always take)    */
    int   encoder_backward;         /* how the masks are used: GEOADV_ENC_BWD_AUTO (0) = the pool Jacobian (encoder_jac.h) where
                                     * it can be evaluated beside the symmetric Chamfer scan, else the masked backward;
                                     * _MASKED (1) = always back-propagate dz through the critical rows; _JACOBIAN (2) = always
                                     * the Jacobian (a launch of its own where nothing hosts it).  Equal to rounding.       */
    int   separate_adam;            /* 1: the Adam step is its own launch (the path loss_dist_type 'pert' always takes)
                                     * instead of riding in the next forward's point loaders                           */
    int   chamfer_kernel;           /* GEOADV_CHAMFER_AUTO (0: by batch size, GEOADV_SYM_MIN_POINTS), _TWO_SCAN (the public op's kernel),
                                     * _SYMMETRIC (one evaluation per pair serves both directions)                      */
    int   recon_lists;              /* nn_distance(recon, target) between two all-pairs scans from exact neighbour lists (csrc/chamfer_lists.h):
                                     * GEOADV_RECON_LISTS_ADAPTIVE (0, default) = on from the 49th forward after set_inputs / init_pert (Adam's
                                     * first steps move the reconstruction fastest; those forwards scan), switched off for the rest of a batch when the scan
                                     * has to take most clouds back (a victim whose reconstructions jump past the skin) and on again by
                                     * set_inputs; _OFF (1) = every forward scans; _PINNED (2) = on from the first forward, no policy.  Used by the output-space
                                     * attack on clouds of up to 2048 points under the symmetric scan with the paired search in use, without the EMD term; every other
                                     * configuration scans as before.  Same results, bit for bit.  Per handle. */
    /* The kNN outlier term: the defense-aware (adaptive) attack.  With knn_weight != 0 the loop minimises, per cloud b,
     *   loss_adv + dist_weight[b] * (loss_dist + knn_weight * K(adv))
     * K and dK/dadv EXACTLY the rule of geoadv_knn_outlier_loss above with k = knn_k and alpha = (double)knn_alpha (search knn_point(k + 1),
     * SOR statistics in float64, mask held constant, float64 accumulation in the stated order, one rounding to fp32), applied to the
     * fp32 cloud adv = x + pert of the cached forward -- the cloud the step's backward kernels read.  It enters the step as
     *   g_dist[b,i] <- fadd_rn(g_dist[b,i], fmul_rn(dist_weight[b], fmul_rn(knn_weight, dK[b,i])))
     * both products and the sum each rounded to fp32, no contraction: the loop's Chamfer gradient g_dist already carries
     * dist_weight[b] when it is formed (Adam adds g_dist as it stands), so the term takes the same factor here.  This happens in
     * the step after g_dist exists -- from the forward's loss launch or from the step's own gradient launch, max-point branch
     * included -- and before the decoder / encoder backward and the Adam step, whether Adam is its own launch or rides in the next
     * forward's loaders.  Two launches more per iteration (the search, and a second instance of the op's gradient launch that adds
     * in place and writes nothing else), on the run's stream, counted under GEOADV_PROF_LOSS_GRAD; their workspace
     * (geoadv_knn_outlier_loss_workspace_bytes(batch, n, knn_k)) and a double[batch] for K are part of the handle's arena.
     * The history rows of geoadv_attack_run, geoadv_attack_get_best and its keep-best rule, geoadv_attack_peek and the TESTS ONLY
     * read-outs are unchanged and do not contain K.
     * geoadv_attack_create returns GEOADV_EINVAL (nothing allocated) for knn_weight != 0 with: knn_weight not finite;
     * loss_dist_type GEOADV_LOSS_DIST_PERT (that path has no g_dist); knn_k outside 1 ... 15; knn_alpha negative or not finite;
     * n < knn_k + 2 or n > 16384; batch > 65535.
     * knn_rule = 1 swaps the rule for the SURFACE rule of geoadv_knn_outlier_loss (GEOADV_KNN_LOSS_SURFACE) with k = knn_k and
     * thr = knn_thresh: the mask is the set geoadv_outlier_filter removes, K the hinge on it -- the attack aware of the paper's own
     * off-surface defense.  Same launches, same place in the step, same three fp32 roundings into g_dist, same arena.  knn_alpha
     * is then not read; with knn_weight = 0 neither member below is read; knn_rule = 0 is the handle described above, bit for bit.
     * Further refusals with knn_weight != 0: a knn_rule other than 0 / 1; under rule 1 knn_k > 7 and a negative or non-finite
     * knn_thresh.  (The two members stand before knn_weight: tests hold knn_weight / knn_k / knn_alpha / loss_in_scan to the
     * struct's last four places.) */
    int    knn_rule;                /* 0 (default) = the SOR rule, 1 = the surface rule                                         */
    float  knn_thresh;              /* read only under knn_rule 1: >= 0, finite                                                 */
    float  knn_weight;              /* 0 (default) = off: none of knn_rule, knn_thresh, knn_k, knn_alpha is read, nothing is reserved
                                     * or launched -- arena, launches and every output bit are those of a handle without them */
    int    knn_k;                   /* 1 ... 15                                                                                */
    float  knn_alpha;               /* >= 0, finite; the op's alpha is (double)knn_alpha                                    */
    /* (The three members above stand before loss_in_scan, which stays the struct's last member, and are all int / float: callers
     * that fill the struct by name, or zero it and set what they need, are not affected by their position.)                  */
    int   loss_in_scan;             /* 0 (default): the loss / metrics / keep-best and Chamfer-gradient workgroups ride as the last
                                     * workgroups of the symmetric scan's launch where that pays and it can host them (the paired
                                     * search in the launch and two scan workgroups per CU: batch >= 64 at 2048 points; both losses Chamfer, no EMD
                                     * term, batch a multiple of 8, one row super-tile, and a device that deals workgroup i to XCD
                                     * i % 8: checked once per handle) -- they wait for their cloud's workgroups through a counter
                                     * instead of a kernel boundary; 1: always a launch of their own; 2: riding wherever the launch CAN
                                     * host them, paying or not (the parity tests).  Same results, bit for bit. */
} geoadv_attack_config;
#define GEOADV_SMALL_BATCH_POINTS 10240  /* batch * n_points below this: no paired grid search (all_pairs_source_dist = 0)                    */
#define GEOADV_SYM_MIN_POINTS      4096  /* batch * n_points from this on: chamfer_kernel AUTO = the symmetric scan, and with it
                                          * encoder_backward AUTO = the pool Jacobian (it rides in that scan's launch); below: the two-scan
                                          * kernel and the masked backward                                                               */
#define GEOADV_ENC_BWD_AUTO      0
#define GEOADV_ENC_BWD_MASKED    1
#define GEOADV_ENC_BWD_JACOBIAN  2
#define GEOADV_CHAMFER_AUTO      0
#define GEOADV_CHAMFER_TWO_SCAN  1
#define GEOADV_CHAMFER_SYMMETRIC 2
#define GEOADV_RECON_LISTS_ADAPTIVE 0
#define GEOADV_RECON_LISTS_OFF      1
#define GEOADV_RECON_LISTS_PINNED   2

/* Allocates device memory; synchronous.  Its own device work -- the arena's zero fill and, for the symmetric scan, a probe launch of
 * how the device deals workgroups to its XCDs, which writes the handle's own scratch -- runs on the null stream and is complete
 * on return; the caller has nothing to synchronise, and no stream of the caller's is waited for. */
int  geoadv_attack_create(geoadv_attack **out, const geoadv_ae *ae, const geoadv_attack_config *cfg);
void geoadv_attack_destroy(geoadv_attack *at);

/* feed_dict of adv_ae.py:202,213: x = source_pc[B,N,3], gt = target_pc[B,N,3],
 * target_z = target_latent[B,bneck], dist_weight[B].  Device pointers, copied into the handle. */
int geoadv_attack_set_inputs(geoadv_attack *at, const float *source_pc, const float *target_pc,
                             const float *target_latent, const float *dist_weight, void *stream);
/* Adversary.init_pert (adversary.py:27-28): pert <- init[B,N,3] (device).  Also resets the
 * best-so-far bookkeeping of _attack_one_batch (adv_ae.py:197-200).  The Adam slots and beta
 * powers are NOT reset (they are never re-initialised in the reference, adv_ae.py:74) unless
 * reset_optimizer != 0. */
int geoadv_attack_init_pert(geoadv_attack *at, const float *init_pert, int reset_optimizer, void *stream);

/* Runs `iterations` iterations of the hot loop (adv_ae.py:216-246): each is one Adam step on
 * pert followed by the evaluation of the per-cloud metrics of the UPDATED pert; iterations whose
 * 1-based global index is >= thresh take part in the keep-best update (strict '<' on the target
 * reconstruction error).  Everything stays on the device; nothing is synchronised.
 * `first_iteration` is the 0-based index of the first iteration of this call within the current
 * dist-weight run (so a 500-iteration attack may be issued as several calls).
 * metrics_hist: optional device buffer [iterations, 6, B] receiving, per iteration,
 *   loss_adv, loss_dist, loss_pert, loss_max (or max_dist), input_dist, loss_ae  (adv_ae.py:219-221). */
int geoadv_attack_run(geoadv_attack *at, int first_iteration, int iterations, int thresh,
                      float *metrics_hist, void *stream);

/* Results of the keep-best bookkeeping (adv_ae.py:238-249), device -> caller device buffers:
 * metrics[B,5] = loss_adv, loss_dist, source_chamfer_dist, target_nre, target_recon_error
 * (target_nre = target_recon_error / target_ae_loss_ref[b]), adv[B,N,3], recon[B,N,3]. */
int geoadv_attack_get_best(geoadv_attack *at, const float *target_ae_loss_ref,
                           float *metrics, float *adv, float *recon, void *stream);

/* From the next forward on: on != 0 -- nn_distance(adv, x) through the paired grid search (where the handle's size supports it);
 * 0 -- the all-pairs kernel for every cloud.  Same results either way; a caller that sees most clouds handed back
 * (geoadv_attack_search_state: a victim whose perturbations leave the grid cells) switches the search off and saves its cost.
 * Overrides geoadv_attack_config.all_pairs_source_dist, including its small-batch rule. */
int geoadv_attack_set_source_search(geoadv_attack *at, int on);

/* Health of the run since the last set_inputs / init_pert: synchronises the stream and returns GEOADV_EHIP (message in
 * geoadv_last_error) if an in-launch hand-off of the loop ever gave up waiting -- the bounded spin of the dense encoder backward
 * on its cloud's decoder-tail flag; never observed, but a run after it would have used a stale gradient.  geoadv_attack_get_best
 * additionally NaN-fills the metrics of such a run.  Also GEOADV_ERANGE if the victim's F16X2 range guard tripped (geoadv_ae_status).
 * Callers that synchronise anyway (to download results) call this first. */
int geoadv_attack_status(geoadv_attack *at, void *stream);

/* Introspection for tests: copies of the current device state (any pointer may be NULL).
 * pert/adv/recon/grad [B,N,3]; latent [B,bneck]; idx_* [B,N] of the last forward:
 * idx_r1/idx_r2 = nn_distance(recon, gt) indices, idx_a1/idx_a2 = nn_distance(adv, x) indices. */
int geoadv_attack_peek(geoadv_attack *at, float *pert, float *adv, float *recon, float *latent,
                       float *grad, int *idx_r1, int *idx_r2, int *idx_a1, int *idx_a2, void *stream);

/* TESTS ONLY.  The loss / Chamfer-gradient launch of the loop reads the symmetric scan's row minima in the cheapest form the shape
 * admits; `form` selects, from the next forward on, the forms it replaced -- bit 0: packed (distance, index) words only from 9
 * column slices on (8 slices leave as one partial per slice), bit 1: the general multi-pass gradient body at every size and the
 * packed words folded through LDS.  0 = the default.  Same results, bit for bit. */
int geoadv_attack_test_loss_form(geoadv_attack *at, int form);
/* TESTS ONLY.  Copies of what the cached forward's loss launch left (any pointer may be NULL): the Chamfer gradients g_recon / g_dist
 * [B,N,3] w.r.t. the reconstruction and the adversarial cloud, losses [8,B] (loss_adv, loss_dist, loss_pert, loss_max | max_dist,
 * input_dist, loss_ae, loss_max(pert), max_dist), and the row minima dist_r1 / dist_a1 [B,N] of nn_distance(recon, gt) / (adv, x). */
int geoadv_attack_test_loss_state(geoadv_attack *at, float *g_recon, float *g_dist, float *losses, float *dist_r1, float *dist_a1,
                                  void *stream);
/* TESTS ONLY.  What the cached forward launched (it is run first if there is none), so that a test can assert the form it was written
 * for; plan[GEOADV_PLAN_*] (host memory, GEOADV_PLAN_COUNT entries).  jstar (device, [2,B], or NULL): the arg-max points that forward's loss row found -- first
 * arg-max of the (adv -> source) distances, first arg-max of |pert|^2 -- which the max-point terms of the step use. */
enum {
    GEOADV_PLAN_SYMMETRIC = 0,   /* 1: the symmetric scan, 0: the two-scan kernel (rows always final, the next four entries 0) */
    GEOADV_PLAN_SCREENED = 1,    /* 1: the matrix-pipe-screened scan kernel, 0: the plain one */
    GEOADV_PLAN_RTILES = 2,      /* row super-tiles of the scan's launch shape */
    GEOADV_PLAN_RSLICES = 3,     /* row partials per row (column slices x column waves) */
    GEOADV_PLAN_ROWS = 4,        /* how the row minima left the scan: GEOADV_PLAN_ROWS_* */
    GEOADV_PLAN_LOSS = 5,        /* which loss row ran: GEOADV_PLAN_LOSS_* */
    GEOADV_PLAN_GRAD = 6,        /* which Chamfer gradient ran or is left to the step: GEOADV_PLAN_GRAD_* */
    GEOADV_PLAN_H = 7,           /* parts per (cloud, problem) of the fixed-point gradient body (0 where none runs) */
    GEOADV_PLAN_RANGE = 8,       /* receiving points per part: part h owns the points [h * range, (h + 1) * range) (0 where none runs) */
    GEOADV_PLAN_COUNT = 9
};
enum { GEOADV_PLAN_ROWS_FINAL = 0, GEOADV_PLAN_ROWS_PARTIALS = 1, GEOADV_PLAN_ROWS_PACKED = 2, GEOADV_PLAN_ROWS_MERGE_LAUNCH = 3 };
enum { GEOADV_PLAN_LOSS_METRICS = 0, GEOADV_PLAN_LOSS_FUSED = 1, GEOADV_PLAN_LOSS_RIDERS = 2 };
enum { GEOADV_PLAN_GRAD_NONE = 0, GEOADV_PLAN_GRAD_FUSED_1PASS = 1, GEOADV_PLAN_GRAD_FUSED_GENERAL = 2, GEOADV_PLAN_GRAD_STEP_FX_1PASS = 3,
       GEOADV_PLAN_GRAD_STEP_FX_GENERAL = 4, GEOADV_PLAN_GRAD_STEP_SORTED = 5 };
int geoadv_attack_test_plan(geoadv_attack *at, int plan[GEOADV_PLAN_COUNT], int *jstar, void *stream);
/* TESTS ONLY, host only (no device is touched): every decision of one launch of the symmetric Chamfer scan, as the pure plan function
 * behind geoadv_nn_distance_sym, geoadv_chamfer_matrix, the training step and the attack loop's forward makes it.
 * request[GEOADV_SYM_REQ_COUNT]: problems (1 or 2), clouds, rows, columns; flags: the loop's launch rule, second pair gated, the
 * search / Jacobian / loss riders asked for (+ workgroups per cloud of the loss riders, + hosted wherever possible), the caller takes
 * deferred rows, has a packed buffer (+ the fewest partials per row that are packed); clouds of the second operand of an all-pairs
 * matrix (0: cloud c against cloud c); the screen switch.  out[GEOADV_SYM_OUT_COUNT]: screened, kernel (0 plain, 8 screened),
 * the launch shape, row partials per row, GEOADV_PLAN_ROWS_*, (first block, blocks) of the search, the scan, the Jacobian and the loss
 * riders, the grid, dynamic LDS bytes, arrivals a cloud's loss counter gains, the Jacobian riders' priority flag, scratch floats per
 * (pair, cloud) group and the offsets of the four partial arrays in floats (sizes saturate at INT_MAX). */
enum { GEOADV_SYM_REQ_NP = 0, GEOADV_SYM_REQ_B, GEOADV_SYM_REQ_N, GEOADV_SYM_REQ_M, GEOADV_SYM_REQ_LOOP, GEOADV_SYM_REQ_NEED1,
       GEOADV_SYM_REQ_SEARCH, GEOADV_SYM_REQ_JAC, GEOADV_SYM_REQ_LOSS, GEOADV_SYM_REQ_LOSS_ROWS, GEOADV_SYM_REQ_LOSS_FORCE,
       GEOADV_SYM_REQ_DEFER, GEOADV_SYM_REQ_PACKED, GEOADV_SYM_REQ_PACK_FROM, GEOADV_SYM_REQ_Q_CLOUDS, GEOADV_SYM_REQ_SCREEN,
       GEOADV_SYM_REQ_COUNT };
enum { GEOADV_SYM_OUT_SCREENED = 0, GEOADV_SYM_OUT_KERNEL, GEOADV_SYM_OUT_RW, GEOADV_SYM_OUT_CW, GEOADV_SYM_OUT_RTILES, GEOADV_SYM_OUT_C,
       GEOADV_SYM_OUT_S, GEOADV_SYM_OUT_CSLICES, GEOADV_SYM_OUT_RSLICES, GEOADV_SYM_OUT_ROWS, GEOADV_SYM_OUT_SEARCH_FIRST,
       GEOADV_SYM_OUT_SEARCH_BLOCKS, GEOADV_SYM_OUT_SCAN_FIRST, GEOADV_SYM_OUT_SCAN_BLOCKS, GEOADV_SYM_OUT_JAC_FIRST, GEOADV_SYM_OUT_JAC_BLOCKS,
       GEOADV_SYM_OUT_LOSS_FIRST, GEOADV_SYM_OUT_LOSS_BLOCKS, GEOADV_SYM_OUT_GRID, GEOADV_SYM_OUT_LDS_BYTES, GEOADV_SYM_OUT_LOSS_ARRIVALS,
       GEOADV_SYM_OUT_RAISE_PRIO, GEOADV_SYM_OUT_GROUP_FLOATS, GEOADV_SYM_OUT_ROWPART_D, GEOADV_SYM_OUT_ROWPART_I, GEOADV_SYM_OUT_COLPART_D,
       GEOADV_SYM_OUT_COLPART_I, GEOADV_SYM_OUT_COUNT };
int geoadv_debug_chamfer_sym_plan(const int *request, int *out);
/* ... and the scratch, in floats, that covers every plan of `pairs` problems of b clouds (what an attack handle reserves). */
size_t geoadv_debug_chamfer_sym_workspace_floats(int pairs, int b, int n, int m);
/* TESTS ONLY: the two fp16 pieces of the f16x2 encoder arithmetic for n pairs of values, in[2 i] and in[2 i + 1] (device memory,
 * 2 n floats): w0[i] = the packed first pieces (low half: in[2 i]), w1[i] = the packed second pieces in the form the kernels use
 * (one mixed-precision FMA per value), w1_ref[i] = the same in the plain convert-subtract-convert form (n words each, device). */
int geoadv_debug_h2_split(const float *in, int n, unsigned *w0, unsigned *w1, unsigned *w1_ref, void *stream);
/* TESTS ONLY: which form the first EMD levels took (csrc/emd.hip, "Sparse levels" -- decided on the device per cloud pair and level).
 * Reads the scratch a FINISHED geoadv_approx_match_mode (fused = 0) or geoadv_emd_cost_grad1_mode (fused != 0) call with the same
 * (b, n, m) left in `temp` (device); the call must not have carried GEOADV_EMD_DENSE_LEVELS, which leaves that scratch unwritten.
 * out[b][GEOADV_EMD_SPARSE_LEVELS][3] (host): use (1: the level's sweeps walked the cell grid), then the number of HEAVY own points
 * of cloud 1 and of cloud 2 (they took the dense form inside the sparse launch; 0 where use is 0).  All zeros where the clouds are
 * too large for any sparse scratch.  Synchronises the stream. */
#define GEOADV_EMD_SPARSE_LEVELS 3
int geoadv_debug_emd_sparse_state(int fused, int b, int n, int m, const float *temp, int *out, void *stream);

/* How nn_distance(adv, x) is being answered: *searched = 1 if the paired grid search is in use for this handle (0: all-pairs
 * kernel, by configuration or batch size), *handed_back = number of clouds of the batch whose pairing the search currently
 * judges too poor (they go through the all-pairs kernel; verdicts of the last forward).  Synchronises the stream. */
int geoadv_attack_search_state(geoadv_attack *at, int *searched, int *handed_back, void *stream);

/* From the next forward on: on != 0 -- nn_distance(recon, target) from the neighbour lists where the handle has them (the first
 * forward after it is an anchor); 0 -- the all-pairs scan in every forward; 2 ... 256 -- on, with that many forwards per anchor from
 * the next forward on (16 when the handle is created).  Same results either way. */
int geoadv_attack_set_recon_lists(geoadv_attack *at, int on);
/* How nn_distance(recon, target) has been answered since the handle was created (host memory; synchronises the stream):
 * state[GEOADV_LIST_STATE_*] = lists in use now; anchors (scan + list build) and list iterations (scan gated off for every cloud not
 * handed back) launched; queries certified from their list, listed but refused, unlisted (both answered by brute force in the list
 * launch); cloud-iterations the scan took over because the cloud had been handed back; clouds currently handed back; forwards
 * per anchor. */
enum { GEOADV_LIST_STATE_ON = 0, GEOADV_LIST_STATE_ANCHORS, GEOADV_LIST_STATE_LIST_ITERATIONS, GEOADV_LIST_STATE_CERTIFIED,
       GEOADV_LIST_STATE_REFUSED, GEOADV_LIST_STATE_UNLISTED, GEOADV_LIST_STATE_HANDED_BACK, GEOADV_LIST_STATE_FLAGGED,
       GEOADV_LIST_STATE_PERIOD, GEOADV_LIST_STATE_COUNT };
int geoadv_attack_list_state(geoadv_attack *at, long long state[GEOADV_LIST_STATE_COUNT], void *stream);

/* ------------------------------------------------------------------------------------------
 * Victim auto-encoder TRAINING step: PointNetAutoEncoder._create_loss / _setup_optimizer
 * (src/pointnet_ae.py:71-99) driven by AutoEncoder.partial_fit (src/autoencoder.py:105-125) with the
 * architecture of src/ae_templates.py:22-33: encoder BN in TRAINING mode (tflearn batch_normalization:
 * batch statistics over all batch*n_points rows, differentiated through; moving averages updated with
 * `bn_decay`, zero_debias=False), loss = reduce_mean(dist1) + reduce_mean(dist2) of nn_distance(recon, gt) or the approx-EMD
 * match cost (geoadv_train_config.loss),
 * Adam (TF 1.13 ApplyAdam form, beta1 .9, beta2 .999, eps 1e-8) on every trainable variable.
 * One handle = one model replica with a fixed batch size; everything is device resident.
 * ---------------------------------------------------------------------------------------- */
typedef struct geoadv_trainer geoadv_trainer;
typedef struct geoadv_train_config {
    int   batch;            /* conf.batch_size (default_train_params: 50)          */
    float learning_rate;    /* conf.learning_rate (0.0005)                         */
    float bn_decay;         /* encoder b_norm_decay (encoders_decoders.py:20: 0.9) */
    int   loss;             /* conf.loss (pointnet_ae.py:74-79): GEOADV_TRAIN_LOSS_CHAMFER (0) = reduce_mean(dist1) +
                             * reduce_mean(dist2) of nn_distance(recon, gt); GEOADV_TRAIN_LOSS_EMD (1) =
                             * reduce_mean(match_cost(recon, gt, approx_match(recon, gt))), the match held constant in the
                             * backward (approx_match is registered NoGradient, tf_approxmatch.py:19)                  */
    int   max_workgroups;   /* 0 = as many persistent workgroups as the device holds (the layer kernels deal their 64- / 32-row
                             * tiles round-robin over them); > 0 caps them.  Results do not depend on it beyond the order of
                             * the per-workgroup weight-gradient partial sums; the parity tests use small values so that
                             * small shapes run the kernels' multi-tile pipelines                                       */
} geoadv_train_config;
#define GEOADV_TRAIN_LOSS_CHAMFER 0
#define GEOADV_TRAIN_LOSS_EMD     1

/* init: HOST weights (the initial variable values; bn_mean / bn_var = the moving averages).  n_points % 64 == 0. */
int  geoadv_trainer_create(geoadv_trainer **out, const geoadv_ae_weights *init, const geoadv_train_config *cfg);
void geoadv_trainer_destroy(geoadv_trainer *t);
/* partial_fit(X, GT): x, gt device [batch,n,3] (gt NULL = x, the non-denoising case); loss: device float (of the
 * PRE-update weights, like the fetched `self.loss`), recon: device [batch,n,3] or NULL. */
int geoadv_trainer_step(geoadv_trainer *t, const float *x, const float *gt, float *loss, float *recon, void *stream);
/* The two halves of a step, for data-parallel training: forward_backward leaves d loss / d variable in the flat
 * gradient buffer; the caller sum-all-reduces that buffer over the ranks (RCCL) and calls apply with
 * grad_scale = 1 / world_size. */
int geoadv_trainer_forward_backward(geoadv_trainer *t, const float *x, const float *gt, float *loss, float *recon, void *stream);
int geoadv_trainer_apply(geoadv_trainer *t, float grad_scale, void *stream);
/* Synchronised batch norm for data-parallel training (so that `world` ranks with `batch` clouds each take EXACTLY the
 * step of one replica with world * batch clouds): the encoder's only coupling between rows is a pair of per-channel
 * sums per layer and direction, so the step is cut into geoadv_trainer_num_phases() phases; after phase p the caller
 * sum-all-reduces the *count doubles geoadv_trainer_exchange(t, p, ...) points at (RCCL; <= 4 KB, latency-bound) and
 * runs phase p + 1.  After the last phase: all-reduce the flat gradient buffer, geoadv_trainer_apply(t, 1.0f), and add
 * up the ranks' geoadv_trainer_fetch losses.  geoadv_trainer_set_world(t, world) switches the mode (1 = off). */
/* set_world takes no stream: it uploads the new gradient scale with a synchronous copy from host memory, complete on return, and
 * does not wait for a step in flight -- the caller must have synchronised every stream on which a step of this handle was queued. */
int geoadv_trainer_set_world(geoadv_trainer *t, int world);
int geoadv_trainer_num_phases(void);
int geoadv_trainer_run_phase(geoadv_trainer *t, int phase, const float *x, const float *gt, void *stream);
int geoadv_trainer_exchange(geoadv_trainer *t, int phase, double **buf, size_t *count);
int geoadv_trainer_fetch(geoadv_trainer *t, float *loss, float *recon, void *stream);
/* Device pointers of the flat parameter / gradient buffers (`count` floats each) and where each variable sits:
 * offsets26 = enc_w[5], enc_b[5], bn_gamma[5], bn_beta[5], dec_w[3], dec_b[3] (in floats). */
int geoadv_trainer_buffers(geoadv_trainer *t, float **params, float **grads, size_t *count);
int geoadv_trainer_layout(const geoadv_trainer *t, size_t *offsets26);
/* Read-only TEST view of what the last forward_backward kept on the device: *ptr and its element *count for
 *   GEOADV_TRAIN_STATE_ACT         float [batch*n][C_layer]  pre-BN activations a_layer (layer 0..4)
 *   GEOADV_TRAIN_STATE_BN_MEAN / _INV_STD / _SCALE / _SHIFT   float [C_layer]  the batch statistics of layer `layer` and
 *                                  their folded form (the ReLU passes where fmaf(a, scale, shift) > 0)
 *   GEOADV_TRAIN_STATE_IDX1 / _IDX2   int [batch][n]  the Chamfer matches (loss 'chamfer')
 *   GEOADV_TRAIN_STATE_POOL_MAX    int [batch][128]  bit patterns of the max-pooled code; _POOL_TIES: rows attaining it
 *   GEOADV_TRAIN_STATE_DEC1 / _DEC2   float [batch][256]  the decoder's hidden activations (after their ReLU)
 * The pointers stay valid for the handle's life; the next step overwrites what they point to. */
#define GEOADV_TRAIN_STATE_ACT         0
#define GEOADV_TRAIN_STATE_BN_MEAN     1
#define GEOADV_TRAIN_STATE_BN_INV_STD  2
#define GEOADV_TRAIN_STATE_BN_SCALE    3
#define GEOADV_TRAIN_STATE_BN_SHIFT    4
#define GEOADV_TRAIN_STATE_IDX1        5
#define GEOADV_TRAIN_STATE_IDX2        6
#define GEOADV_TRAIN_STATE_POOL_MAX    7
#define GEOADV_TRAIN_STATE_POOL_TIES   8
#define GEOADV_TRAIN_STATE_DEC1        9
#define GEOADV_TRAIN_STATE_DEC2        10
int geoadv_trainer_state(const geoadv_trainer *t, int what, int layer, const void **ptr, size_t *count);
/* Synchronises `stream` and downloads the current variables (and moving averages) into the HOST buffers `dst` points to -- what
 * saver.save writes (autoencoder.py:213-215); feed them to geoadv_ae_create to attack the trained model.  The steps to be
 * exported must have been queued on `stream` (or be complete). */
int geoadv_trainer_export(geoadv_trainer *t, const geoadv_ae_weights *dst, void *stream);

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's roofline leg).
 * enable is a bit mask of GEOADV_PROF_* classes (bit k = class k, -1 = all, 0 = off; enabling resets
 * the totals): every geoadv_attack_run iteration brackets the selected kernels with events (a fixed
 * pool is recycled; when it runs dry the stream is synchronised once).  geoadv_attack_profile_read synchronises the stream and returns, for
 * kernel class `which` (GEOADV_PROF_*), the number of launches timed and their total ms. */
#define GEOADV_PROF_ENCODER_FWD 0
#define GEOADV_PROF_DECODER_FWD 1
#define GEOADV_PROF_CHAMFER_FWD 2
#define GEOADV_PROF_LOSS_GRAD   3
#define GEOADV_PROF_DECODER_BWD 4
#define GEOADV_PROF_ENCODER_BWD 5
#define GEOADV_PROF_ADAM        6
#define GEOADV_PROF_COUNT       7
int geoadv_attack_profile(geoadv_attack *at, int enable);
int geoadv_attack_profile_read(geoadv_attack *at, int which, int *launches, float *total_ms);
/* roctx ranges "geoadv:<class>" around the launches of every kernel class (for rocprofv3 --marker-trace timelines);
 * libroctx64 is looked up at run time.  Returns GEOADV_EINVAL if it cannot be found. */
int geoadv_attack_markers(geoadv_attack *at, int enable);
/* Time only every stride-th launch of each selected class (a pair of events between two dependent kernels costs ~1 us of
 * GPU time; sampling keeps a timed region honest).  Default 1. */
int geoadv_attack_profile_stride(geoadv_attack *at, int stride);

#ifdef __cplusplus
}
#endif
#endif /* GEOADV_H */
