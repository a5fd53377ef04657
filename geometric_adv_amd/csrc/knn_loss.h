// The kNN outlier term of the attack loop (knn_loss.hip; the rule at geoadv_attack_config in include/geoadv.h).
#pragma once
#include "common.h"

namespace geoadv {

// g_dist[c,i] <- fadd_rn(g_dist[c,i], fmul_rn(dist_weight[c], fmul_rn(weight, dK/dxyz[c,i]))) and loss[c] = K(xyz[c]) (float64), K and dK
// exactly as geoadv_knn_outlier_loss forms them: its search (default kernel choice) and the gradient launch's second instance, which
// writes nothing else.  rule 0: the SOR rule with `alpha`; rule 1: the surface rule (GEOADV_KNN_LOSS_SURFACE), `alpha` its threshold.
// Both on `st`, on `workspace` of geoadv_knn_outlier_loss_workspace_bytes(b, n, k) bytes; nothing process-wide.
int launch_knn_term(int rule, int b, int n, int k, double alpha, float weight, const float *dist_weight /* [b] */,
                    const float *xyz /* [b,n,3] */, float *g_dist /* [b,n,3] */, double *loss /* [b] */, void *workspace,
                    size_t workspace_bytes, hipStream_t st);

}  // namespace geoadv
