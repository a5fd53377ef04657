// The FoldingNet graph of a whole training batch, built by foldingnet.hip's kernels for fold_train.hip: the kNN /
// covariance / CSR build and the pick resolution of the inference forward, for b clouds in ONE chunk, left in the caller's
// workspace so that the training step can read the adjacency rows in its pool backward.
#pragma once
#include "common.h"

namespace geoadv {

constexpr long long FOLD_TRAIN_MAX_ROWS = 1 << 17;     // b * n of one chunk (foldingnet.hip: fold_chunk)

struct FoldTrainGraph {
    const float *cov;            // [b][n][9]
    const int *cols;             // [2][b][n][16] neighbour indices of both pools
    const int *off, *deg, *col;  // CSR: the sorted unique row of point i of cloud c is col[c * 32 n + off[c n + i] ...], deg entries
};

size_t fold_train_graph_bytes(int b, int n);
// picks [2][b][n][16] device: read when sampling is GEOADV_FOLD_PICKS_GIVEN, written when GEOADV_FOLD_PICKS_DEVICE (cloud k
// draws with ordinal ordinal0 + k).  b * n <= FOLD_TRAIN_MAX_ROWS.
int fold_train_graph(int b, int n, const float *pc, int sampling, unsigned long long seed, long long ordinal0, int *picks,
                     void *workspace, hipStream_t st, FoldTrainGraph *out);

}  // namespace geoadv
