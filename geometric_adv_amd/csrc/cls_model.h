// The PointNet classifier's handle, its forward scratch and the argument blocks of its per-point chain, shared by the
// forward (classifier.hip) and the input gradient (cls_grad.hip), which recomputes the forward's tiles bit for bit.
#pragma once
#include "point_tile.h"
#include "host_util.h"

namespace geoadv {

constexpr int CLS_MAX_GRID_Y = 65535;

enum {   // GEOADV_CLS_* layer order (include/geoadv.h)
    T1C1 = 0, T1C2, T1C3, T1F1, T1F2, T1XYZ, C1, C2, T2C1, T2C2, T2C3, T2F1, T2F2, T2FEAT, C3, C4, C5, F1, F2, F3
};

struct ClsLayerDev {                                // one per-point layer
    PackedLayer L;                                  // packed fragments (mid / wide layers); L.w of cloud c = L.w + c * cloud_stride
    const float *scale, *shift;
    int cloud_stride;                               // floats; 0 = shared by all clouds
};
struct ClsChainArgs {
    const float *x;                                 // [b][n][3]
    const float *w0; int w0_cloud_stride;           // layer 0 (fan-in 3): [3][64] row-major
    const float *sc0, *sh0;
    ClsLayerDev mid[3];                             // narrow MFMA layers
    ClsLayerDev wide;                               // 128 -> 1024, pooled
    unsigned *pooled;                               // [b][1024] float bits, zeroed before the launch
    int n, slices;
};

// narrow layer: out[64][NOUT] = relu((in @ W) * scale + shift)
template <int NOUT>
__device__ __forceinline__ void cls_mid(const float *in, int s_in, const ClsLayerDev &d, int cloud, float *out, int s_out) {
    PackedLayer L = d.L;
    L.w += (size_t)cloud * d.cloud_stride;
    layer_gemm<PT_ROWS, NOUT, 1>(in, s_in, L, nullptr, [&](int row, int col, float a) {
        out[row * s_out + col] = fmaxf(a * d.scale[col] + d.shift[col], 0.f);
    });
}

// Scratch of one forward of at most CLS_MAX_GRID_Y clouds, carved from the caller's workspace
struct ClsScratch {
    unsigned *pooled;        // [3][b][1024]
    float *t1, *w1f;         // [b][9], [b][192]
    float *t2, *w3p;         // [b][4096] each
    size_t bytes;
};
inline ClsScratch carve_cls(void *workspace, int b) {
    ClsScratch s;
    Carver cv(workspace);
    s.pooled = cv.take<unsigned>(3 * (size_t)b * PT_POOL);
    s.t1 = cv.take<float>((size_t)b * 9);
    s.w1f = cv.take<float>((size_t)b * 192);
    s.t2 = cv.take<float>((size_t)b * 4096);
    s.w3p = cv.take<float>((size_t)b * 4096);
    s.bytes = cv.bytes();
    return s;
}

}  // namespace geoadv

struct geoadv_cls {
    int num_classes;
    void *arena;
    const float *raw[GEOADV_CLS_LAYERS];      // row-major [in][out] (head layers, layer 0s, the fold operands)
    const float *packed[GEOADV_CLS_LAYERS];   // MFMA fragments (per-point layers of fan-in >= 64)
    const float *scale[GEOADV_CLS_LAYERS], *shift[GEOADV_CLS_LAYERS];
    const float *bias[GEOADV_CLS_LAYERS];     // linear layers: b (+ the identity for the two transforms)
    // for the input gradient (cls_grad.hip):
    const float *packed_t[GEOADV_CLS_LAYERS]; // MFMA fragments of W^T (the narrow per-point layers of fan-in >= 64)
    const float *raw_t[GEOADV_CLS_LAYERS];    // W^T row-major [1024][128] (the three pooled layers)
};
