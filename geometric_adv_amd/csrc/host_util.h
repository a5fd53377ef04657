// Host-side plumbing shared by the model translation units (ae.hip, classifier.hip, atlasnet.hip, foldingnet.hip): the MFMA
// fragment packers, the create-time arena, the torch batch-norm fold and the pooled layer's launch shape.  (The workspace
// carver, Carver, is in common.h: the operators use it too.)
#pragma once
#include <math.h>
#include <vector>
#include "ae.h"

namespace geoadv {

// W -> 32x32x2 fragments (ae.h: PackedLayer).  B[k][n] for k < K, n < N comes from `at(k, n)`; zero padded to (Kp, Np).
template <class F>
inline void pack_fragments(float *dst, int K, int N, int Kp, int Np, F at) {
    const int kg = Kp / 8;
    for (int cb = 0; cb < Np / 32; ++cb)
        for (int t = 0; t < kg; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u) {
                    const int k = 8 * t + 4 * (lane >> 5) + u, n = 32 * cb + (lane & 31);
                    dst[(((size_t)cb * kg + t) * 64 + lane) * 4 + u] = (k < K && n < N) ? at(k, n) : 0.f;
                }
}
// a row-major W [K][N], K a multiple of 8 and N of 32
inline void pack_fragments(float *dst, const float *W, int K, int N) {
    pack_fragments(dst, K, N, K, N, [&](int k, int n) { return W[(size_t)k * N + n]; });
}

// the 16x16x4 packing (ae.h)
template <class F>
inline void pack_fragments16(float *dst, int K, int N, int Kp, int Np, F at) {
    const int kg = Kp / 16;
    for (int cb = 0; cb < Np / 16; ++cb)
        for (int t = 0; t < kg; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u) {
                    const int k = 16 * t + 4 * (lane >> 4) + u, n = 16 * cb + (lane & 15);
                    dst[(((size_t)cb * kg + t) * 64 + lane) * 4 + u] = (k < K && n < N) ? at(k, n) : 0.f;
                }
}

// A model's device constants, laid out on the host (blocks of floats at 64-float alignment, zero filled) and uploaded as
// one allocation.  (Pointers into `host` do not survive a later reserve.)
struct HostArena {
    std::vector<float> host;
    size_t reserve(size_t count) {
        const size_t off = rup(host.size(), 64);
        host.resize(off + count, 0.f);
        return off;
    }
    size_t bytes() const { return sizeof(float) * host.size(); }
    // hipMalloc + copy into *arena; on failure nothing stays allocated and the status is returned with the error text set
    int upload(const char *who, void **arena) const {
        if (hipMalloc(arena, bytes()) != hipSuccess) {
            set_error("%s: hipMalloc of %zu bytes failed", who, bytes());
            return GEOADV_ENOMEM;
        }
        const hipError_t e = hipMemcpy(*arena, host.data(), bytes(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(*arena);
            set_error("%s: upload failed: %s", who, hipGetErrorString(e));
            return GEOADV_EHIP;
        }
        return GEOADV_OK;
    }
};

// Folded batch norm of N channels as torch's eval mode rounds it (eps 1e-5): scale = gamma * rsqrt(var + eps),
// shift = (b - mean) * scale + beta; without batch norm (g null) scale 1, shift b.  (The TF models -- the victim
// auto-encoder, the classifier -- fold shift = b * scale + (beta - mean * scale), which rounds differently: they keep
// their own loops.)
inline void fold_bn_torch(float *sc, float *sh, int N, const float *b, const float *g, const float *be, const float *m,
                          const float *v) {
    for (int c = 0; c < N; ++c) {
        if (g) {
            const float inv = g[c] * (1.0f / sqrtf(v[c] + 1e-5f));
            sc[c] = inv;
            sh[c] = (b[c] - m[c]) * inv + be[c];
        } else {
            sc[c] = 1.f;
            sh[c] = b[c];
        }
    }
}

// Column slices of the pooled 128 -> 1024 layer (point_tile.h: pooled_wide_layer): small batches split the 1024 columns
// over up to 4 workgroups per tile (each recomputes its tile's narrow layers) so that the launch covers the 256 CUs.
inline int pooled_slices(int tiles, int clouds) {
    int slices = 1;
    while (slices < 4 && (size_t)tiles * clouds * slices < 2 * kCUs) slices *= 2;
    return slices;
}

}  // namespace geoadv
