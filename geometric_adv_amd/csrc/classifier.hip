// geoadv_cls: the PointNet classifier of the reference's semantic evaluation (classifier/pointnet_cls.py:30-84 with
// classifier/transform_nets.py), inference only, fp32 throughout.
//
// Six launches per forward (plus one memset of the three pooled vectors):
//   chain<1>  T-Net1 per point: tconv1 3->64 (VALU), tconv2 64->128, tconv3 128->1024 -> running max     (pooled[0])
//   head<T1>  tfc1 1024->512, tfc2 512->256, transform_XYZ 256->9 (+I) = T1; writes W1'[c] = T1 @ W_conv1   (per cloud)
//   chain<3>  conv1' 3->64 (x @ W1'), conv2 64->64, T-Net2 tconv1 64->64, tconv2 64->128, tconv3 128->1024 -> max
//   head<T2>  tfc1, tfc2, transform_feat 256->4096 (+I) = T2; writes W3'[c] = T2 @ W_conv3, packed for the MFMA
//   chain<3>  conv1', conv2, conv3' 64->64 (h @ W3'), conv4 64->128, conv5 128->1024 -> max                  (pooled[2])
//   head<CLS> fc1, fc2, fc3 256->C: logits, first-max argmax
// FOLDING: T1 is folded into conv1 and T2 into conv3 (the products x @ T1 @ W and h @ T2 @ W are rounded as x @ (T1 @ W)),
// per cloud, by the head kernel that computes the transform.  The third chain recomputes conv1 / conv2 (4 288 of its
// 147 648 multiply-adds per point) instead of storing the 64-wide features of every point.
//
// The chain kernel: a workgroup owns a tile of 64 points of one cloud (and a slice of the 1024 pooled columns: small batches
// split the columns over up to four workgroups, each recomputing the cheap narrow prefix).  The narrow layers run from LDS
// through layer_gemm (mfma_tile.h, v_mfma_f32_32x32x2_f32); the 1024-wide layer (point_tile.h: pooled_wide_layer, shared with
// AtlasNet and FoldingNet) streams 32-column blocks through gemm_chain and folds each block's 64 rows into a per-column max in registers -- the [n x 1024] activation never leaves the CU.  The
// cross-tile max is an unsigned atomicMax on the float bits of post-ReLU values (>= +0; a NaN becomes +0 in the ReLU), which
// is exact and independent of the order of tiles; rows past n are excluded before the max.  Per-point work does not depend
// on the point's position, so a cloud's logits do not depend on its point order, padding or batch neighbours.
//
// Batch norm is folded at create time (eps 1e-3, tf_util.batch_norm_template): y = relu((x @ W) * scale + shift),
// scale = gamma * rsqrt(var + eps), shift = b * scale + (beta - mean * scale).
#include "cls_model.h"
#include <math.h>
#include <string.h>

namespace geoadv {

template <int NMID>
__global__ __launch_bounds__(PT_THREADS, 2) void cls_chain_kernel(ClsChainArgs A, int cloud0) {
    __shared__ __attribute__((aligned(16))) float bufA[PT_ROWS * PT_SA];     // 64-wide activations
    __shared__ __attribute__((aligned(16))) float bufB[PT_ROWS * PT_SB];     // up to 128-wide
    __shared__ float pts[PT_ROWS * 3];
    const int tile = blockIdx.x, cloud = cloud0 + blockIdx.y, slice = blockIdx.z;
    const int n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    load_points_conv1(A.x + ((size_t)cloud * n + n0) * 3, live, A.w0 + (size_t)cloud * A.w0_cloud_stride, A.sc0, A.sh0, pts, bufA);
    if (NMID == 1) {
        cls_mid<128>(bufA, PT_SA, A.mid[0], cloud, bufB, PT_SB);
    } else {
        cls_mid<64>(bufA, PT_SA, A.mid[0], cloud, bufB, PT_SB);
        __syncthreads();
        cls_mid<64>(bufB, PT_SB, A.mid[1], cloud, bufA, PT_SA);
        __syncthreads();
        cls_mid<128>(bufA, PT_SA, A.mid[2], cloud, bufB, PT_SB);
    }
    __syncthreads();
    // the wide layer, pooled on the float bits of the post-ReLU values: non-negative floats order like their bits, +0 (the
    // ReLU's floor, and what a NaN becomes) is the identity of the max and is never sent to the atomic
    pooled_wide_layer(bufB, PT_SB, A.wide.L, A.wide.scale, A.wide.shift, slice, A.slices, live, A.pooled + (size_t)cloud * PT_POOL,
                      [](float v) { return __float_as_uint(fmaxf(v, 0.f)); });
}

enum { CLS_HEAD_T1 = 0, CLS_HEAD_T2 = 1, CLS_HEAD_CLS = 2 };
struct ClsHeadArgs {
    const unsigned *pooled;                         // [b][1024] float bits
    const float *w1, *sc1, *sh1;                    // 1024 -> 512
    const float *w2, *sc2, *sh2;                    // 512 -> 256
    const float *w3, *b3;                           // 256 -> M, linear (b3 carries the identity for the transforms)
    int M;
    float *t_out, *t_user;                          // T1 / T2: [b][M] (t_user may be null); CLS: logits [b][M]
    const float *fold_w;                            // T1: conv1 weights [3][64]; T2: conv3 weights [64][64]
    float *fold_out;                                // T1: W1' [b][3][64]; T2: W3' packed [b][4096]
    int *labels;                                    // CLS: [b]
};

template <int MODE>
__global__ __launch_bounds__(PT_THREADS) void cls_head_kernel(ClsHeadArgs H, int cloud0) {
    __shared__ float in[PT_POOL], h1[512], part[512], h2[256];
    __shared__ float tv[MODE == CLS_HEAD_T1 ? 16 : 4096];
    const int c = cloud0 + blockIdx.x, t = threadIdx.x;
    for (int k = t; k < PT_POOL; k += PT_THREADS) in[k] = __uint_as_float(H.pooled[(size_t)c * PT_POOL + k]);
    __syncthreads();
    {
        float a = 0.f;
        const float *w = H.w1 + t;
#pragma unroll 8
        for (int k = 0; k < PT_POOL; ++k) a = fmaf(in[k], w[(size_t)k * 512], a);
        h1[t] = fmaxf(a * H.sc1[t] + H.sh1[t], 0.f);
    }
    __syncthreads();
    {
        const int o = t & 255, k0 = (t >> 8) * 256;
        float a = 0.f;
        const float *w = H.w2 + o;
#pragma unroll 8
        for (int k = k0; k < k0 + 256; ++k) a = fmaf(h1[k], w[(size_t)k * 256], a);
        part[t] = a;
    }
    __syncthreads();
    if (t < 256) h2[t] = fmaxf((part[t] + part[t + 256]) * H.sc2[t] + H.sh2[t], 0.f);
    __syncthreads();
    const int M = H.M;
    for (int o = t; o < M; o += PT_THREADS) {
        float a = 0.f;
        const float *w = H.w3 + o;
#pragma unroll 8
        for (int k = 0; k < 256; ++k) a = fmaf(h2[k], w[(size_t)k * M], a);
        a = a + H.b3[o];
        H.t_out[(size_t)c * M + o] = a;
        if (H.t_user) H.t_user[(size_t)c * M + o] = a;
        if (MODE != CLS_HEAD_T1) tv[o] = a;
        else if (o < 16) tv[o] = a;
    }
    __syncthreads();
    if (MODE == CLS_HEAD_T1) {
        // W1'[k][n] = sum_j T1[k][j] Wc1[j][n]: (x @ T1) @ Wc1 with x a row vector (pointnet_cls.py:38)
        if (t < 192) {
            const int k = t >> 6, nn = t & 63;
            float a = tv[3 * k] * H.fold_w[nn];
            a = fmaf(tv[3 * k + 1], H.fold_w[64 + nn], a);
            a = fmaf(tv[3 * k + 2], H.fold_w[128 + nn], a);
            H.fold_out[(size_t)c * 192 + t] = a;
        }
    } else if (MODE == CLS_HEAD_T2) {
        // W3'[k][n] = sum_j T2[k][j] Wc3[j][n] (pointnet_cls.py:51), written in the 32x32x2 fragment layout (ae.h, K = N = 64)
        for (int e = t; e < 4096; e += PT_THREADS) {
            const int k = e >> 6, nn = e & 63;
            float a = 0.f;
            for (int j = 0; j < 64; ++j) a = fmaf(tv[64 * k + j], H.fold_w[64 * j + nn], a);
            const int cb = nn >> 5, kg = k >> 3, lane = ((k & 7) >> 2) * 32 + (nn & 31), u = k & 3;
            H.fold_out[(size_t)c * 4096 + ((cb * 8 + kg) * 64 + lane) * 4 + u] = a;
        }
    } else if (t == 0) {
        // np.argmax: the first maximum; a NaN counts as the maximum (the first NaN wins)
        int best = 0;
        float bv = tv[0];
        for (int o = 1; o < M && !(bv != bv); ++o)
            if (tv[o] > bv || tv[o] != tv[o]) { best = o; bv = tv[o]; }
        H.labels[c] = best;
    }
}

}  // namespace geoadv

using namespace geoadv;

namespace {
const int kIn[GEOADV_CLS_LAYERS] = {3, 64, 128, 1024, 512, 256, 3, 64, 64, 64, 128, 1024, 512, 256, 64, 64, 128, 1024, 512, 256};
const int kOut[GEOADV_CLS_LAYERS] = {64, 128, 1024, 512, 256, 9, 64, 64, 64, 128, 1024, 512, 256, 4096, 64, 128, 1024, 512, 256, 0};
bool has_bn(int l) { return l != T1XYZ && l != T2FEAT && l != F3; }
}  // namespace

extern "C" int geoadv_cls_create(geoadv_cls **out, const geoadv_cls_weights *hw) {
    GA_REQUIRE(out && hw, "cls_create: null argument");
    const int C = hw->num_classes;
    GA_REQUIRE(C >= 1 && C <= 1024, "cls_create: num_classes %d out of range [1, 1024]", C);
    for (int l = 0; l < GEOADV_CLS_LAYERS; ++l) {
        GA_REQUIRE(hw->w[l] && hw->b[l], "cls_create: null weight pointer at layer %d", l);
        if (has_bn(l))
            GA_REQUIRE(hw->gamma[l] && hw->beta[l] && hw->mean[l] && hw->var[l], "cls_create: null batch-norm pointer at layer %d", l);
        else
            GA_REQUIRE(!hw->gamma[l] && !hw->beta[l] && !hw->mean[l] && !hw->var[l],
                       "cls_create: layer %d has no batch norm: its batch-norm pointers must be NULL", l);
    }
    int outw[GEOADV_CLS_LAYERS];
    for (int l = 0; l < GEOADV_CLS_LAYERS; ++l) outw[l] = l == F3 ? C : kOut[l];
    HostArena arena;
    std::vector<float> &host = arena.host;
    size_t o_raw[GEOADV_CLS_LAYERS], o_pk[GEOADV_CLS_LAYERS], o_sc[GEOADV_CLS_LAYERS], o_sh[GEOADV_CLS_LAYERS], o_b[GEOADV_CLS_LAYERS];
    size_t o_pt[GEOADV_CLS_LAYERS], o_rt[GEOADV_CLS_LAYERS];
    for (int l = 0; l < GEOADV_CLS_LAYERS; ++l) {
        const int K = kIn[l], N = outw[l];
        o_raw[l] = arena.reserve((size_t)K * N);
        memcpy(&host[o_raw[l]], hw->w[l], sizeof(float) * K * N);
        o_pk[l] = 0;
        if (l == T1C2 || l == T1C3 || l == C2 || l == T2C1 || l == T2C2 || l == T2C3 || l == C4 || l == C5) {   // MFMA operands
            o_pk[l] = arena.reserve((size_t)K * N);
            pack_fragments(&host[o_pk[l]], hw->w[l], K, N);
        }
        o_pt[l] = o_rt[l] = 0;
        if (l == T1C2 || l == C2 || l == T2C1 || l == T2C2 || l == C4) {   // W^T as MFMA operands: the input gradient's narrow layers
            o_pt[l] = arena.reserve((size_t)K * N);
            const float *W = hw->w[l];
            pack_fragments(&host[o_pt[l]], N, K, N, K, [&](int k, int n) { return W[(size_t)n * N + k]; });
        }
        if (l == T1C3 || l == T2C3 || l == C5) {                          // W^T row-major: its pooled layers
            o_rt[l] = arena.reserve((size_t)K * N);
            for (int k = 0; k < K; ++k)
                for (int n = 0; n < N; ++n) host[o_rt[l] + (size_t)n * K + k] = hw->w[l][(size_t)k * N + n];
        }
        o_sc[l] = o_sh[l] = o_b[l] = 0;
        if (has_bn(l)) {   // TF's fold, eps 1e-3 -- not host_util.h's fold_bn_torch, which rounds the shift differently
            o_sc[l] = arena.reserve(N);
            o_sh[l] = arena.reserve(N);
            for (int c = 0; c < N; ++c) {
                const float inv = hw->gamma[l][c] * (1.0f / sqrtf(hw->var[l][c] + 1e-3f));
                host[o_sc[l] + c] = inv;
                host[o_sh[l] + c] = hw->b[l][c] * inv + (hw->beta[l][c] - hw->mean[l][c] * inv);
            }
        } else {
            o_b[l] = arena.reserve(N);
            for (int c = 0; c < N; ++c) host[o_b[l] + c] = hw->b[l][c];
            // transform_nets.py: biases += [1,0,0,0,1,0,0,0,1] / eye(64).flatten() -- added here, once
            if (l == T1XYZ) for (int d = 0; d < 3; ++d) host[o_b[l] + 4 * d] += 1.0f;
            if (l == T2FEAT) for (int d = 0; d < 64; ++d) host[o_b[l] + 65 * d] += 1.0f;
        }
    }
    geoadv_cls *m = new geoadv_cls();
    m->num_classes = C;
    if (int rc = arena.upload("cls_create", &m->arena)) {
        delete m;
        return rc;
    }
    const float *base = static_cast<const float *>(m->arena);
    for (int l = 0; l < GEOADV_CLS_LAYERS; ++l) {
        m->raw[l] = base + o_raw[l];
        m->packed[l] = o_pk[l] ? base + o_pk[l] : nullptr;
        m->packed_t[l] = o_pt[l] ? base + o_pt[l] : nullptr;
        m->raw_t[l] = o_rt[l] ? base + o_rt[l] : nullptr;
        m->scale[l] = has_bn(l) ? base + o_sc[l] : nullptr;
        m->shift[l] = has_bn(l) ? base + o_sh[l] : nullptr;
        m->bias[l] = has_bn(l) ? nullptr : base + o_b[l];
    }
    *out = m;
    return GEOADV_OK;
}

extern "C" void geoadv_cls_destroy(geoadv_cls *cls) {
    if (!cls) return;
    (void)hipFree(cls->arena);
    delete cls;
}

namespace {
int chunk_of(int b) { return b < CLS_MAX_GRID_Y ? b : CLS_MAX_GRID_Y; }
ClsLayerDev layer_dev(const geoadv_cls *m, int l, int K, int N) {
    return ClsLayerDev{PackedLayer{m->packed[l], K, N}, m->scale[l], m->shift[l], 0};
}
}  // namespace

extern "C" size_t geoadv_cls_workspace_bytes(const geoadv_cls *cls, int b, int n) {
    (void)n;
    if (!cls || b <= 0) return 256;
    return carve_cls(nullptr, chunk_of(b)).bytes + 256;
}

extern "C" int geoadv_cls_forward(const geoadv_cls *cls, int b, int n, const float *pc, float *logits, int *labels,
                                  float *transform_in, float *transform_feat, void *workspace, void *stream) {
    GA_REQUIRE(cls, "cls_forward: null handle");
    GA_REQUIRE(b >= 1, "cls_forward: batch %d must be >= 1", b);
    GA_REQUIRE(n >= 1 && n <= 16384, "cls_forward: n %d out of range [1, 16384]", n);
    GA_REQUIRE(pc && workspace, "cls_forward: null point cloud or workspace");
    hipStream_t st = as_stream(stream);
    const int C = cls->num_classes;
    const int tiles = cdiv(n, PT_ROWS);
    const int bc = chunk_of(b);
    const ClsScratch s = carve_cls(workspace, bc);
    const int slices = pooled_slices(tiles, b);     // (each slice recomputes its tile's narrow layers, ~7 % of a chain's work)

    ClsChainArgs ca{};
    ca.x = pc;
    ca.n = n;
    ca.slices = slices;
    ClsHeadArgs ha{};
    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nb = std::min(bc, b - c0);
        const float *x = pc + (size_t)c0 * n * 3;
        GA_HIP(hipMemsetAsync(s.pooled, 0, sizeof(unsigned) * 3 * (size_t)nb * PT_POOL, st));
        const dim3 grid(tiles, nb, slices);
        // T-Net1 chain
        ca.x = x;
        ca.w0 = cls->raw[T1C1]; ca.w0_cloud_stride = 0; ca.sc0 = cls->scale[T1C1]; ca.sh0 = cls->shift[T1C1];
        ca.mid[0] = layer_dev(cls, T1C2, 64, 128);
        ca.wide = layer_dev(cls, T1C3, 128, 1024);
        ca.pooled = s.pooled;
        hipLaunchKernelGGL(cls_chain_kernel<1>, grid, dim3(PT_THREADS), 0, st, ca, 0);
        GA_LAUNCH_CHECK();
        ha.pooled = s.pooled;
        ha.w1 = cls->raw[T1F1]; ha.sc1 = cls->scale[T1F1]; ha.sh1 = cls->shift[T1F1];
        ha.w2 = cls->raw[T1F2]; ha.sc2 = cls->scale[T1F2]; ha.sh2 = cls->shift[T1F2];
        ha.w3 = cls->raw[T1XYZ]; ha.b3 = cls->bias[T1XYZ]; ha.M = 9;
        ha.t_out = s.t1; ha.t_user = transform_in ? transform_in + (size_t)c0 * 9 : nullptr;
        ha.fold_w = cls->raw[C1]; ha.fold_out = s.w1f; ha.labels = nullptr;
        hipLaunchKernelGGL(cls_head_kernel<CLS_HEAD_T1>, dim3(nb), dim3(PT_THREADS), 0, st, ha, 0);
        GA_LAUNCH_CHECK();
        // conv1', conv2, T-Net2 chain
        ca.w0 = s.w1f; ca.w0_cloud_stride = 192; ca.sc0 = cls->scale[C1]; ca.sh0 = cls->shift[C1];
        ca.mid[0] = layer_dev(cls, C2, 64, 64);
        ca.mid[1] = layer_dev(cls, T2C1, 64, 64);
        ca.mid[2] = layer_dev(cls, T2C2, 64, 128);
        ca.wide = layer_dev(cls, T2C3, 128, 1024);
        ca.pooled = s.pooled + (size_t)nb * PT_POOL;
        hipLaunchKernelGGL(cls_chain_kernel<3>, grid, dim3(PT_THREADS), 0, st, ca, 0);
        GA_LAUNCH_CHECK();
        ha.pooled = ca.pooled;
        ha.w1 = cls->raw[T2F1]; ha.sc1 = cls->scale[T2F1]; ha.sh1 = cls->shift[T2F1];
        ha.w2 = cls->raw[T2F2]; ha.sc2 = cls->scale[T2F2]; ha.sh2 = cls->shift[T2F2];
        ha.w3 = cls->raw[T2FEAT]; ha.b3 = cls->bias[T2FEAT]; ha.M = 4096;
        ha.t_out = s.t2; ha.t_user = transform_feat ? transform_feat + (size_t)c0 * 4096 : nullptr;
        ha.fold_w = cls->raw[C3]; ha.fold_out = s.w3p;
        hipLaunchKernelGGL(cls_head_kernel<CLS_HEAD_T2>, dim3(nb), dim3(PT_THREADS), 0, st, ha, 0);
        GA_LAUNCH_CHECK();
        // conv1', conv2, conv3' .. conv5 chain
        ca.mid[1] = ClsLayerDev{PackedLayer{s.w3p, 64, 64}, cls->scale[C3], cls->shift[C3], 4096};
        ca.mid[2] = layer_dev(cls, C4, 64, 128);
        ca.wide = layer_dev(cls, C5, 128, 1024);
        ca.pooled = s.pooled + 2 * (size_t)nb * PT_POOL;
        hipLaunchKernelGGL(cls_chain_kernel<3>, grid, dim3(PT_THREADS), 0, st, ca, 0);
        GA_LAUNCH_CHECK();
        ha.pooled = ca.pooled;
        ha.w1 = cls->raw[F1]; ha.sc1 = cls->scale[F1]; ha.sh1 = cls->shift[F1];
        ha.w2 = cls->raw[F2]; ha.sc2 = cls->scale[F2]; ha.sh2 = cls->shift[F2];
        ha.w3 = cls->raw[F3]; ha.b3 = cls->bias[F3]; ha.M = C;
        ha.t_out = logits ? logits + (size_t)c0 * C : s.t2;      // (t2 is free again: [b][4096] >= [b][C])
        ha.t_user = nullptr;
        ha.fold_w = nullptr; ha.fold_out = nullptr;
        ha.labels = labels ? labels + c0 : reinterpret_cast<int *>(s.t1);
        hipLaunchKernelGGL(cls_head_kernel<CLS_HEAD_CLS>, dim3(nb), dim3(PT_THREADS), 0, st, ha, 0);
        GA_LAUNCH_CHECK();
    }
    return GEOADV_OK;
}
