// geoadv_atlas: the AtlasNet auto-encoder of the transfer experiment (transfer/atlasnet/model/model_blocks.py:28-105,
// atlasnet.py:45-67 with train=False), inference only, fp32 throughout.
//
// Four launches per forward (plus one memset of the pooled keys), per chunk of clouds:
//   atlas_enc_kernel      conv1 3->64 (VALU), conv2 64->128, conv3 128->1024 (BN, NO ReLU) -> running max          (keys)
//   fc_batched_kernel     lin1 1024->1024, BN, ReLU                                          (batched over clouds: M = b)
//   fc_batched_kernel     lin2 1024->1024, BN, ReLU = the latent z; its epilogue forms c[b][p] = s1_p * z_b + t1_p
//   atlas_decoder_kernel  per (primitive, 64-row tile of that primitive's (cloud, template point) rows):
//                         relu(s1 * (W1 t) + c) generated as the A operand of conv2 1024->512, the hidden 512->512
//                         layers in LDS, last_conv 512->3 on the VALU, written straight to recon[b][p * g2 + t][:]
//
// The pooled values of conv3 are batch-normed but not rectified, so they can be negative: tiles are combined with an
// unsigned atomicMax on an ORDER-PRESERVING key of the float (positive: the sign bit set; negative: every bit flipped).  The
// key of every real float is > 0, so 0 (the memset) is the identity; the max is exact and independent of the order of tiles.
//
// Batch norm is folded at create time (eps 1e-5, torch eval mode): y = (x @ W) * scale + shift with
// scale = gamma * rsqrt(var + eps), shift = (b - mean) * scale + beta.  The decoder's first layer is
// bn1(W1 t + b1 + z) = s1 * (W1 t) + (s1 * z + t1), t1 = (b1 - mean1) * s1 + beta1; W1 is stored pre-scaled by s1.
// Without decoder batch norm (remove_all_batchNorms) scale = 1 and shift = b.
//
// Every per-row / per-point computation is independent of the row's position in its tile and no sum is split by batch
// size, so a cloud's outputs do not depend on b, on its position in the batch or on its point order.
#include "point_tile.h"
#include "host_util.h"
#include <math.h>
#include <string.h>

namespace geoadv {

constexpr int AT_LAT = PT_POOL;                   // the latent: the pooled layer's width, and the FC layers'
constexpr int AT_MAX_NB = 128, AT_MAX_L = 4;
constexpr size_t AT_DEC_LDS = sizeof(float) * (PT_ROWS * PT_SH + 2 * 3 * PT_ROWS + 3 * PT_ROWS) + sizeof(int) * 2 * PT_ROWS;

// ------------------------------------------------------------------------------------------------ encoder per-point chain
struct AtlasEncArgs {
    const float *x;                                 // [b][n][3]
    const float *w0, *sc0, *sh0;                    // conv1: [3][64] row-major
    PackedLayer l1; const float *sc1, *sh1;         // conv2 64 -> 128
    PackedLayer l2; const float *sc2, *sh2;         // conv3 128 -> 1024, pooled (no ReLU)
    unsigned *keys;                                 // [b][1024] order-preserving keys, zeroed before the launch
    int n, slices;
};

__global__ __launch_bounds__(PT_THREADS, 2) void atlas_enc_kernel(AtlasEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[PT_ROWS * PT_SA];
    __shared__ __attribute__((aligned(16))) float bufB[PT_ROWS * PT_SB];
    __shared__ float pts[PT_ROWS * 3];
    const int tile = blockIdx.x, cloud = blockIdx.y, slice = blockIdx.z;
    const int n = A.n, n0 = tile * PT_ROWS;
    const int live = n - n0 < PT_ROWS ? n - n0 : PT_ROWS;
    load_points_conv1(A.x + ((size_t)cloud * n + n0) * 3, live, A.w0, A.sc0, A.sh0, pts, bufA);
    layer_gemm<PT_ROWS, 128, 1>(bufA, PT_SA, A.l1, nullptr, [&](int row, int col, float a) {
        bufB[row * PT_SB + col] = fmaxf(a * A.sc1[col] + A.sh1[col], 0.f);
    });
    __syncthreads();
    // conv3, pooled on the keys of the unrectified values
    pooled_wide_layer(bufB, PT_SB, A.l2, A.sc2, A.sh2, slice, A.slices, live, A.keys + (size_t)cloud * AT_LAT,
                      [](float v) { return float_key(v); });
}

// ------------------------------------------------------------------------------------------------ decoder chain
struct AtlasDecArgs {
    const float *tmpl;                              // [nb][g2][dim]
    const float *w1s;                               // [nb][dim][1024]: s1 * W1
    const float *c;                                 // [b][nb][1024]
    const float *l2w, *sc2, *sh2;                   // conv2 packed [nb][1024 * 512], [nb][512]
    const float *lhw, *sch, *shh;                   // conv_list packed [nb][L][512 * 512], [nb][L][512]
    const float *wl, *bl;                           // last_conv [nb][512][3], [nb][3]
    float *recon;                                   // [b][nb * g2][3]
    int b, nb, g2, dim, num_layers, tiles, blocks;
};

__global__ __launch_bounds__(PT_THREADS) void atlas_decoder_kernel(AtlasDecArgs A) {
    extern __shared__ __attribute__((aligned(16))) float at_lds[];
    float *H = at_lds;                                          // [64][PT_SH]
    float *part = H + PT_ROWS * PT_SH;                          // [2][64 * 3] last_conv partial sums (two halves of K)
    float *tp = part + 2 * 3 * PT_ROWS;                         // [64][3] template coordinates of the tile's rows
    int *rcloud = reinterpret_cast<int *>(tp + 3 * PT_ROWS);    // [64] cloud of each row
    int *rpoint = rcloud + PT_ROWS;                             // [64] template point of each row
    // XCD-aware order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, so workgroup g is given the
    // logical tile (g % 8) * (grid / 8) + g / 8 -- each XCD walks a contiguous range of tiles and keeps one primitive's
    // 4 MB of decoder weights in its L2 while it does.  (Placement only changes speed.)
    const int g = blockIdx.x, per = gridDim.x >> 3;
    const int logical = (g & 7) * per + (g >> 3);
    if (logical >= A.blocks) return;
    const int p = __builtin_amdgcn_readfirstlane(logical / A.tiles), tile = logical - p * A.tiles;
    const int rows = A.b * A.g2, r0 = tile * PT_ROWS;
    const int live = rows - r0 < PT_ROWS ? rows - r0 : PT_ROWS;
    if (threadIdx.x < PT_ROWS) {
        const int r = r0 + (threadIdx.x < live ? threadIdx.x : 0);     // padding rows repeat the tile's first row
        const int c = r / A.g2, t = r - c * A.g2;
        rcloud[threadIdx.x] = c;
        rpoint[threadIdx.x] = t;
        for (int d = 0; d < 3; ++d) tp[threadIdx.x * 3 + d] = d < A.dim ? A.tmpl[((size_t)p * A.g2 + t) * A.dim + d] : 0.f;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cb0 = 2 * wave;                                   // the wave's two 32-column blocks of the 512 outputs
    // conv2 1024 -> 512, its A operand generated in two 512-wide K chunks: relu(s1 * (W1 t) + c[cloud][p])
    {
        const PackedLayer L{A.l2w + (size_t)p * AT_LAT * PT_HID, AT_LAT, PT_HID};
        const float *w1 = A.w1s + (size_t)p * A.dim * AT_LAT;
        f32x16 acc[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q][0] = acc[q][1] = f32x16{};
        for (int ch = 0; ch < 2; ++ch) {
            const int k0 = ch * PT_HID;
            for (int e = threadIdx.x; e < PT_ROWS * (PT_HID / 4); e += PT_THREADS) {
                const int r = e >> 7, k = k0 + 4 * (e & 127);
                const float4 cv = *reinterpret_cast<const float4 *>(A.c + ((size_t)rcloud[r] * A.nb + p) * AT_LAT + k);
                float v[4] = {cv.x, cv.y, cv.z, cv.w};
                for (int d = 0; d < A.dim; ++d) {
                    const float4 wv = *reinterpret_cast<const float4 *>(w1 + d * AT_LAT + k);
                    const float td = tp[r * 3 + d];
                    v[0] = fmaf(wv.x, td, v[0]); v[1] = fmaf(wv.y, td, v[1]);
                    v[2] = fmaf(wv.z, td, v[2]); v[3] = fmaf(wv.w, td, v[3]);
                }
                *reinterpret_cast<float4 *>(H + r * PT_SH + (k - k0)) =
                    make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
            }
            __syncthreads();
            // gemm_chain reads A at in + row * s_in + 8 t for k-groups t in [64 ch, 64 ch + 64): the chunk starts at H
#pragma unroll
            for (int q = 0; q < 2; ++q) gemm_chain<2>(H - k0, PT_SH, 0, L, cb0 + q, k0 / 8, k0 / 8 + PT_HID / 8, acc[q]);
            __syncthreads();
        }
        dec512_epilogue<true>(H, acc, cb0, A.sc2 + (size_t)p * PT_HID, A.sh2 + (size_t)p * PT_HID);
        __syncthreads();
    }
    // conv_list: 512 -> 512, in place in H
    for (int l = 0; l < A.num_layers; ++l) {
        const size_t pl = (size_t)p * A.num_layers + l;
        dec512_hidden<true>(H, PackedLayer{A.lhw + pl * PT_HID * PT_HID, PT_HID, PT_HID}, A.sch + pl * PT_HID, A.shh + pl * PT_HID);
    }
    // last_conv 512 -> 3, written straight to the reconstruction
    dec512_last(H, A.wl + (size_t)p * PT_HID * 3, A.bl + p * 3, part, [&](int o, float y) {
        const int r = o / 3, d = o - 3 * r;
        const size_t P = (size_t)A.nb * A.g2;
        if (r < live) A.recon[((size_t)rcloud[r] * P + (size_t)p * A.g2 + rpoint[r]) * 3 + d] = y;
    });
}

}  // namespace geoadv

using namespace geoadv;

struct geoadv_atlas {
    geoadv_atlas_config cfg;
    void *arena;
    const float *e_w0, *e_sc[GEOADV_ATLAS_ENC_LAYERS], *e_sh[GEOADV_ATLAS_ENC_LAYERS];
    const float *e_pk1, *e_pk2;                     // conv2, conv3 packed
    const float *e_lin[2];                          // lin1, lin2 row-major [1024][1024]
    const float *tmpl, *w1s, *s1, *t1;              // decoder layer 1: template, s1 * W1, scale, shift   (per primitive)
    const float *l2w, *sc2, *sh2, *lhw, *sch, *shh, *wl, *bl;
};

extern "C" int geoadv_atlas_create(geoadv_atlas **out, const geoadv_atlas_config *cfg, const geoadv_atlas_weights *hw,
                                   const float *host_template) {
    GA_REQUIRE(out && cfg && hw && host_template, "atlas_create: null argument");
    const int NB = cfg->nb_primitives, G2 = cfg->points_per_primitive, DIM = cfg->dim_template, NL = cfg->num_layers;
    GA_REQUIRE(NB >= 1 && NB <= AT_MAX_NB, "atlas_create: nb_primitives %d out of range [1, %d]", NB, AT_MAX_NB);
    GA_REQUIRE(G2 >= 1 && G2 <= 65536, "atlas_create: points_per_primitive %d out of range [1, 65536]", G2);
    GA_REQUIRE(DIM == 2 || DIM == 3, "atlas_create: dim_template %d is not 2 or 3", DIM);
    GA_REQUIRE(cfg->bottleneck_size == AT_LAT, "atlas_create: bottleneck_size %d is not %d", cfg->bottleneck_size, AT_LAT);
    GA_REQUIRE(cfg->hidden_neurons == PT_HID, "atlas_create: hidden_neurons %d is not %d", cfg->hidden_neurons, PT_HID);
    GA_REQUIRE(NL >= 0 && NL <= AT_MAX_L, "atlas_create: num_layers %d out of range [0, %d]", NL, AT_MAX_L);
    GA_REQUIRE(cfg->activation == 0, "atlas_create: activation %d is not 0 (relu)", cfg->activation);
    GA_REQUIRE(cfg->decoder_bn == 0 || cfg->decoder_bn == 1, "atlas_create: decoder_bn %d is not 0 or 1", cfg->decoder_bn);
    for (int l = 0; l < GEOADV_ATLAS_ENC_LAYERS; ++l)
        GA_REQUIRE(hw->enc_w[l] && hw->enc_b[l] && hw->enc_gamma[l] && hw->enc_beta[l] && hw->enc_mean[l] && hw->enc_var[l],
                   "atlas_create: null encoder pointer at layer %d", l);
    const int NDL = 3 + NL;
    for (int l = 0; l < GEOADV_ATLAS_MAX_DEC_LAYERS; ++l) {
        const bool used = l < NDL, bn = used && cfg->decoder_bn && l != NDL - 1;
        GA_REQUIRE(!used || (hw->dec_w[l] && hw->dec_b[l]), "atlas_create: null decoder weight pointer at layer %d", l);
        if (bn)
            GA_REQUIRE(hw->dec_gamma[l] && hw->dec_beta[l] && hw->dec_mean[l] && hw->dec_var[l],
                       "atlas_create: null decoder batch-norm pointer at layer %d", l);
        else
            GA_REQUIRE(!hw->dec_gamma[l] && !hw->dec_beta[l] && !hw->dec_mean[l] && !hw->dec_var[l],
                       "atlas_create: decoder layer %d has no batch norm: its batch-norm pointers must be NULL", l);
    }
    static const int eout[5] = {64, 128, AT_LAT, AT_LAT, AT_LAT};
    HostArena arena;
    std::vector<float> &host = arena.host;
    size_t o_w0, o_esc[5], o_esh[5], o_pk1, o_pk2, o_lin[2];
    o_w0 = arena.reserve(3 * 64);
    memcpy(&host[o_w0], hw->enc_w[0], sizeof(float) * 3 * 64);
    o_pk1 = arena.reserve(64 * 128);
    pack_fragments(&host[o_pk1], hw->enc_w[1], 64, 128);
    o_pk2 = arena.reserve((size_t)128 * AT_LAT);
    pack_fragments(&host[o_pk2], hw->enc_w[2], 128, AT_LAT);
    for (int q = 0; q < 2; ++q) {
        o_lin[q] = arena.reserve((size_t)AT_LAT * AT_LAT);
        memcpy(&host[o_lin[q]], hw->enc_w[3 + q], sizeof(float) * AT_LAT * AT_LAT);
    }
    for (int l = 0; l < 5; ++l) {
        o_esc[l] = arena.reserve(eout[l]);
        o_esh[l] = arena.reserve(eout[l]);
        fold_bn_torch(&host[o_esc[l]], &host[o_esh[l]], eout[l], hw->enc_b[l], hw->enc_gamma[l], hw->enc_beta[l], hw->enc_mean[l],
                hw->enc_var[l]);
    }
    const bool bn = cfg->decoder_bn != 0;
    auto dec_bn = [&](int l, int p, int N, float *sc, float *sh) {
        const size_t o = (size_t)p * N;
        fold_bn_torch(sc, sh, N, hw->dec_b[l] + o, bn ? hw->dec_gamma[l] + o : nullptr, bn ? hw->dec_beta[l] + o : nullptr,
                bn ? hw->dec_mean[l] + o : nullptr, bn ? hw->dec_var[l] + o : nullptr);
    };
    const size_t o_tmpl = arena.reserve((size_t)NB * G2 * DIM);
    memcpy(&host[o_tmpl], host_template, sizeof(float) * NB * G2 * DIM);
    const size_t o_w1s = arena.reserve((size_t)NB * DIM * AT_LAT), o_s1 = arena.reserve((size_t)NB * AT_LAT), o_t1 = arena.reserve((size_t)NB * AT_LAT);
    const size_t o_l2w = arena.reserve((size_t)NB * AT_LAT * PT_HID), o_sc2 = arena.reserve((size_t)NB * PT_HID), o_sh2 = arena.reserve((size_t)NB * PT_HID);
    const size_t nh = (size_t)NB * NL;
    const size_t o_lhw = arena.reserve(nh * PT_HID * PT_HID + 1), o_sch = arena.reserve(nh * PT_HID + 1), o_shh = arena.reserve(nh * PT_HID + 1);
    const size_t o_wl = arena.reserve((size_t)NB * PT_HID * 3), o_bl = arena.reserve((size_t)NB * 3);
    for (int p = 0; p < NB; ++p) {
        float *s1 = &host[o_s1 + (size_t)p * AT_LAT], *t1 = &host[o_t1 + (size_t)p * AT_LAT];
        dec_bn(0, p, AT_LAT, s1, t1);
        const float *w1 = hw->dec_w[0] + (size_t)p * DIM * AT_LAT;
        for (int d = 0; d < DIM; ++d)
            for (int k = 0; k < AT_LAT; ++k) host[o_w1s + ((size_t)p * DIM + d) * AT_LAT + k] = s1[k] * w1[(size_t)d * AT_LAT + k];
        pack_fragments(&host[o_l2w + (size_t)p * AT_LAT * PT_HID], hw->dec_w[1] + (size_t)p * AT_LAT * PT_HID, AT_LAT, PT_HID);
        dec_bn(1, p, PT_HID, &host[o_sc2 + (size_t)p * PT_HID], &host[o_sh2 + (size_t)p * PT_HID]);
        for (int l = 0; l < NL; ++l) {
            const size_t pl = (size_t)p * NL + l;
            pack_fragments(&host[o_lhw + pl * PT_HID * PT_HID], hw->dec_w[2 + l] + (size_t)p * PT_HID * PT_HID, PT_HID, PT_HID);
            dec_bn(2 + l, p, PT_HID, &host[o_sch + pl * PT_HID], &host[o_shh + pl * PT_HID]);
        }
        memcpy(&host[o_wl + (size_t)p * PT_HID * 3], hw->dec_w[NDL - 1] + (size_t)p * PT_HID * 3, sizeof(float) * PT_HID * 3);
        memcpy(&host[o_bl + (size_t)p * 3], hw->dec_b[NDL - 1] + (size_t)p * 3, sizeof(float) * 3);
    }
    geoadv_atlas *m = new geoadv_atlas();
    m->cfg = *cfg;
    if (int rc = arena.upload("atlas_create", &m->arena)) {
        delete m;
        return rc;
    }
    const float *base = static_cast<const float *>(m->arena);
    m->e_w0 = base + o_w0;
    for (int l = 0; l < 5; ++l) { m->e_sc[l] = base + o_esc[l]; m->e_sh[l] = base + o_esh[l]; }
    m->e_pk1 = base + o_pk1; m->e_pk2 = base + o_pk2;
    m->e_lin[0] = base + o_lin[0]; m->e_lin[1] = base + o_lin[1];
    m->tmpl = base + o_tmpl; m->w1s = base + o_w1s; m->s1 = base + o_s1; m->t1 = base + o_t1;
    m->l2w = base + o_l2w; m->sc2 = base + o_sc2; m->sh2 = base + o_sh2;
    m->lhw = base + o_lhw; m->sch = base + o_sch; m->shh = base + o_shh;
    m->wl = base + o_wl; m->bl = base + o_bl;
    *out = m;
    return GEOADV_OK;
}

extern "C" void geoadv_atlas_destroy(geoadv_atlas *atlas) {
    if (!atlas) return;
    (void)hipFree(atlas->arena);
    delete atlas;
}

namespace {
struct AtlasScratch {
    unsigned *keys;          // [bc][1024]
    float *h1, *z;           // [bc][1024]
    float *c;                // [bc][nb][1024]
    size_t bytes;
};
AtlasScratch carve_atlas(void *workspace, int bc, int nb) {
    AtlasScratch s;
    Carver cv(workspace);
    s.keys = cv.take<unsigned>((size_t)bc * AT_LAT);
    s.h1 = cv.take<float>((size_t)bc * AT_LAT);
    s.z = cv.take<float>((size_t)bc * AT_LAT);
    s.c = cv.take<float>((size_t)bc * nb * AT_LAT);
    s.bytes = cv.bytes();
    return s;
}
// clouds per chunk: bounds the per-(cloud, primitive) layer-1 shifts at 8192 x 4 KiB and the grids' y extents
int atlas_chunk(int b, int nb) {
    const int cap = std::max(1, 8192 / nb);
    return std::min(b, std::min(cap, 1024));
}
}  // namespace

extern "C" size_t geoadv_atlas_workspace_bytes(const geoadv_atlas *atlas, int b, int n) {
    (void)n;
    if (!atlas || b <= 0) return 256;
    return carve_atlas(nullptr, atlas_chunk(b, atlas->cfg.nb_primitives), atlas->cfg.nb_primitives).bytes + 256;
}

extern "C" int geoadv_atlas_forward(const geoadv_atlas *atlas, int b, int n, const float *pc, float *latent, float *recon,
                                    void *workspace, void *stream) {
    GA_REQUIRE(atlas, "atlas_forward: null handle");
    GA_REQUIRE(b >= 1, "atlas_forward: batch %d must be >= 1", b);
    GA_REQUIRE(n >= 1 && n <= 16384, "atlas_forward: n %d out of range [1, 16384]", n);
    GA_REQUIRE(pc && recon && workspace, "atlas_forward: null point cloud, reconstruction or workspace");
    static DeviceOnce attr;
    if (int rc = attr.run([]() -> int {
            GA_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(atlas_decoder_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)AT_DEC_LDS));
            return GEOADV_OK;
        })) return rc;
    hipStream_t st = as_stream(stream);
    const geoadv_atlas_config &cf = atlas->cfg;
    const int NB = cf.nb_primitives, G2 = cf.points_per_primitive;
    const size_t P = (size_t)NB * G2;
    const int tiles = cdiv(n, PT_ROWS);
    const int bc = atlas_chunk(b, NB);
    const AtlasScratch s = carve_atlas(workspace, bc, NB);
    const int slices = pooled_slices(tiles, b);

    AtlasEncArgs ea{};
    ea.w0 = atlas->e_w0; ea.sc0 = atlas->e_sc[0]; ea.sh0 = atlas->e_sh[0];
    ea.l1 = PackedLayer{atlas->e_pk1, 64, 128}; ea.sc1 = atlas->e_sc[1]; ea.sh1 = atlas->e_sh[1];
    ea.l2 = PackedLayer{atlas->e_pk2, 128, AT_LAT}; ea.sc2 = atlas->e_sc[2]; ea.sh2 = atlas->e_sh[2];
    ea.keys = s.keys; ea.n = n; ea.slices = slices;
    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nbc = std::min(bc, b - c0);
        GA_HIP(hipMemsetAsync(s.keys, 0, sizeof(unsigned) * (size_t)nbc * AT_LAT, st));
        ea.x = pc + (size_t)c0 * n * 3;
        hipLaunchKernelGGL(atlas_enc_kernel, dim3(tiles, nbc, slices), dim3(PT_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        const dim3 fg(AT_LAT / 64, cdiv(nbc, FC_CLOUDS));
        FcBatchedArgs fa{};
        fa.keys = s.keys; fa.w = atlas->e_lin[0]; fa.sc = atlas->e_sc[3]; fa.sh = atlas->e_sh[3];
        fa.out = s.h1; fa.N = AT_LAT; fa.b = nbc; fa.relu = 1; fa.nb = NB;
        hipLaunchKernelGGL(fc_batched_kernel<AT_LAT>, fg, dim3(FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        float *z = latent ? latent + (size_t)c0 * AT_LAT : s.z;
        fa.keys = nullptr; fa.in = s.h1; fa.w = atlas->e_lin[1]; fa.sc = atlas->e_sc[4]; fa.sh = atlas->e_sh[4];
        fa.out = z; fa.s1 = atlas->s1; fa.t1 = atlas->t1; fa.c = s.c;
        hipLaunchKernelGGL(fc_batched_kernel<AT_LAT>, fg, dim3(FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        AtlasDecArgs da{};
        da.tmpl = atlas->tmpl; da.w1s = atlas->w1s; da.c = s.c;
        da.l2w = atlas->l2w; da.sc2 = atlas->sc2; da.sh2 = atlas->sh2;
        da.lhw = atlas->lhw; da.sch = atlas->sch; da.shh = atlas->shh;
        da.wl = atlas->wl; da.bl = atlas->bl;
        da.recon = recon + (size_t)c0 * P * 3;
        da.b = nbc; da.nb = NB; da.g2 = G2; da.dim = cf.dim_template; da.num_layers = cf.num_layers;
        da.tiles = cdiv(nbc * G2, PT_ROWS);
        da.blocks = da.tiles * NB;
        const int grid = cdiv(da.blocks, 8) * 8;
        hipLaunchKernelGGL(atlas_decoder_kernel, dim3(grid), dim3(PT_THREADS), AT_DEC_LDS, st, da);
        GA_LAUNCH_CHECK();
    }
    return GEOADV_OK;
}
