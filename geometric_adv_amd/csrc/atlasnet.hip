// geoadv_atlas: the AtlasNet auto-encoder of the transfer experiment (transfer/atlasnet/model/model_blocks.py:28-105,
// atlasnet.py:45-67 with train=False), inference only, fp32 throughout.
//
// Four launches per forward (plus one memset of the pooled keys), per chunk of clouds:
//   atlas_enc_kernel      conv1 3->64 (VALU), conv2 64->128, conv3 128->1024 (BN, NO ReLU) -> running max          (keys)
//   atlas_fc_kernel       lin1 1024->1024, BN, ReLU                                          (batched over clouds: M = b)
//   atlas_fc_kernel       lin2 1024->1024, BN, ReLU = the latent z; its epilogue forms c[b][p] = s1_p * z_b + t1_p
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
#include "mfma_tile.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace geoadv {

constexpr int AT_ROWS = 64, AT_THREADS = 512, AT_LAT = 1024, AT_HID = 512;
constexpr int AT_SA = 68, AT_SB = 132;            // encoder LDS row strides (64- and 128-wide activations)
constexpr int AT_SH = AT_HID + 4;                 // decoder LDS row stride: 512-wide activations / 512-wide layer-1 chunks
constexpr int AT_MAX_NB = 128, AT_MAX_L = 4;
constexpr int AT_FC_CLOUDS = 8, AT_FC_THREADS = 256;
constexpr size_t AT_DEC_LDS = sizeof(float) * (AT_ROWS * AT_SH + 2 * 3 * AT_ROWS + 3 * AT_ROWS) + sizeof(int) * 2 * AT_ROWS;

__device__ __forceinline__ unsigned atlas_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float atlas_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ------------------------------------------------------------------------------------------------ encoder per-point chain
struct AtlasEncArgs {
    const float *x;                                 // [b][n][3]
    const float *w0, *sc0, *sh0;                    // conv1: [3][64] row-major
    PackedLayer l1; const float *sc1, *sh1;         // conv2 64 -> 128
    PackedLayer l2; const float *sc2, *sh2;         // conv3 128 -> 1024, pooled (no ReLU)
    unsigned *keys;                                 // [b][1024] order-preserving keys, zeroed before the launch
    int n, slices;
};

__global__ __launch_bounds__(AT_THREADS, 2) void atlas_enc_kernel(AtlasEncArgs A) {
    __shared__ __attribute__((aligned(16))) float bufA[AT_ROWS * AT_SA];
    __shared__ __attribute__((aligned(16))) float bufB[AT_ROWS * AT_SB];
    __shared__ float pts[AT_ROWS * 3];
    const int tile = blockIdx.x, cloud = blockIdx.y, slice = blockIdx.z;
    const int n = A.n, n0 = tile * AT_ROWS;
    const int live = n - n0 < AT_ROWS ? n - n0 : AT_ROWS;
    if (threadIdx.x < AT_ROWS * 3) {
        const int r = threadIdx.x / 3;
        pts[threadIdx.x] = r < live ? A.x[((size_t)cloud * n + n0) * 3 + threadIdx.x] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < AT_ROWS * 64; e += AT_THREADS) {      // conv1 3 -> 64 on the VALU
        const int r = e >> 6, c = e & 63;
        const float a = pts[3 * r] * A.w0[c] + pts[3 * r + 1] * A.w0[64 + c] + pts[3 * r + 2] * A.w0[128 + c];
        bufA[r * AT_SA + c] = fmaxf(a * A.sc0[c] + A.sh0[c], 0.f);
    }
    __syncthreads();
    layer_gemm<AT_ROWS, 128, 1>(bufA, AT_SA, A.l1, nullptr, [&](int row, int col, float a) {
        bufB[row * AT_SB + col] = fmaxf(a * A.sc1[col] + A.sh1[col], 0.f);
    });
    __syncthreads();
    // conv3: 32-column blocks of this workgroup's slice dealt to the 8 waves, both row blocks per wave; the max over the
    // tile's live rows is taken in registers, then across tiles by the atomic on the keys
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, i = lane & 31;
    const int nblk = (AT_LAT / 32) / A.slices;
    unsigned *keys = A.keys + (size_t)cloud * AT_LAT;
    for (int j = wave; j < nblk; j += AT_THREADS / 64) {
        const int cb = slice * nblk + j;
        f32x16 acc[2] = {};
        gemm_chain<2>(bufB, AT_SB, 0, A.l2, cb, 0, 128 / 8, acc);
        const int col = cb * 32 + i;
        const float sc = A.sc2[col], sh = A.sh2[col];
        unsigned m = 0;                              // below the key of every float
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rm * 32 + acc_row(r, h);
                const unsigned v = atlas_key(acc[rm][r] * sc + sh);
                if (row < live) m = max(m, v);
            }
        m = max(m, (unsigned)__shfl_xor((int)m, 32));
        if (h == 0 && m != 0) atomicMax(keys + col, m);
    }
}

// ------------------------------------------------------------------------------------------------ FC head (M = b)
// One workgroup: 64 output columns (a lane each) x 8 clouds, the 1024 inputs split in four quarters over the 4 waves and
// summed in a fixed order -- the same for every cloud, whatever the batch size.
struct AtlasFcArgs {
    const unsigned *keys;                           // input as pooled keys [b][1024] (lin1), or
    const float *in;                                // as floats [b][1024] (lin2)
    const float *w, *sc, *sh;                       // [1024][1024] row-major, folded BN
    float *out;                                     // [b][1024]
    const float *s1, *t1;                           // non-null: c[b][p][:] = s1[p] * out + t1[p]   (decoder layer 1)
    float *c;
    int nb, b;
};

__global__ __launch_bounds__(AT_FC_THREADS) void atlas_fc_kernel(AtlasFcArgs F) {
    __shared__ float xin[AT_FC_CLOUDS][AT_LAT];
    __shared__ float part[4][AT_FC_CLOUDS][64];
    const int c0 = blockIdx.y * AT_FC_CLOUDS, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + lane;
    for (int e = threadIdx.x; e < AT_FC_CLOUDS * AT_LAT; e += AT_FC_THREADS) {
        const int j = e >> 10, k = e & (AT_LAT - 1), c = c0 + j;
        float v = 0.f;
        if (c < F.b) v = F.keys ? atlas_unkey(F.keys[(size_t)c * AT_LAT + k]) : F.in[(size_t)c * AT_LAT + k];
        xin[j][k] = v;
    }
    __syncthreads();
    float acc[AT_FC_CLOUDS] = {};
    const int k0 = wave * (AT_LAT / 4);
    const float *w = F.w + (size_t)k0 * AT_LAT + col;
#pragma unroll 8
    for (int k = 0; k < AT_LAT / 4; ++k) {
        const float wv = w[(size_t)k * AT_LAT];
#pragma unroll
        for (int j = 0; j < AT_FC_CLOUDS; ++j) acc[j] = fmaf(xin[j][k0 + k], wv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < AT_FC_CLOUDS; ++j) part[wave][j][lane] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < AT_FC_CLOUDS * 64; e += AT_FC_THREADS) {
        const int j = e >> 6, l = e & 63, c = c0 + j;
        if (c >= F.b) continue;
        const int o = blockIdx.x * 64 + l;
        const float s = (part[0][j][l] + part[1][j][l]) + (part[2][j][l] + part[3][j][l]);
        const float y = fmaxf(s * F.sc[o] + F.sh[o], 0.f);
        F.out[(size_t)c * AT_LAT + o] = y;
        if (F.c)
            for (int p = 0; p < F.nb; ++p)
                F.c[((size_t)c * F.nb + p) * AT_LAT + o] = fmaf(F.s1[(size_t)p * AT_LAT + o], y, F.t1[(size_t)p * AT_LAT + o]);
    }
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

// relu((acc * scale + shift)) of a wave's 2 x 2 (column block, row block) accumulators into the LDS activation tile
__device__ __forceinline__ void atlas_dec_epilogue(float *H, const f32x16 (&acc)[2][2], int cb0, const float *sc,
                                                   const float *sh) {
    const int lane = threadIdx.x & 63, h = lane >> 5, i = lane & 31;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int col = (cb0 + q) * 32 + i;
        const float s = sc[col], t = sh[col];
#pragma unroll
        for (int rm = 0; rm < 2; ++rm)
#pragma unroll
            for (int r = 0; r < 16; ++r) H[(rm * 32 + acc_row(r, h)) * AT_SH + col] = fmaxf(acc[q][rm][r] * s + t, 0.f);
    }
}

__global__ __launch_bounds__(AT_THREADS) void atlas_decoder_kernel(AtlasDecArgs A) {
    extern __shared__ __attribute__((aligned(16))) float at_lds[];
    float *H = at_lds;                                          // [64][AT_SH]
    float *part = H + AT_ROWS * AT_SH;                          // [2][64 * 3] last_conv partial sums (two halves of K)
    float *tp = part + 2 * 3 * AT_ROWS;                         // [64][3] template coordinates of the tile's rows
    int *rcloud = reinterpret_cast<int *>(tp + 3 * AT_ROWS);    // [64] cloud of each row
    int *rpoint = rcloud + AT_ROWS;                             // [64] template point of each row
    // XCD-aware order: the dispatcher deals consecutive workgroups round-robin to the 8 XCDs, so workgroup g is given the
    // logical tile (g % 8) * (grid / 8) + g / 8 -- each XCD walks a contiguous range of tiles and keeps one primitive's
    // 4 MB of decoder weights in its L2 while it does.  (Placement only changes speed.)
    const int g = blockIdx.x, per = gridDim.x >> 3;
    const int logical = (g & 7) * per + (g >> 3);
    if (logical >= A.blocks) return;
    const int p = __builtin_amdgcn_readfirstlane(logical / A.tiles), tile = logical - p * A.tiles;
    const int rows = A.b * A.g2, r0 = tile * AT_ROWS;
    const int live = rows - r0 < AT_ROWS ? rows - r0 : AT_ROWS;
    if (threadIdx.x < AT_ROWS) {
        const int r = r0 + (threadIdx.x < live ? threadIdx.x : 0);     // padding rows repeat the tile's first row
        const int c = r / A.g2, t = r - c * A.g2;
        rcloud[threadIdx.x] = c;
        rpoint[threadIdx.x] = t;
        for (int d = 0; d < 3; ++d) tp[threadIdx.x * 3 + d] = d < A.dim ? A.tmpl[((size_t)p * A.g2 + t) * A.dim + d] : 0.f;
    }
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cb0 = 2 * wave;                                   // the wave's two 32-column blocks of the 512 outputs
    f32x16 acc[2][2];
    // conv2 1024 -> 512, its A operand generated in two 512-wide K chunks: relu(s1 * (W1 t) + c[cloud][p])
    {
        const PackedLayer L{A.l2w + (size_t)p * AT_LAT * AT_HID, AT_LAT, AT_HID};
        const float *w1 = A.w1s + (size_t)p * A.dim * AT_LAT;
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[q][0] = acc[q][1] = f32x16{};
        for (int ch = 0; ch < 2; ++ch) {
            const int k0 = ch * AT_HID;
            for (int e = threadIdx.x; e < AT_ROWS * (AT_HID / 4); e += AT_THREADS) {
                const int r = e >> 7, k = k0 + 4 * (e & 127);
                const float4 cv = *reinterpret_cast<const float4 *>(A.c + ((size_t)rcloud[r] * A.nb + p) * AT_LAT + k);
                float v[4] = {cv.x, cv.y, cv.z, cv.w};
                for (int d = 0; d < A.dim; ++d) {
                    const float4 wv = *reinterpret_cast<const float4 *>(w1 + d * AT_LAT + k);
                    const float td = tp[r * 3 + d];
                    v[0] = fmaf(wv.x, td, v[0]); v[1] = fmaf(wv.y, td, v[1]);
                    v[2] = fmaf(wv.z, td, v[2]); v[3] = fmaf(wv.w, td, v[3]);
                }
                *reinterpret_cast<float4 *>(H + r * AT_SH + (k - k0)) =
                    make_float4(fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f));
            }
            __syncthreads();
            // gemm_chain reads A at in + row * s_in + 8 t for k-groups t in [64 ch, 64 ch + 64): the chunk starts at H
#pragma unroll
            for (int q = 0; q < 2; ++q) gemm_chain<2>(H - k0, AT_SH, 0, L, cb0 + q, k0 / 8, k0 / 8 + AT_HID / 8, acc[q]);
            __syncthreads();
        }
        atlas_dec_epilogue(H, acc, cb0, A.sc2 + (size_t)p * AT_HID, A.sh2 + (size_t)p * AT_HID);
        __syncthreads();
    }
    // conv_list: 512 -> 512, in place in H (every wave has read all of H before the barrier that precedes the epilogue)
    for (int l = 0; l < A.num_layers; ++l) {
        const size_t pl = (size_t)p * A.num_layers + l;
        const PackedLayer L{A.lhw + pl * AT_HID * AT_HID, AT_HID, AT_HID};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            acc[q][0] = acc[q][1] = f32x16{};
            gemm_chain<2>(H, AT_SH, 0, L, cb0 + q, 0, AT_HID / 8, acc[q]);
        }
        __syncthreads();
        atlas_dec_epilogue(H, acc, cb0, A.sch + pl * AT_HID, A.shh + pl * AT_HID);
        __syncthreads();
    }
    // last_conv 512 -> 3 on the VALU: 192 (row, coordinate) outputs x two halves of K
    {
        const float *wl = A.wl + (size_t)p * AT_HID * 3;
        if (threadIdx.x < 2 * 3 * AT_ROWS) {
            const int half = threadIdx.x / (3 * AT_ROWS), o = threadIdx.x - half * 3 * AT_ROWS;
            const int r = o / 3, d = o - 3 * r;
            const float *hr = H + r * AT_SH + half * (AT_HID / 2);
            const float *wk = wl + half * (AT_HID / 2) * 3 + d;
            float a = 0.f;
#pragma unroll 8
            for (int k = 0; k < AT_HID / 2; ++k) a = fmaf(hr[k], wk[3 * k], a);
            part[threadIdx.x] = a;
        }
        __syncthreads();
        if (threadIdx.x < 3 * AT_ROWS) {
            const int r = threadIdx.x / 3, d = threadIdx.x - 3 * r;
            if (r < live) {
                const float y = (part[threadIdx.x] + part[threadIdx.x + 3 * AT_ROWS]) + A.bl[p * 3 + d];
                const size_t P = (size_t)A.nb * A.g2;
                A.recon[((size_t)rcloud[r] * P + (size_t)p * A.g2 + rpoint[r]) * 3 + d] = y;
            }
        }
    }
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

namespace {
inline size_t at_rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// W [K][N] row-major -> 32x32x2 fragments (ae.h): dst[((cb * K/8 + t) * 64 + lane) * 4 + u] = W[8t + 4(lane>>5) + u][32cb + (lane&31)]
void at_pack(float *dst, const float *W, int K, int N) {
    const int kg = K / 8;
    for (int cb = 0; cb < N / 32; ++cb)
        for (int t = 0; t < kg; ++t)
            for (int lane = 0; lane < 64; ++lane)
                for (int u = 0; u < 4; ++u) {
                    const int k = 8 * t + 4 * (lane >> 5) + u, n = 32 * cb + (lane & 31);
                    dst[(((size_t)cb * kg + t) * 64 + lane) * 4 + u] = W[(size_t)k * N + n];
                }
}
// folded batch norm of N channels: scale, shift (with the layer's bias); no BN: scale 1, shift b
void at_fold(float *sc, float *sh, int N, const float *b, const float *g, const float *be, const float *m, const float *v) {
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
}  // namespace

extern "C" int geoadv_atlas_create(geoadv_atlas **out, const geoadv_atlas_config *cfg, const geoadv_atlas_weights *hw,
                                   const float *host_template) {
    GA_REQUIRE(out && cfg && hw && host_template, "atlas_create: null argument");
    const int NB = cfg->nb_primitives, G2 = cfg->points_per_primitive, DIM = cfg->dim_template, NL = cfg->num_layers;
    GA_REQUIRE(NB >= 1 && NB <= AT_MAX_NB, "atlas_create: nb_primitives %d out of range [1, %d]", NB, AT_MAX_NB);
    GA_REQUIRE(G2 >= 1 && G2 <= 65536, "atlas_create: points_per_primitive %d out of range [1, 65536]", G2);
    GA_REQUIRE(DIM == 2 || DIM == 3, "atlas_create: dim_template %d is not 2 or 3", DIM);
    GA_REQUIRE(cfg->bottleneck_size == AT_LAT, "atlas_create: bottleneck_size %d is not %d", cfg->bottleneck_size, AT_LAT);
    GA_REQUIRE(cfg->hidden_neurons == AT_HID, "atlas_create: hidden_neurons %d is not %d", cfg->hidden_neurons, AT_HID);
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
    std::vector<float> host;
    auto reserve = [&](size_t count) { size_t off = at_rup(host.size(), 64); host.resize(off + count, 0.f); return off; };
    size_t o_w0, o_esc[5], o_esh[5], o_pk1, o_pk2, o_lin[2];
    o_w0 = reserve(3 * 64);
    memcpy(&host[o_w0], hw->enc_w[0], sizeof(float) * 3 * 64);
    o_pk1 = reserve(64 * 128);
    at_pack(&host[o_pk1], hw->enc_w[1], 64, 128);
    o_pk2 = reserve((size_t)128 * AT_LAT);
    at_pack(&host[o_pk2], hw->enc_w[2], 128, AT_LAT);
    for (int q = 0; q < 2; ++q) {
        o_lin[q] = reserve((size_t)AT_LAT * AT_LAT);
        memcpy(&host[o_lin[q]], hw->enc_w[3 + q], sizeof(float) * AT_LAT * AT_LAT);
    }
    for (int l = 0; l < 5; ++l) {
        o_esc[l] = reserve(eout[l]);
        o_esh[l] = reserve(eout[l]);
        at_fold(&host[o_esc[l]], &host[o_esh[l]], eout[l], hw->enc_b[l], hw->enc_gamma[l], hw->enc_beta[l], hw->enc_mean[l],
                hw->enc_var[l]);
    }
    const bool bn = cfg->decoder_bn != 0;
    auto dec_bn = [&](int l, int p, int N, float *sc, float *sh) {
        const size_t o = (size_t)p * N;
        at_fold(sc, sh, N, hw->dec_b[l] + o, bn ? hw->dec_gamma[l] + o : nullptr, bn ? hw->dec_beta[l] + o : nullptr,
                bn ? hw->dec_mean[l] + o : nullptr, bn ? hw->dec_var[l] + o : nullptr);
    };
    const size_t o_tmpl = reserve((size_t)NB * G2 * DIM);
    memcpy(&host[o_tmpl], host_template, sizeof(float) * NB * G2 * DIM);
    const size_t o_w1s = reserve((size_t)NB * DIM * AT_LAT), o_s1 = reserve((size_t)NB * AT_LAT), o_t1 = reserve((size_t)NB * AT_LAT);
    const size_t o_l2w = reserve((size_t)NB * AT_LAT * AT_HID), o_sc2 = reserve((size_t)NB * AT_HID), o_sh2 = reserve((size_t)NB * AT_HID);
    const size_t nh = (size_t)NB * NL;
    const size_t o_lhw = reserve(nh * AT_HID * AT_HID + 1), o_sch = reserve(nh * AT_HID + 1), o_shh = reserve(nh * AT_HID + 1);
    const size_t o_wl = reserve((size_t)NB * AT_HID * 3), o_bl = reserve((size_t)NB * 3);
    for (int p = 0; p < NB; ++p) {
        float *s1 = &host[o_s1 + (size_t)p * AT_LAT], *t1 = &host[o_t1 + (size_t)p * AT_LAT];
        dec_bn(0, p, AT_LAT, s1, t1);
        const float *w1 = hw->dec_w[0] + (size_t)p * DIM * AT_LAT;
        for (int d = 0; d < DIM; ++d)
            for (int k = 0; k < AT_LAT; ++k) host[o_w1s + ((size_t)p * DIM + d) * AT_LAT + k] = s1[k] * w1[(size_t)d * AT_LAT + k];
        at_pack(&host[o_l2w + (size_t)p * AT_LAT * AT_HID], hw->dec_w[1] + (size_t)p * AT_LAT * AT_HID, AT_LAT, AT_HID);
        dec_bn(1, p, AT_HID, &host[o_sc2 + (size_t)p * AT_HID], &host[o_sh2 + (size_t)p * AT_HID]);
        for (int l = 0; l < NL; ++l) {
            const size_t pl = (size_t)p * NL + l;
            at_pack(&host[o_lhw + pl * AT_HID * AT_HID], hw->dec_w[2 + l] + (size_t)p * AT_HID * AT_HID, AT_HID, AT_HID);
            dec_bn(2 + l, p, AT_HID, &host[o_sch + pl * AT_HID], &host[o_shh + pl * AT_HID]);
        }
        memcpy(&host[o_wl + (size_t)p * AT_HID * 3], hw->dec_w[NDL - 1] + (size_t)p * AT_HID * 3, sizeof(float) * AT_HID * 3);
        memcpy(&host[o_bl + (size_t)p * 3], hw->dec_b[NDL - 1] + (size_t)p * 3, sizeof(float) * 3);
    }
    geoadv_atlas *m = new geoadv_atlas();
    m->cfg = *cfg;
    const size_t bytes = sizeof(float) * host.size();
    if (hipMalloc(&m->arena, bytes) != hipSuccess) {
        delete m;
        set_error("atlas_create: hipMalloc of %zu bytes failed", bytes);
        return GEOADV_ENOMEM;
    }
    const hipError_t e = hipMemcpy(m->arena, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->arena);
        delete m;
        set_error("atlas_create: upload failed: %s", hipGetErrorString(e));
        return GEOADV_EHIP;
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
AtlasScratch carve_atlas(void *base, int bc, int nb) {
    AtlasScratch s;
    char *p = static_cast<char *>(base);
    auto take = [&](size_t bytes) { char *q = p; p += at_rup(bytes, 256); return q; };
    s.keys = reinterpret_cast<unsigned *>(take(sizeof(unsigned) * (size_t)bc * AT_LAT));
    s.h1 = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * AT_LAT));
    s.z = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * AT_LAT));
    s.c = reinterpret_cast<float *>(take(sizeof(float) * (size_t)bc * nb * AT_LAT));
    s.bytes = (size_t)(p - static_cast<char *>(base));
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
    const int tiles = cdiv(n, AT_ROWS);
    void *aligned = reinterpret_cast<void *>(at_rup(reinterpret_cast<size_t>(workspace), 256));
    const int bc = atlas_chunk(b, NB);
    const AtlasScratch s = carve_atlas(aligned, bc, NB);
    int slices = 1;    // small batches split conv3's 1024 columns over up to 4 workgroups per tile (as classifier.hip)
    while (slices < 4 && (size_t)tiles * b * slices < 2 * kCUs) slices *= 2;

    AtlasEncArgs ea{};
    ea.w0 = atlas->e_w0; ea.sc0 = atlas->e_sc[0]; ea.sh0 = atlas->e_sh[0];
    ea.l1 = PackedLayer{atlas->e_pk1, 64, 128}; ea.sc1 = atlas->e_sc[1]; ea.sh1 = atlas->e_sh[1];
    ea.l2 = PackedLayer{atlas->e_pk2, 128, AT_LAT}; ea.sc2 = atlas->e_sc[2]; ea.sh2 = atlas->e_sh[2];
    ea.keys = s.keys; ea.n = n; ea.slices = slices;
    for (int c0 = 0; c0 < b; c0 += bc) {
        const int nbc = std::min(bc, b - c0);
        GA_HIP(hipMemsetAsync(s.keys, 0, sizeof(unsigned) * (size_t)nbc * AT_LAT, st));
        ea.x = pc + (size_t)c0 * n * 3;
        hipLaunchKernelGGL(atlas_enc_kernel, dim3(tiles, nbc, slices), dim3(AT_THREADS), 0, st, ea);
        GA_LAUNCH_CHECK();
        const dim3 fg(AT_LAT / 64, cdiv(nbc, AT_FC_CLOUDS));
        AtlasFcArgs fa{};
        fa.keys = s.keys; fa.w = atlas->e_lin[0]; fa.sc = atlas->e_sc[3]; fa.sh = atlas->e_sh[3];
        fa.out = s.h1; fa.nb = NB; fa.b = nbc;
        hipLaunchKernelGGL(atlas_fc_kernel, fg, dim3(AT_FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        float *z = latent ? latent + (size_t)c0 * AT_LAT : s.z;
        fa.keys = nullptr; fa.in = s.h1; fa.w = atlas->e_lin[1]; fa.sc = atlas->e_sc[4]; fa.sh = atlas->e_sh[4];
        fa.out = z; fa.s1 = atlas->s1; fa.t1 = atlas->t1; fa.c = s.c;
        hipLaunchKernelGGL(atlas_fc_kernel, fg, dim3(AT_FC_THREADS), 0, st, fa);
        GA_LAUNCH_CHECK();
        AtlasDecArgs da{};
        da.tmpl = atlas->tmpl; da.w1s = atlas->w1s; da.c = s.c;
        da.l2w = atlas->l2w; da.sc2 = atlas->sc2; da.sh2 = atlas->sh2;
        da.lhw = atlas->lhw; da.sch = atlas->sch; da.shh = atlas->shh;
        da.wl = atlas->wl; da.bl = atlas->bl;
        da.recon = recon + (size_t)c0 * P * 3;
        da.b = nbc; da.nb = NB; da.g2 = G2; da.dim = cf.dim_template; da.num_layers = cf.num_layers;
        da.tiles = cdiv(nbc * G2, AT_ROWS);
        da.blocks = da.tiles * NB;
        const int grid = cdiv(da.blocks, 8) * 8;
        hipLaunchKernelGGL(atlas_decoder_kernel, dim3(grid), dim3(AT_THREADS), AT_DEC_LDS, st, da);
        GA_LAUNCH_CHECK();
    }
    return GEOADV_OK;
}
