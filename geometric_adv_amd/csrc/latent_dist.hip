// All-pairs Euclidean distance of latent codes: out[i, j] = || a[i] - b[j] ||_2, the matrix behind the latent-space target
// choice (attacker/prepare_indices_for_attack.py:89-101, src/general_utils.py:94-106).  The matrix is used only through an
// argsort, so it carries the reference's BITS: np.linalg.norm(s - t, axis=-1) of float32 rows of d <= 128 elements is
//     diff = a[k] - b[k];  sq = diff * diff (rounded on its own);  numpy's pairwise sum of one contiguous run of sq:
//         d < 8 : res = 0; res += sq[k] in order
//         else  : eight accumulators r[j] = sq[j]; r[j] += sq[8 g + j] for every further full group of eight;
//                 res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)); the last d mod 8 elements added to res in order
//     sqrt(res), correctly rounded.
// Here the accumulators start at +0 and every group is ADDED: 0 + sq is sq (a square is never -0), and with no full group the
// combine of eight zeros is the +0 the short form starts from, so one code path gives both forms.  (a - b)^2 and (b - a)^2 are
// the same bits: the matrix of b == a is exactly symmetric with a +0 diagonal.  Plain fp32 VALU, no FMA (-ffp-contract=off), fp32
// denormals kept and a correctly rounded square root (both hipcc's defaults).
//
// One 256-thread workgroup per 64 x 64 tile of out; a lane owns 4 rows x 4 columns with their 8 accumulators each (128 VGPRs).
// The rows of a and b go through LDS in chunks of 64 k, TRANSPOSED ([k][row], 68 floats per k): for one k every lane reads its 4
// rows and its 4 columns as one ds_read_b128 each -- the 16 column quads of a wave are 256 contiguous bytes (all 64 banks once),
// the row quads broadcast -- and the accumulator index k mod 8 is a compile-time constant of the unrolled group.  The staging
// store puts 16 consecutive k of 2 rows into each 32-lane group: bank (4 k + row) mod 32, 2-way, which a ds_write_b32 hides.
// Rows past na / nb and k past d are staged as zeros and never written out / never summed; nothing outside a and b is read.
#include "common.h"

namespace geoadv {

constexpr int LD_TILE = 64;         // rows of a and of b per workgroup
constexpr int LD_KC = 64;           // k per LDS chunk (a multiple of 8: a group of eight never straddles two chunks)
constexpr int LD_STRIDE = 68;       // floats per k in LDS: 16-byte aligned quads, and 4 k + row walks the 32 store banks
constexpr int LD_THREADS = 256;
constexpr int LD_MAX_D = 128;       // numpy sums a longer run in blocks of 128 (another order)
constexpr int LD_MAX_GRID_Y = 65535;

__device__ __forceinline__ void ld_stage(float *s, const float *src, int rows, int row0, int d, int k0, int t) {
    // element e of the chunk: k = 16 (e >> 10) + (e & 15), row = (e >> 4) & 63
#pragma unroll 4
    for (int it = 0; it < LD_TILE * LD_KC / LD_THREADS; ++it) {
        const int kk = 16 * (it >> 2) + (t & 15), row = (t >> 4) + 16 * (it & 3);
        const bool ok = row0 + row < rows && k0 + kk < d;
        s[kk * LD_STRIDE + row] = ok ? src[(size_t)(row0 + row) * d + k0 + kk] : 0.0f;
    }
}

__global__ __launch_bounds__(LD_THREADS) void latent_dist_kernel(int na, int nb, int d, const float *a, const float *b, float *out) {
    __shared__ __attribute__((aligned(16))) float sa[LD_KC * LD_STRIDE];
    __shared__ __attribute__((aligned(16))) float sb[LD_KC * LD_STRIDE];
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const int i0 = blockIdx.y * LD_TILE, j0 = blockIdx.x * LD_TILE;
    const int groups = d >> 3;

    float r[4][4][8];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[p][q][j] = 0.0f;

    int k0 = 0;
    for (;;) {
        ld_stage(sa, a, na, i0, d, k0, t);
        ld_stage(sb, b, nb, j0, d, k0, t);
        __syncthreads();
        const int gend = min(LD_KC / 8, groups - (k0 >> 3));        // full groups of eight in this chunk (<= 0: none)
        for (int g = 0; g < gend; ++g) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float4 av = *reinterpret_cast<const float4 *>(&sa[(8 * g + j) * LD_STRIDE + 4 * ty]);
                const float4 bv = *reinterpret_cast<const float4 *>(&sb[(8 * g + j) * LD_STRIDE + 4 * tx]);
                const float ar[4] = {av.x, av.y, av.z, av.w}, bc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float diff = ar[p] - bc[q];
                        const float sq = diff * diff;
                        r[p][q][j] = r[p][q][j] + sq;
                    }
            }
        }
        if (k0 + LD_KC >= d) break;         // the last chunk stays in LDS for the tail below
        k0 += LD_KC;
        __syncthreads();
    }

    float res[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float *x = r[p][q];
            res[p][q] = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
        }
    // the last d mod 8 elements, one by one; 8 * groups and d - 1 lie in the same chunk (the one in LDS)
    for (int k = 8 * groups; k < d; ++k) {
        const float4 av = *reinterpret_cast<const float4 *>(&sa[(k - k0) * LD_STRIDE + 4 * ty]);
        const float4 bv = *reinterpret_cast<const float4 *>(&sb[(k - k0) * LD_STRIDE + 4 * tx]);
        const float ar[4] = {av.x, av.y, av.z, av.w}, bc[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float diff = ar[p] - bc[q];
                const float sq = diff * diff;
                res[p][q] = res[p][q] + sq;
            }
    }

#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int i = i0 + 4 * ty + p;
        if (i >= na) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + 4 * tx + q;
            if (j < nb) out[(size_t)i * nb + j] = sqrtf(res[p][q]);
        }
    }
}

}  // namespace geoadv

using namespace geoadv;

extern "C" int geoadv_latent_dist_matrix(int na, int nb, int d, const float *a, const float *b, float *out, void *stream) {
    GA_REQUIRE(na >= 0 && nb >= 0, "latent_dist_matrix: bad dimensions (na=%d, nb=%d)", na, nb);
    GA_REQUIRE(d >= 1 && d <= LD_MAX_D, "latent_dist_matrix: d=%d is not supported: 1 <= d <= %d", d, LD_MAX_D);
    if (na == 0 || nb == 0) return GEOADV_OK;
    GA_REQUIRE(a && b && out, "latent_dist_matrix: null pointer");
    GA_REQUIRE(cdiv(na, LD_TILE) <= LD_MAX_GRID_Y, "latent_dist_matrix: na=%d is too large (at most %d rows per call)", na,
               LD_MAX_GRID_Y * LD_TILE);
    latent_dist_kernel<<<dim3(cdiv(nb, LD_TILE), cdiv(na, LD_TILE)), LD_THREADS, 0, as_stream(stream)>>>(na, nb, d, a, b, out);
    GA_LAUNCH_CHECK();
    return GEOADV_OK;
}
