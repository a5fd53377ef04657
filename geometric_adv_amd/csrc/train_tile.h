// The GEMM shared by the layer-by-layer training steps (cls_train.hip, fold_train.hip, atlas_train.hip): the strided fp32
// product on v_mfma_f32_32x32x2_f32 with its fixed-order split-K, and its host launch.  The column-sum and batch-norm kernels
// the three steps share are in train_bn.h.  Every kernel is `static`: each translation unit that includes this header gets
// its own copy.
#pragma once
#include "mfma_tile.h"

namespace geoadv {

constexpr int CT_TILE = 64, CT_KT = 32, CT_THREADS = 256, CT_LDS = CT_TILE + 4;
constexpr size_t CT_PARTIAL_FLOATS = (size_t)16 << 20;     // split-K partials (64 MB)

// C[z] = alpha * sum_k A(i, k) B(k, j) (+ bias[j]) (+ C[z] if accumulate); element (i, k) of batch z at
// A[z * sAz + i * sAi + k * sAk], (k, j) at B[z * sBz + k * sBk + j * sBj], C row-major with row stride ldc.
// ksplit > 1: block z * ksplit + s writes the partial of its K range to P[(s * batch + z) * M * N] and ct_splitk_reduce adds
// the ksplit partials in ascending order in double.
struct GemmArgs {
    const float *A; long long sAi, sAk, sAz;
    const float *B; long long sBk, sBj, sBz;
    float *C; long long ldc, sCz;
    const float *bias;
    float alpha;
    int M, N, K, batch, ksplit, accumulate;
    float *P;
};

static __global__ __launch_bounds__(CT_THREADS) void ct_gemm_kernel(GemmArgs g) {
    __shared__ float As[CT_KT][CT_LDS], Bs[CT_KT][CT_LDS];
    const int z = blockIdx.z / g.ksplit, s = blockIdx.z % g.ksplit;
    const int i0 = blockIdx.y * CT_TILE, j0 = blockIdx.x * CT_TILE;
    const int kchunk = ((g.K + g.ksplit - 1) / g.ksplit + CT_KT - 1) / CT_KT * CT_KT;
    const int kb = s * kchunk, ke = min(g.K, kb + kchunk);
    const float *A = g.A + z * g.sAz, *B = g.B + z * g.sBz;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, h = lane >> 5, li = lane & 31;
    const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
    const bool a_kfast = g.sAk == 1, b_jfast = g.sBj == 1;
    f32x16 acc = {};
    for (int k0 = kb; k0 < ke; k0 += CT_KT) {
#pragma unroll
        for (int q = 0; q < CT_KT * CT_TILE / CT_THREADS; ++q) {
            const int e = t + q * CT_THREADS;
            int r, k;
            if (a_kfast) { r = e / CT_KT; k = e % CT_KT; } else { k = e / CT_TILE; r = e % CT_TILE; }
            const int gi = i0 + r, gk = k0 + k;
            As[k][r] = (gi < g.M && gk < ke) ? A[gi * g.sAi + gk * g.sAk] : 0.f;
            int c, kk;
            if (b_jfast) { kk = e / CT_TILE; c = e % CT_TILE; } else { c = e / CT_KT; kk = e % CT_KT; }
            const int gj = j0 + c, gk2 = k0 + kk;
            Bs[kk][c] = (gj < g.N && gk2 < ke) ? B[gk2 * g.sBk + gj * g.sBj] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < CT_KT; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + h][wr + li], Bs[kk + h][wc + li], acc, 0, 0, 0);
        __syncthreads();
    }
    const int col = j0 + wc + li;
    if (col >= g.N) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = i0 + wr + acc_row(r, h);
        if (row >= g.M) continue;
        if (g.ksplit > 1) {
            g.P[((size_t)(s * g.batch + z) * g.M + row) * g.N + col] = acc[r];
        } else {
            float v = acc[r] * g.alpha;
            if (g.bias) v = v + g.bias[col];
            float *c = g.C + z * g.sCz + (size_t)row * g.ldc + col;
            *c = g.accumulate ? *c + v : v;
        }
    }
}

static __global__ __launch_bounds__(256) void ct_splitk_reduce(GemmArgs g) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t per = (size_t)g.M * g.N;
    if (e >= per * g.batch) return;
    const int z = (int)(e / per);
    const int row = (int)((e % per) / g.N), col = (int)(e % g.N);
    double a = 0.0;
    for (int s = 0; s < g.ksplit; ++s) a += (double)g.P[(size_t)s * per * g.batch + e];
    float v = (float)a * g.alpha;
    if (g.bias) v = v + g.bias[col];
    float *c = g.C + z * g.sCz + (size_t)row * g.ldc + col;
    *c = g.accumulate ? *c + v : v;
}

// The split of the K range ct_launch_gemm takes for a shape: more than 1 only when the tiles alone would leave most of the
// device idle; it depends on the shape alone, so a step is reproducible.
inline int ct_ksplit(int M, int N, int K, int batch) {
    int ks = 1;
    const long long blocks = (long long)cdiv(N, CT_TILE) * cdiv(M, CT_TILE) * batch;
    if (blocks < 512 && K >= 4 * CT_KT) {
        ks = (int)std::min<long long>(cdiv(K, 4 * CT_KT), 512 / blocks);
        while (ks > 1 && (size_t)ks * batch * M * N > CT_PARTIAL_FLOATS) --ks;
    }
    return ks;
}

// Launches the GEMM (and its split-K reduction over `partials`, CT_PARTIAL_FLOATS floats) with the split of ct_ksplit.
inline hipError_t ct_launch_gemm(GemmArgs g, float *partials, hipStream_t st) {
    const int gx = cdiv(g.N, CT_TILE), gy = cdiv(g.M, CT_TILE);
    const int ks = ct_ksplit(g.M, g.N, g.K, g.batch);
    g.ksplit = ks;
    g.P = partials;
    hipLaunchKernelGGL(ct_gemm_kernel, dim3(gx, gy, g.batch * ks), dim3(CT_THREADS), 0, st, g);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess && ks > 1) {
        const size_t total = (size_t)g.batch * g.M * g.N;
        hipLaunchKernelGGL(ct_splitk_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, g);
        err = hipGetLastError();
    }
    return err;
}

}  // namespace geoadv
