// cgemm_f64.h -- the batched fp64 (complex) GEMM of the separable DFT operators, shared by classic.hip (frequency extrapolation) and
// metrics.hip (the high-frequency energy ratio) and eda.hip (the DCT and the accumulated spectra), with the cached full DFT operator.
#pragma once
#include "common.h"

#include <algorithm>
#include <cmath>

namespace {

enum { CG_STORE = 0, CG_ABS = 1, CG_MASKED_ABS_SUM = 2 };

// C[b] (M x N, row-major, batch stride scb) = A[b] (M x K) . B[b] (K x N) with element strides (sa_m, sa_k), (sb_k, sb_n) and batch strides
// sab, sbb (0: shared).  Complex where AI / BI say the operand has an imaginary part.  EPI: CG_STORE writes C (cr, and ci when complex);
// CG_ABS writes |C| to cr only; CG_MASKED_ABS_SUM writes, per workgroup, the sum of |C| over the elements (m, n) whose fftshift-ed offset
// from the centre (M / 2, N / 2) is longer than mask_r, to cr[b * scb + blockIdx.y * gridDim.x + blockIdx.x] (each thread's 16 in a fixed
// order, then a fixed LDS tree: the same bits on every run).  64 x 64 tile per 256-thread workgroup, 4 x 4 outputs per thread
// (rows tr + 16 i, cols tc + 16 j), K in steps of 16 through LDS.
constexpr int GT = 64, GK = 16;

template <bool AI, bool BI, int EPI>
__global__ void __launch_bounds__(256) cgemm_f64_kernel(int M, int N, int K, const double* ar, const double* ai, int64_t sa_m, int64_t sa_k, int64_t sab,
                                                        const double* br, const double* bi, int64_t sb_k, int64_t sb_n, int64_t sbb,
                                                        double* cr, double* ci, int64_t scb, double mask_r) {
    constexpr bool CPLX = AI || BI;
    __shared__ double Ar[GK][GT + 1], Ai[AI ? GK : 1][GT + 1], Br[GK][GT + 1], Bi[BI ? GK : 1][GT + 1];
    const int64_t b = blockIdx.z;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int tr = threadIdx.x >> 4, tc = threadIdx.x & 15;
    ar += b * sab; br += b * sbb;
    if (AI) ai += b * sab;
    if (BI) bi += b * sbb;
    double accr[4][4] = {}, acci[4][4] = {};
    for (int k0 = 0; k0 < K; k0 += GK) {
        for (int q = threadIdx.x; q < GT * GK; q += 256) {
            const int kk = q & (GK - 1), mm = q >> 4;                 // A tile: (m0 + mm, k0 + kk)
            const int gm = m0 + mm, gk = k0 + kk;
            const bool ok = gm < M && gk < K;
            const int64_t off = (int64_t)gm * sa_m + (int64_t)gk * sa_k;
            Ar[kk][mm] = ok ? ar[off] : 0.0;
            if (AI) Ai[kk][mm] = ok ? ai[off] : 0.0;
            const int nn = q & (GT - 1), kb = q >> 6;                  // B tile: (k0 + kb, n0 + nn)
            const int gn = n0 + nn, gkb = k0 + kb;
            const bool okb = gn < N && gkb < K;
            const int64_t offb = (int64_t)gkb * sb_k + (int64_t)gn * sb_n;
            Br[kb][nn] = okb ? br[offb] : 0.0;
            if (BI) Bi[kb][nn] = okb ? bi[offb] : 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < GK; ++kk) {
            double a_r[4], a_i[4], b_r[4], b_i[4];
            for (int u = 0; u < 4; ++u) {
                a_r[u] = Ar[kk][tr + 16 * u]; a_i[u] = AI ? Ai[kk][tr + 16 * u] : 0.0;
                b_r[u] = Br[kk][tc + 16 * u]; b_i[u] = BI ? Bi[kk][tc + 16 * u] : 0.0;
            }
            for (int u = 0; u < 4; ++u)
                for (int v = 0; v < 4; ++v) {
                    accr[u][v] = fma(a_r[u], b_r[v], accr[u][v]);
                    if (AI && BI) accr[u][v] = fma(-a_i[u], b_i[v], accr[u][v]);
                    if (BI) acci[u][v] = fma(a_r[u], b_i[v], acci[u][v]);
                    if (AI) acci[u][v] = fma(a_i[u], b_r[v], acci[u][v]);
                }
        }
        __syncthreads();
    }
    if (EPI == CG_MASKED_ABS_SUM) {
        double s = 0.0;
        for (int u = 0; u < 4; ++u)
            for (int v = 0; v < 4; ++v) {
                const int gm = m0 + tr + 16 * u, gn = n0 + tc + 16 * v;
                if (gm >= M || gn >= N) continue;
                const int dy = (gm + M / 2) % M - M / 2, dx = (gn + N / 2) % N - N / 2;
                if (sqrt((double)dy * dy + (double)dx * dx) > mask_r) s += CPLX ? hypot(accr[u][v], acci[u][v]) : fabs(accr[u][v]);
            }
        double* red = &Ar[0][0];                               // GK * (GT + 1) >= 256 doubles, free after the last barrier of the K loop
        red[threadIdx.x] = s;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) cr[b * scb + (int64_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0];
        return;
    }
    for (int u = 0; u < 4; ++u)
        for (int v = 0; v < 4; ++v) {
            const int gm = m0 + tr + 16 * u, gn = n0 + tc + 16 * v;
            if (gm >= M || gn >= N) continue;
            const int64_t o = b * scb + (int64_t)gm * N + gn;
            if (EPI == CG_ABS) cr[o] = CPLX ? hypot(accr[u][v], acci[u][v]) : fabs(accr[u][v]);
            else {
                cr[o] = accr[u][v];
                if (CPLX) ci[o] = acci[u][v];
            }
        }
}

template <int EPI>
void cgemm_dispatch(bool a_im, bool b_im, dim3 grid, hipStream_t st, int M, int N, int K, const double* ar, const double* ai, int64_t sa_m, int64_t sa_k,
                    int64_t sab, const double* br, const double* bi, int64_t sb_k, int64_t sb_n, int64_t sbb, double* cr, double* ci, int64_t scb,
                    double mask_r = 0.0) {
#define SR_CGEMM(AI_, BI_) hipLaunchKernelGGL((cgemm_f64_kernel<AI_, BI_, EPI>), grid, dim3(256), 0, st, M, N, K, ar, ai, sa_m, sa_k, sab, br, bi, sb_k, sb_n, sbb, cr, ci, scb, mask_r)
    if (a_im && b_im) SR_CGEMM(true, true);
    else if (a_im) SR_CGEMM(true, false);
    else if (b_im) SR_CGEMM(false, true);
    else SR_CGEMM(false, false);
#undef SR_CGEMM
}

// A_N[k][x] = exp(-2 pi i k x / N), the phase reduced exactly in integers; [N][N] real parts, then [N][N] imaginary parts
__global__ void dft_full_operator_kernel(int N, double* re, double* im) {
    const int64_t total = (int64_t)N * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t m = ((i / N) * (i % N)) % N;
        double sn, cs;
        sincospi(2.0 * (double)m / (double)N, &sn, &cs);
        re[i] = cs;
        im[i] = -sn;
    }
}

// the operator of one N, built once per context; its dft_ops key is -N (frequency extrapolation's keys (N << 32) | n are positive)
int dft_full_operator(sr_ctx* ctx, int N, hipStream_t st, const double** re, const double** im) {
    const int64_t key = -(int64_t)N;
    auto it = ctx->dft_ops.find(key);
    if (it == ctx->dft_ops.end()) {
        const int64_t nel = (int64_t)N * N;
        double* p = static_cast<double*>(ctx->dalloc(sizeof(double) * (size_t)nel * 2));
        if (!p) return SR_ERR_OOM;
        hipLaunchKernelGGL(dft_full_operator_kernel, dim3((unsigned)std::min<int64_t>((nel + 255) / 256, 65535)), dim3(256), 0, st, N, p, p + nel);
        SR_HIP(ctx, hipGetLastError());
        SR_HIP(ctx, hipStreamSynchronize(st));      // once per size: later calls may come on other streams
        it = ctx->dft_ops.emplace(key, p).first;
    }
    *re = it->second;
    *im = it->second + (int64_t)N * N;
    return SR_OK;
}

}  // namespace
