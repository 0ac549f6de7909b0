// head_train.hip -- the per-batch work of FineTunedVGG16.fit (reference VGG16_model.py:111-157) that is not the frozen conv base.
//
//   sr_affine_warp: keras ImageDataGenerator's transform as the host's FineTunedVGG16._augment computes it (VGG16_model.py:129-134): output
//     pixel o of batch image b samples image idx[b] of the device-resident set at rot_b @ o + off_b, bilinear (scipy order=1), every tap index
//     clamped (mode="nearest"), then the horizontal flip.  The gather of the batch's rows of the epoch permutation is fused into it.  The
//     coordinates are fp32 double-float sums of the host's fp64 parameters split into hi + lo halves, so a sample point is exact to far below
//     an fp32 ulp of the coordinate and an integer one (identity, flip, integer shift) is exact: those outputs are bitwise copies.  Memory-bound:
//     each thread writes 4 consecutive NHWC floats with one 16-byte store when H W C is a multiple of 4.
//   sr_dense_head_step: GAP -> Dropout -> Dense 512->256 ReLU -> Dropout -> Dense 256->C softmax with mean sparse CCE + l2 sum(k1^2), forward
//     and backward in two launches:
//     1. rows: one workgroup per HROWS rows.  x0 = g * m0 / keep staged in LDS, z1 = x0 k1 + b1 (thread j owns hidden unit j for all the rows,
//        k1 read once per workgroup), x1 = relu(z1) * m1 / keep, logits, softmax, clipped CE and the argmax per row, dz2 = (p - onehot) / n and
//        dz1 = (dz2 k2^T) * m1 / keep * [z1 > 0].  Workgroup 0 also sums k1^2 (fp64) for the l2 term of the loss.
//     2. grads: one thread per parameter of the flat head bucket (dense kernel, dense bias, predictions kernel, predictions bias -- the layout
//        of train.ParamBucket), the sum over the batch rows in row order; then one thread sums the rows' losses and hits (fp64, row order).
//     No float atomics: the gradients and the statistics are the same bits on every run.  At 32 x 512 x 256 the products are 4 MFLOP per step,
//     ~1 us of VALU work spread over the grid: the step is bound by its launches, not by its arithmetic.
//   sr_dense_head_step_dx: the same two launches (the same kernels: the same bits in grads and stats) and a third for the gradient at the
//     features, dfeats = (dz1 k1^T) * m0 / keep -- what the fine-tuned conv base's backward pass starts from.
//   sr_pool_gap_bwd: GlobalAveragePooling2D, MaxPooling2D(2,2) and the last conv's ReLU backward in one launch: dfeats [B,C] -> dz [B,H,W,C] at
//     that conv's pre-activation, bit for bit the GAP spread (dfeats / ((H/2)(W/2))), sr_maxpool2_bwd and SR_ELT_RELU_BWD one after the other.
#include "common.h"
#include "fp_sep.h"
#include "warp_sample.h"

#include <algorithm>
#include <cmath>
#include <string>

namespace {

constexpr int HIN = 512, HHID = 256, HROWS = 8;

template <int VEC>
__global__ void __launch_bounds__(256) affine_warp_kernel(const float* __restrict__ x, int N, int H, int W, int C, const int* __restrict__ idx,
                                                          const float* __restrict__ prm, float* __restrict__ y) {
    const int b = blockIdx.y;
    const int64_t per = (int64_t)H * W * C;
    const int src = idx[b];
    const float* p = prm + (int64_t)b * WARP_PRM;
    float hi[6], lo[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { hi[k] = p[k]; lo[k] = p[6 + k]; }
    const bool flip = p[12] != 0.f;
    const bool ok = src >= 0 && src < N;
    const float* xi = x + (ok ? (int64_t)src : 0) * per;
    float* yo = y + (int64_t)b * per;
    for (int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC; e0 < per; e0 += (int64_t)gridDim.x * 256 * VEC) {
        float out[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const int64_t e = e0 + q;
            float val = __int_as_float(0x7fc00000);   // NaN: an index outside the image set reads nothing
            if (ok && e < per) {
                const int64_t pix = e / C;
                const int c = (int)(e - pix * C);
                const int oy = (int)(pix / W);
                int ox = (int)(pix - (int64_t)oy * W);
                if (flip) ox = W - 1 - ox;
                const WarpTaps t = warp_taps(hi, lo, oy, ox, H, W);
                const float v00 = xi[((int64_t)t.ya * W + t.xa) * C + c], v01 = xi[((int64_t)t.ya * W + t.xb) * C + c];
                const float v10 = xi[((int64_t)t.yb * W + t.xa) * C + c], v11 = xi[((int64_t)t.yb * W + t.xb) * C + c];
                val = bilerp(v00, v01, v10, v11, t.ty, t.tx);
            }
            out[q] = val;
        }
        if constexpr (VEC == 4) {
            *reinterpret_cast<f32x4*>(yo + e0) = f32x4{out[0], out[1], out[2], out[3]};
        } else {
            yo[e0] = out[0];
        }
    }
}

struct HeadWork {
    float *x0, *x1, *dz1, *dz2;       // [n,512] [n,256] [n,256] [n,C]  (dz2 holds the logits, then p, then dz2)
    double* loss;                     // [n]
    int* hit;                         // [n]
};

size_t align256(size_t b) { return (b + 255) / 256 * 256; }

HeadWork head_work(void* w, int n, int C) {
    char* p = static_cast<char*>(w);
    HeadWork h;
    h.x0 = reinterpret_cast<float*>(p); p += align256(sizeof(float) * (size_t)n * HIN);
    h.x1 = reinterpret_cast<float*>(p); p += align256(sizeof(float) * (size_t)n * HHID);
    h.dz1 = reinterpret_cast<float*>(p); p += align256(sizeof(float) * (size_t)n * HHID);
    h.dz2 = reinterpret_cast<float*>(p); p += align256(sizeof(float) * (size_t)n * C);
    h.loss = reinterpret_cast<double*>(p); p += align256(sizeof(double) * (size_t)n);
    h.hit = reinterpret_cast<int*>(p);
    return h;
}

int64_t head_work_bytes(int n, int C) {
    return (int64_t)(align256(sizeof(float) * (size_t)n * HIN) + 2 * align256(sizeof(float) * (size_t)n * HHID) + align256(sizeof(float) * (size_t)n * C) +
                     align256(sizeof(double) * (size_t)n) + align256(sizeof(int) * (size_t)n));
}

__global__ void __launch_bounds__(256) head_rows_kernel(const float* __restrict__ g, int n, int C, const int* __restrict__ labels,
                                                        const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, float kscale,
                                                        const float* __restrict__ prm, int train, HeadWork wk, double* __restrict__ stats) {
    const float* k1 = prm;
    const float* b1 = k1 + HIN * HHID;
    const float* k2 = b1 + HHID;
    const float* b2 = k2 + (int64_t)HHID * C;
    __shared__ float sx0[HROWS][HIN];
    __shared__ float sx1[HROWS][HHID];
    __shared__ double sred[256];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * HROWS;
    const int nr = min(HROWS, n - r0);

    for (int e = tid; e < HROWS * HIN; e += 256) {
        const int r = e / HIN, i = e - r * HIN;
        float v = 0.f;
        if (r < nr) {
            const int64_t o = (int64_t)(r0 + r) * HIN + i;
            v = g[o];
            if (m0) v = m0[o] ? mul_sep(v, kscale) : 0.f;
            if (train) wk.x0[o] = v;
        }
        sx0[r][i] = v;
    }
    __syncthreads();

    // z1 = x0 k1 + b1 for the workgroup's rows; thread j = hidden unit j
    const int j = tid;
    float acc[HROWS];
#pragma unroll
    for (int r = 0; r < HROWS; ++r) acc[r] = 0.f;
    double sq = 0.0;
    const bool l2_wg = blockIdx.x == 0;
    for (int i = 0; i < HIN; ++i) {
        const float w = k1[(int64_t)i * HHID + j];
        if (l2_wg) sq = fma((double)w, (double)w, sq);
#pragma unroll
        for (int r = 0; r < HROWS; ++r) acc[r] = __fmaf_rn(sx0[r][i], w, acc[r]);
    }
    float z1[HROWS], f1[HROWS];               // f1: the factor of dz1 = dx1 * m1 / keep * [z1 > 0]
#pragma unroll
    for (int r = 0; r < HROWS; ++r) {
        z1[r] = add_sep(acc[r], b1[j]);
        float a = fmaxf(z1[r], 0.f);
        float m = 1.f;
        if (m1 && r < nr) m = m1[(int64_t)(r0 + r) * HHID + j] ? kscale : 0.f;
        a = mul_sep(a, m);
        f1[r] = z1[r] > 0.f ? m : 0.f;
        sx1[r][j] = a;
        if (train && r < nr) wk.x1[(int64_t)(r0 + r) * HHID + j] = a;
    }
    if (l2_wg) {                              // sum k1^2 in a fixed tree order
        sred[tid] = sq;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) sred[tid] += sred[tid + s];
            __syncthreads();
        }
        if (tid == 0) stats[2] = sred[0];
    }
    __syncthreads();

    // logits of every (row, class) of the workgroup
    for (int e = tid; e < nr * C; e += 256) {
        const int r = e / C, c = e - r * C;
        float s = 0.f;
        for (int q = 0; q < HHID; ++q) s = __fmaf_rn(sx1[r][q], k2[(int64_t)q * C + c], s);
        wk.dz2[(int64_t)(r0 + r) * C + c] = add_sep(s, b2[c]);
    }
    __syncthreads();

    // softmax, clipped CE and argmax: one thread per row
    if (tid < nr) {
        const int r = r0 + tid;
        float* z = wk.dz2 + (int64_t)r * C;
        float mx = z[0];
        for (int c = 1; c < C; ++c) mx = fmaxf(mx, z[c]);
        float sum = 0.f;
        for (int c = 0; c < C; ++c) { const float ex = expf(sub_sep(z[c], mx)); z[c] = ex; sum = add_sep(sum, ex); }
        int am = 0;
        float pm = -1.f;
        for (int c = 0; c < C; ++c) { const float p = __fdiv_rn(z[c], sum); z[c] = p; if (p > pm) { pm = p; am = c; } }
        const int y = labels[r];
        double l = NAN;
        int hit = 0;
        if (y >= 0 && y < C) {
            l = -log(fmin(fmax((double)z[y], 1e-7), 1.0 - 1e-7));
            hit = am == y;
            if (train) z[y] = sub_sep(z[y], 1.f);
        }
        if (train) for (int c = 0; c < C; ++c) z[c] = __fdiv_rn(z[c], (float)n);
        wk.loss[r] = l;
        wk.hit[r] = hit;
    }
    if (!train) return;
    __syncthreads();

    // dz1 = (dz2 k2^T) * m1 / keep * [z1 > 0]
    for (int r = 0; r < nr; ++r) {
        const float* d = wk.dz2 + (int64_t)(r0 + r) * C;
        float s = 0.f;
        for (int c = 0; c < C; ++c) s = __fmaf_rn(d[c], k2[(int64_t)j * C + c], s);
        wk.dz1[(int64_t)(r0 + r) * HHID + j] = mul_sep(s, f1[r]);
    }
}

// one thread per parameter of the flat head bucket; the batch rows summed in row order.  grads == nullptr: statistics only.
__global__ void __launch_bounds__(256) head_grads_kernel(int n, int C, const float* __restrict__ prm, float l2x2, HeadWork wk, float* __restrict__ grads,
                                                         double* __restrict__ stats) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        double l = 0.0, h = 0.0;
        for (int r = 0; r < n; ++r) { l += wk.loss[r]; h += wk.hit[r]; }
        stats[0] = l;
        stats[1] = h;
    }
    if (!grads) return;
    const int64_t nk1 = (int64_t)HIN * HHID, nb1 = HHID, nk2 = (int64_t)HHID * C;
    float s = 0.f;
    if (e < nk1) {
        const int i = (int)(e / HHID), j = (int)(e - (int64_t)i * HHID);
        for (int r = 0; r < n; ++r) s = __fmaf_rn(wk.x0[(int64_t)r * HIN + i], wk.dz1[(int64_t)r * HHID + j], s);
        if (l2x2 != 0.f) s = add_sep(s, mul_sep(l2x2, prm[e]));
    } else if (e < nk1 + nb1) {
        const int j = (int)(e - nk1);
        for (int r = 0; r < n; ++r) s = add_sep(s, wk.dz1[(int64_t)r * HHID + j]);
    } else if (e < nk1 + nb1 + nk2) {
        const int64_t q = e - nk1 - nb1;
        const int j = (int)(q / C), c = (int)(q - (int64_t)j * C);
        for (int r = 0; r < n; ++r) s = __fmaf_rn(wk.x1[(int64_t)r * HHID + j], wk.dz2[(int64_t)r * C + c], s);
    } else if (e < nk1 + nb1 + nk2 + C) {
        const int c = (int)(e - nk1 - nb1 - nk2);
        for (int r = 0; r < n; ++r) s = add_sep(s, wk.dz2[(int64_t)r * C + c]);
    } else {
        return;
    }
    grads[e] = s;
}

// dfeats = (dz1 k1^T) * m0 / keep: one thread per input feature i for the workgroup's HROWS rows, dz1 staged in LDS, the 256 hidden units
// summed in index order (thread i streams row i of k1 with 16-byte loads)
__global__ void __launch_bounds__(256) head_dfeats_kernel(int n, const uint8_t* __restrict__ m0, float kscale, const float* __restrict__ prm, HeadWork wk,
                                                          float* __restrict__ dfeats) {
    __shared__ float sdz[HROWS][HHID];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.y * HROWS;
    const int nr = min(HROWS, n - r0);
    for (int e = tid; e < HROWS * HHID; e += 256) {
        const int r = e / HHID, j = e - r * HHID;
        sdz[r][j] = r < nr ? wk.dz1[(int64_t)(r0 + r) * HHID + j] : 0.f;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;          // < HIN: the grid is HIN / 256 wide
    const f32x4* k1 = reinterpret_cast<const f32x4*>(prm + (int64_t)i * HHID);
    float acc[HROWS];
#pragma unroll
    for (int r = 0; r < HROWS; ++r) acc[r] = 0.f;
    for (int j4 = 0; j4 < HHID / 4; ++j4) {
        const f32x4 w = k1[j4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int r = 0; r < HROWS; ++r) acc[r] = __fmaf_rn(sdz[r][j4 * 4 + q], w[q], acc[r]);
        }
    }
    for (int r = 0; r < nr; ++r) {
        const int64_t o = (int64_t)(r0 + r) * HIN + i;
        float v = acc[r];
        if (m0) v = m0[o] ? mul_sep(v, kscale) : 0.f;
        dfeats[o] = v;
    }
}

// GAP -> MaxPooling2D(2,2) -> ReLU backward in one pass: element (b,y,x,c) of dz receives dfeats[b,c] / ((H/2)(W/2)) when it is the first
// maximum of its 2x2 window (maxpool2_bwd_kernel's rule and order) and a > 0, else zero.  VEC channels per thread.
template <int VEC>
__global__ void __launch_bounds__(256) pool_gap_bwd_kernel(const float* __restrict__ a, const float* __restrict__ dfeats, int B, int H, int W, int C,
                                                           float* __restrict__ dz) {
    const int oH = H / 2, oW = W / 2, Cv = C / VEC;
    const float cnt = (float)(oH * oW);
    const int64_t n = (int64_t)B * H * W * Cv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % Cv) * VEC;
        int64_t t = i / Cv;
        const int xq = (int)(t % W); t /= W;
        const int yq = (int)(t % H);
        const int64_t b = t / H;
        const int oy = yq >> 1, ox = xq >> 1;
        float out[VEC];
#pragma unroll
        for (int q = 0; q < VEC; ++q) out[q] = 0.f;
        if (oy < oH && ox < oW) {
            const float* base = a + ((b * H + 2 * oy) * W + 2 * ox) * C + c;
            const float* self = a + ((b * H + yq) * W + xq) * C + c;
            const float* d = dfeats + b * C + c;
            float v00[VEC], v01[VEC], v10[VEC], v11[VEC], av[VEC], dv[VEC];
            if constexpr (VEC == 4) {
                const f32x4 p00 = *reinterpret_cast<const f32x4*>(base), p01 = *reinterpret_cast<const f32x4*>(base + C);
                const f32x4 p10 = *reinterpret_cast<const f32x4*>(base + (int64_t)W * C), p11 = *reinterpret_cast<const f32x4*>(base + (int64_t)W * C + C);
                const f32x4 ps = *reinterpret_cast<const f32x4*>(self), pd = *reinterpret_cast<const f32x4*>(d);
#pragma unroll
                for (int q = 0; q < 4; ++q) { v00[q] = p00[q]; v01[q] = p01[q]; v10[q] = p10[q]; v11[q] = p11[q]; av[q] = ps[q]; dv[q] = pd[q]; }
            } else {
                v00[0] = base[0]; v01[0] = base[C]; v10[0] = base[(int64_t)W * C]; v11[0] = base[(int64_t)W * C + C]; av[0] = self[0]; dv[0] = d[0];
            }
            const int me = (yq & 1) * 2 + (xq & 1);
#pragma unroll
            for (int q = 0; q < VEC; ++q) {
                const float m = fmaxf(fmaxf(v00[q], v01[q]), fmaxf(v10[q], v11[q]));
                const int arg = v00[q] == m ? 0 : (v01[q] == m ? 1 : (v10[q] == m ? 2 : 3));
                const float g = arg == me ? __fdiv_rn(dv[q], cnt) : 0.f;
                out[q] = av[q] > 0.f ? g : 0.f;
            }
        }
        float* o = dz + ((b * H + yq) * W + xq) * C + c;
        if constexpr (VEC == 4) {
            *reinterpret_cast<f32x4*>(o) = f32x4{out[0], out[1], out[2], out[3]};
        } else {
            o[0] = out[0];
        }
    }
}

// the checks and the two launches sr_dense_head_step and sr_dense_head_step_dx share; dfeats != nullptr adds the third
int head_step(sr_ctx* ctx, const std::string& who, const float* feats, int n, int in_dim, int hidden, int num_classes, const int32_t* labels,
              const uint8_t* keep0, const uint8_t* keep1, float keep_scale, const float* params, float l2_reg, float* grads, float* dfeats, double* stats,
              void* work, int64_t work_bytes, void* stream) {
    if (!feats || !labels || !params || !stats || !work) return ctx->fail(SR_ERR_INVALID, who + ": null tensor");
    if (in_dim != HIN || hidden != HHID) return ctx->fail(SR_ERR_INVALID, who + ": the head is Dense 512 -> 256 -> num_classes");
    if (n < 1 || num_classes < 2 || (int64_t)n * num_classes >= ((int64_t)1 << 31) || (int64_t)HHID * num_classes >= ((int64_t)1 << 30))
        return ctx->fail(SR_ERR_INVALID, who + ": need n >= 1 and num_classes >= 2");
    if ((keep0 == nullptr) != (keep1 == nullptr)) return ctx->fail(SR_ERR_INVALID, who + ": both dropout masks or neither");
    if (keep0 && !grads) return ctx->fail(SR_ERR_INVALID, who + ": dropout masks in inference mode");
    if (work_bytes < head_work_bytes(n, num_classes)) return ctx->fail(SR_ERR_CAPACITY, who + ": workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const HeadWork wk = head_work(work, n, num_classes);
    const int train = grads != nullptr;
    hipLaunchKernelGGL(head_rows_kernel, dim3((n + HROWS - 1) / HROWS), dim3(256), 0, st, feats, n, num_classes, labels, keep0, keep1, keep_scale, params, train, wk, stats);
    SR_HIP(ctx, hipGetLastError());
    const int64_t np = (int64_t)HIN * HHID + HHID + (int64_t)HHID * num_classes + num_classes;
    const unsigned gg = train ? (unsigned)((np + 255) / 256) : 1u;
    hipLaunchKernelGGL(head_grads_kernel, dim3(gg), dim3(256), 0, st, n, num_classes, params, 2.f * l2_reg, wk, grads, stats);
    SR_HIP(ctx, hipGetLastError());
    if (dfeats) {
        hipLaunchKernelGGL(head_dfeats_kernel, dim3(HIN / 256, (n + HROWS - 1) / HROWS), dim3(256), 0, st, n, keep0, keep_scale, params, wk, dfeats);
        SR_HIP(ctx, hipGetLastError());
    }
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_affine_warp(sr_ctx* ctx, const float* x, int N, int H, int W, int C, const int32_t* idx, int n, const float* params, float* y, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x || !idx || !params || !y) return ctx->fail(SR_ERR_INVALID, "affine_warp: null tensor");
    if (N < 1 || H < 1 || W < 1 || C < 1 || n < 1 || n > 65535) return ctx->fail(SR_ERR_INVALID, "affine_warp: empty set or batch (1 <= n <= 65535)");
    if ((int64_t)H * W * C >= ((int64_t)1 << 31) || H >= (1 << 24) || W >= (1 << 24)) return ctx->fail(SR_ERR_INVALID, "affine_warp: image too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t per = (int64_t)H * W * C;
    const bool v4 = per % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    const int64_t nthr = v4 ? per / 4 : per;
    const unsigned gx = (unsigned)std::min<int64_t>((nthr + 255) / 256, 1024);
    if (v4)
        hipLaunchKernelGGL(affine_warp_kernel<4>, dim3(gx, n), dim3(256), 0, st, x, N, H, W, C, idx, params, y);
    else
        hipLaunchKernelGGL(affine_warp_kernel<1>, dim3(gx, n), dim3(256), 0, st, x, N, H, W, C, idx, params, y);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int64_t sr_dense_head_workspace_bytes(int n, int num_classes) {
    if (n < 1 || num_classes < 2) return -1;
    return head_work_bytes(n, num_classes);
}

int sr_dense_head_step(sr_ctx* ctx, const float* feats, int n, int in_dim, int hidden, int num_classes, const int32_t* labels, const uint8_t* keep0,
                       const uint8_t* keep1, float keep_scale, const float* params, float l2_reg, float* grads, double* stats, void* work,
                       int64_t work_bytes, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    return head_step(ctx, "dense_head_step", feats, n, in_dim, hidden, num_classes, labels, keep0, keep1, keep_scale, params, l2_reg, grads, nullptr, stats, work,
                     work_bytes, stream);
}

int sr_dense_head_step_dx(sr_ctx* ctx, const float* feats, int n, int in_dim, int hidden, int num_classes, const int32_t* labels, const uint8_t* keep0,
                          const uint8_t* keep1, float keep_scale, const float* params, float l2_reg, float* grads, float* dfeats, double* stats, void* work,
                          int64_t work_bytes, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!grads || !dfeats) return ctx->fail(SR_ERR_INVALID, "dense_head_step_dx: null tensor");
    if (n > 65535 * HROWS) return ctx->fail(SR_ERR_INVALID, "dense_head_step_dx: n <= 524280");
    if (reinterpret_cast<uintptr_t>(params) & 15) return ctx->fail(SR_ERR_INVALID, "dense_head_step_dx: params must be 16-byte aligned");
    return head_step(ctx, "dense_head_step_dx", feats, n, in_dim, hidden, num_classes, labels, keep0, keep1, keep_scale, params, l2_reg, grads, dfeats, stats, work,
                     work_bytes, stream);
}

int sr_pool_gap_bwd(sr_ctx* ctx, const float* a, const float* dfeats, int B, int H, int W, int C, float* dz, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!a || !dfeats || !dz) return ctx->fail(SR_ERR_INVALID, "pool_gap_bwd: null tensor");
    if (B < 1 || H < 2 || W < 2 || C < 1) return ctx->fail(SR_ERR_INVALID, "pool_gap_bwd: need B >= 1, H >= 2, W >= 2, C >= 1");
    if (H >= (1 << 15) || W >= (1 << 15)) return ctx->fail(SR_ERR_INVALID, "pool_gap_bwd: map too large");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool v4 = C % 4 == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(dfeats) | reinterpret_cast<uintptr_t>(dz)) & 15) == 0;
    const int64_t nthr = (int64_t)B * H * W * (v4 ? C / 4 : C);
    const int64_t blocks = (nthr + 255) / 256;                 // one thread per VEC channels of a pixel, no cap: B H W C / VEC threads
    if (blocks > 0x7fffffff) return ctx->fail(SR_ERR_INVALID, "pool_gap_bwd: tensor too large");
    const unsigned gx = (unsigned)blocks;
    if (v4)
        hipLaunchKernelGGL(pool_gap_bwd_kernel<4>, dim3(gx), dim3(256), 0, st, a, dfeats, B, H, W, C, dz);
    else
        hipLaunchKernelGGL(pool_gap_bwd_kernel<1>, dim3(gx), dim3(256), 0, st, a, dfeats, B, H, W, C, dz);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
