// study.hip -- the device side of the SR comparison (reference: VGG16_model.py:168-270 for a stack of frames, and the numeric halves of
// SRModels/deep_lerning_visualizations.py:230-314, 454-495): cut the classifier's patches from a whole stack of frames in one launch, vote per
// frame on the device, and count a study's predictions into confusion matrices, so that F frames (or A methods x N frames) cost one read-back.
//
//   extract_patches_batch   a pure gather, HBM-bound.  A patch row is patch*C contiguous values in the destination and, up to the reflected
//                           tail, in the source.  Where patch*C is a multiple of 4 (and both base pointers are 16-byte aligned) a thread
//                           owns four consecutive destination values: one 16-byte (fp32) or 8-byte (bf16) store, and one 16-byte (fp32) or
//                           4-byte (uint8) load where the four sources are contiguous and aligned, four scalar loads in the reflected tail
//                           or at an odd source offset.  Otherwise one value per thread.  The value is sr_extract_patches' expression
//                           (v * mul + add, product and sum rounded separately), so a frame's slice is that call's output bit for bit.
//                           Indices are 64-bit.
//   patch_vote              one workgroup per frame.  Thread t owns column t % Kp (Kp = K rounded up to a power of two <= 64) of the rows
//                           t / Kp, t / Kp + 256 / Kp, ...: loads are coalesced, a row's argmax is a butterfly over its Kp lanes (larger value,
//                           then lower index: np.argmax's first maximum), votes are integer atomics in LDS, and every column sum is one fp64
//                           accumulator per thread followed by a tree over the row groups in LDS -- a fixed order, no float atomics, the
//                           same bits on every run.  Thread 0 then applies the reference's tie rule.
//   classification_counts   one workgroup per method: integer atomics into the (zeroed) K x K matrix, fp64 per-thread sums and an LDS tree.
#include "common.h"
#include "fp_sep.h"

#include <string>

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int reflect_br(int y, int n) { return y < n ? y : 2 * (n - 1) - y; }   // np.pad 'reflect', bottom / right

struct PatchGeom { int F, H, W, C, patch, stride, ny, nx; };

__device__ __forceinline__ float affine(float v, float mul, float add) { return add_sep(mul_sep(v, mul), add); }   // two roundings (fp_sep.h)

// one value per thread: any patch*C, any alignment
template <typename TIn>
__global__ void __launch_bounds__(256) extract_batch_scalar_kernel(const TIn* __restrict__ imgs, PatchGeom g, float mul, float add, int out_dt,
                                                                   void* __restrict__ out) {
    const int64_t n = (int64_t)g.F * g.ny * g.nx * g.patch * g.patch * g.C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i;
        const int c = (int)(t % g.C); t /= g.C;
        const int px = (int)(t % g.patch); t /= g.patch;
        const int py = (int)(t % g.patch); t /= g.patch;
        const int jx = (int)(t % g.nx); t /= g.nx;
        const int jy = (int)(t % g.ny);
        const int64_t f = t / g.ny;
        const int y = reflect_br(jy * g.stride + py, g.H), x = reflect_br(jx * g.stride + px, g.W);
        const float v = affine((float)imgs[((f * g.H + y) * g.W + x) * g.C + c], mul, add);
        if (out_dt == SR_DTYPE_F32) static_cast<float*>(out)[i] = v; else static_cast<bf16_t*>(out)[i] = (bf16_t)v;
    }
}

__device__ __forceinline__ void load4(const float* p, float v[4]) { const float4 q = *reinterpret_cast<const float4*>(p); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
__device__ __forceinline__ void load4(const uint8_t* p, float v[4]) {
    const uchar4 q = *reinterpret_cast<const uchar4*>(p);
    v[0] = (float)q.x; v[1] = (float)q.y; v[2] = (float)q.z; v[3] = (float)q.w;
}

// four consecutive destination values per thread; needs (patch * C) % 4 == 0 (a quad never leaves its patch row), imgs and out 16-byte aligned
template <typename TIn>
__global__ void __launch_bounds__(256) extract_batch_quad_kernel(const TIn* __restrict__ imgs, PatchGeom g, float mul, float add, int out_dt,
                                                                 void* __restrict__ out) {
    const int row = g.patch * g.C, qrow = row >> 2;
    const int64_t nq = (int64_t)g.F * g.ny * g.nx * g.patch * qrow;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = q;
        const int e = (int)(t % qrow) << 2; t /= qrow;                      // first of the four values within the patch row
        const int py = (int)(t % g.patch); t /= g.patch;
        const int jx = (int)(t % g.nx); t /= g.nx;
        const int jy = (int)(t % g.ny);
        const int64_t f = t / g.ny;
        const int y = reflect_br(jy * g.stride + py, g.H);
        const int64_t line = (f * g.H + y) * g.W;                           // pixel index of the source row's first pixel
        const int x0 = jx * g.stride;
        const int px_first = e / g.C, px_last = (e + 3) / g.C;
        float v[4];
        const int64_t s0 = (line + x0) * g.C + e;                           // valid while x0 + px_last < W: no reflection inside the quad
        if (x0 + px_last < g.W && (s0 & 3) == 0) {
            load4(imgs + s0, v);
        } else {
            int px = px_first, c = e - px_first * g.C;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (float)imgs[(line + reflect_br(x0 + px, g.W)) * g.C + c];
                if (++c == g.C) { c = 0; ++px; }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = affine(v[k], mul, add);
        if (out_dt == SR_DTYPE_F32) {
            reinterpret_cast<float4*>(out)[q] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            union { bf16_t h[4]; uint2 u; } pk;
#pragma unroll
            for (int k = 0; k < 4; ++k) pk.h[k] = (bf16_t)v[k];
            reinterpret_cast<uint2*>(out)[q] = pk.u;
        }
    }
}

inline unsigned grid_for(int64_t n) {
    const int64_t g = (n + 255) / 256, cap = 256 * 8 * 4;
    return (unsigned)(g < 1 ? 1 : (g > cap ? cap : g));
}

template <typename TIn>
void extract_batch_launch(const void* imgs, const PatchGeom& g, float mul, float add, int out_dt, void* out, hipStream_t st) {
    const int64_t n = (int64_t)g.F * g.ny * g.nx * g.patch * g.patch * g.C;
    const bool quad = (g.patch * g.C) % 4 == 0 && (((uintptr_t)imgs | (uintptr_t)out) & 15) == 0;
    if (quad)
        hipLaunchKernelGGL(extract_batch_quad_kernel<TIn>, dim3(grid_for(n / 4)), dim3(256), 0, st, static_cast<const TIn*>(imgs), g, mul, add, out_dt, out);
    else
        hipLaunchKernelGGL(extract_batch_scalar_kernel<TIn>, dim3(grid_for(n)), dim3(256), 0, st, static_cast<const TIn*>(imgs), g, mul, add, out_dt, out);
}

// ------------------------------------------------------------------------------------------------ the vote (VGG16_model.py:252-268)
// grid F, block 256.  Kp = K rounded up to a power of two; lanes [g Kp, (g + 1) Kp) of the block form row group g: aligned inside one wave.
__global__ void __launch_bounds__(256) patch_vote_kernel(const float* __restrict__ probs, int P, int K, int Kp, int32_t* __restrict__ cls,
                                                         float* __restrict__ conf, int32_t* __restrict__ votes_out) {
    __shared__ double sums[256];
    __shared__ int votes[64];
    const int tid = threadIdx.x, c = tid & (Kp - 1), grp = tid / Kp, G = 256 / Kp;
    const float* fp = probs + (int64_t)blockIdx.x * P * K;
    if (tid < 64) votes[tid] = 0;
    __syncthreads();
    double acc = 0.0;
    for (int r0 = 0; r0 < P; r0 += G) {                                     // uniform trip count: every lane takes part in the shuffles
        const int r = r0 + grp;
        const bool live = r < P && c < K;
        float v = live ? fp[(int64_t)r * K + c] : -INFINITY;
        int at = live ? c : K;
        if (live) acc += (double)v;
        for (int m = 1; m < Kp; m <<= 1) {
            const float ov = __shfl_xor(v, m, 64);
            const int oa = __shfl_xor(at, m, 64);
            if (ov > v || (ov == v && oa < at)) { v = ov; at = oa; }
        }
        if (c == 0 && r < P && at < K) atomicAdd(&votes[at], 1);
    }
    sums[tid] = acc;                                                        // sums[grp * Kp + c]
    __syncthreads();
    for (int s = G >> 1; s > 0; s >>= 1) {                                  // tree over the row groups, the same order on every run
        if (grp < s) sums[tid] += sums[tid + s * Kp];
        __syncthreads();
    }
    if (votes_out && tid < K) votes_out[(int64_t)blockIdx.x * K + tid] = votes[tid];
    if (tid == 0) {
        int best = 0;
        for (int k = 0; k < K; ++k) best = votes[k] > best ? votes[k] : best;
        int win = -1;
        double win_mean = 0.0;
        for (int k = 0; k < K; ++k) {                                       // among the tied classes the highest mean, first on equal means
            if (votes[k] != best) continue;
            const double mean = sums[k] / (double)P;
            if (win < 0 || mean > win_mean) { win = k; win_mean = mean; }
        }
        cls[blockIdx.x] = win;
        conf[blockIdx.x] = (float)win_mean;                                 // the fp64 mean, rounded once
    }
}

// ------------------------------------------------------------------------------------------------ a study's counts
// grid A, block 256.  confusion zeroed by the caller.  Labels outside [0, K) are counted nowhere (the wrapper validates host labels).
__global__ void __launch_bounds__(256) classification_counts_kernel(const int32_t* __restrict__ y_true, const int32_t* __restrict__ preds,
                                                                    const float* __restrict__ conf, int N, int K, u64* __restrict__ confusion,
                                                                    double* __restrict__ conf_sums) {
    __shared__ double s_all[256], s_ok[256];
    const int a = blockIdx.x, tid = threadIdx.x;
    const int32_t* p = preds + (int64_t)a * N;
    const float* cf = conf ? conf + (int64_t)a * N : nullptr;
    u64* cm = confusion + (int64_t)a * K * K;
    double all = 0.0, ok = 0.0;
    for (int i = tid; i < N; i += 256) {
        const int t = y_true[i], q = p[i];
        if (t >= 0 && t < K && q >= 0 && q < K) atomicAdd(&cm[(int64_t)t * K + q], (u64)1);
        if (cf) {
            const double v = (double)cf[i];
            all += v;
            if (t == q) ok += v;
        }
    }
    s_all[tid] = all; s_ok[tid] = ok;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) { s_all[tid] += s_all[tid + s]; s_ok[tid] += s_ok[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) { conf_sums[2 * a] = s_all[0]; conf_sums[2 * a + 1] = s_ok[0]; }
}

}  // namespace

extern "C" {

int sr_extract_patches_batch(sr_ctx* ctx, const void* imgs, int in_dtype, int F, int H, int W, int C, int patch, int stride, float mul, float add,
                             int out_dtype, void* out, int64_t out_capacity, int* patches_per_image, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (F <= 0 || H <= 0 || W <= 0 || C <= 0 || patch <= 0 || stride <= 0) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: bad shape/patch/stride");
    if (H >= (1 << 20) || W >= (1 << 20) || patch >= (1 << 20) || C > 4096) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: image, patch or channel count too large");
    const int ph = pad_amount(H, patch, stride), pw = pad_amount(W, patch, stride);
    if (ph >= H || pw >= W) return ctx->fail(SR_ERR_INVALID, "reflect padding needs pad < image size");   // np.pad would wrap repeatedly
    const int Hp = H + ph, Wp = W + pw;
    const int ny = Hp >= patch ? (Hp - patch) / stride + 1 : 0, nx = Wp >= patch ? (Wp - patch) / stride + 1 : 0;
    if ((int64_t)ny * nx >= ((int64_t)1 << 31)) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: a frame holds fewer than 2^31 patches");
    if (patches_per_image) *patches_per_image = ny * nx;
    if (!out) return SR_OK;
    if (!imgs) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: null image stack");
    if (in_dtype != SR_DTYPE_F32 && in_dtype != SR_DTYPE_U8) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: in dtype must be f32 or u8");
    if (out_dtype != SR_DTYPE_F32 && out_dtype != SR_DTYPE_BF16) return ctx->fail(SR_ERR_INVALID, "extract_patches_batch: out dtype must be f32 or bf16");
    if (out_capacity < (int64_t)F * ny * nx * patch * patch * C) return ctx->fail(SR_ERR_CAPACITY, "patch buffer too small");
    if (ny * nx == 0) return SR_OK;
    const PatchGeom g{F, H, W, C, patch, stride, ny, nx};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (in_dtype == SR_DTYPE_U8) extract_batch_launch<uint8_t>(imgs, g, mul, add, out_dtype, out, st);
    else extract_batch_launch<float>(imgs, g, mul, add, out_dtype, out, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_patch_vote(sr_ctx* ctx, const float* probs, int F, int P, int K, int32_t* cls_F, float* conf_F, int32_t* votes_FxK, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (K < 1 || K > 64) return ctx->fail(SR_ERR_INVALID, "patch_vote: 1 <= K <= 64");
    if (F < 1 || P < 1 || P > (1 << 30)) return ctx->fail(SR_ERR_INVALID, "patch_vote: F >= 1 and 1 <= P <= 2^30");
    if (!probs || !cls_F || !conf_F) return ctx->fail(SR_ERR_INVALID, "patch_vote: null tensor");
    int Kp = 1;
    while (Kp < K) Kp <<= 1;
    hipLaunchKernelGGL(patch_vote_kernel, dim3(F), dim3(256), 0, static_cast<hipStream_t>(stream), probs, P, K, Kp, cls_F, conf_F, votes_FxK);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_classification_counts(sr_ctx* ctx, const int32_t* y_true_N, const int32_t* preds_AxN, const float* conf_AxN, int A, int N, int K,
                             int64_t* confusion_AxKxK, double* conf_sums_Ax2, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (A < 1 || N < 1 || K < 1 || K > 4096) return ctx->fail(SR_ERR_INVALID, "classification_counts: A, N >= 1 and 1 <= K <= 4096");
    if (!y_true_N || !preds_AxN || !confusion_AxKxK || !conf_sums_Ax2) return ctx->fail(SR_ERR_INVALID, "classification_counts: null tensor");
    hipStream_t st = static_cast<hipStream_t>(stream);
    SR_HIP(ctx, hipMemsetAsync(confusion_AxKxK, 0, sizeof(int64_t) * (size_t)A * K * K, st));
    hipLaunchKernelGGL(classification_counts_kernel, dim3(A), dim3(256), 0, st, y_true_N, preds_AxN, conf_AxN, N, K,
                       reinterpret_cast<u64*>(confusion_AxKxK), conf_sums_Ax2);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
