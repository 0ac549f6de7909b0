// patch_dataset.hip -- training batches cut on the device from resident image stacks (reference SRModels/loading_methods.py:40-191).
//
// load_dataset_as_patches reflect-pads every image at the bottom / right (add_padding) and appends its sliding windows to two dense fp32
// arrays; neighbouring windows overlap, so the arrays repeat every pixel several times.  Here the distinct pixels stay on the device once, as
// uint8 (or as the fp32 result of the srcnn mode's resize), with a table of window origins, and sr_gather_patch_pairs cuts one batch of LR and
// HR patches from them in one launch: the reflect index, the optional BGR -> RGB swap, the uint8 -> [0,1] division and the trainer's affine
// scaling are applied per element on the way.  The arithmetic is the loader's, operation by operation:
//   * float(u) / 255.0f is a correctly rounded division (__fdiv_rn), as NumPy's float32 / 255.0 is.  u * (1 / 255.0f) is NOT the same
//     function: it differs from the quotient in 126 of the 256 codes.
//   * v * mul + add rounds the product and the sum separately (NumPy evaluates `a * 2.0 - 1.0` as two ufuncs), and is skipped when it is
//     the identity, so the default batch is a copy of the stored values.
// Memory-bound and small (a batch is a few hundred KB): one thread per pixel (three channels), no LDS.  Every table entry is clamped into
// range before it is used as an index: whatever the window table and the order hold, no thread reads outside the stacks.
// sr_gather_warp_patches does the same for the classifier's fit (load_defects_dataset_as_patches: one stack, no padding) and applies the
// augmentation warp of sr_affine_warp on the way, with that kernel's own arithmetic (warp_sample.h): no fp32 patch ever lies in memory.
#include "common.h"
#include "fp_sep.h"
#include "warp_sample.h"

#include <algorithm>
#include <cmath>

namespace {

struct Side {
    const void* src;
    float* out;
    int u8, N, H, W, pad_h, pad_w, swap, ph, pw, oscale;      // ph / pw: this side's patch size; oscale: window origin = table origin * oscale
    float mul, add;
    int affine;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// np.pad(mode="reflect") at the bottom / right: index i >= n of the padded axis is 2 (n - 1) - i (valid for pads up to n - 1; clamped besides)
__device__ __forceinline__ int reflect_br(int i, int n) { return clampi(i < n ? i : 2 * (n - 1) - i, 0, n - 1); }

__device__ __forceinline__ void gather_pixel(const Side& s, const int32_t* __restrict__ windows, int n_windows, const int32_t* __restrict__ order,
                                             int64_t offset, int64_t pix) {
    const int per = s.ph * s.pw;
    const int b = (int)(pix / per), r = (int)(pix - (int64_t)b * per);
    const int py = r / s.pw, px = r - py * s.pw;
    const int k = clampi(order[offset + b], 0, n_windows - 1);
    const int img = clampi(windows[3 * (int64_t)k], 0, s.N - 1);
    // y0 * oscale cannot wrap once y0 is clamped: (H + pad_h - ph) is the largest origin of this side, its LR-side counterpart no larger
    const int y0 = clampi(clampi(windows[3 * (int64_t)k + 1], 0, s.H + s.pad_h) * s.oscale, 0, s.H + s.pad_h - s.ph);
    const int x0 = clampi(clampi(windows[3 * (int64_t)k + 2], 0, s.W + s.pad_w) * s.oscale, 0, s.W + s.pad_w - s.pw);
    const int y = reflect_br(y0 + py, s.H), x = reflect_br(x0 + px, s.W);
    const int64_t at = (((int64_t)img * s.H + y) * s.W + x) * 3;
    float v[3];
    if (s.u8) {
        const uint8_t* p = static_cast<const uint8_t*>(s.src) + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)p[c], 255.0f);
    } else {
        const float* p = static_cast<const float*>(s.src) + at;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = p[c];
    }
    if (s.swap) { const float t = v[0]; v[0] = v[2]; v[2] = t; }
    if (s.affine) {                                                  // two roundings, as NumPy's two ufuncs: no fma (fp_sep.h)
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = add_sep(mul_sep(v[c], s.mul), s.add);
    }
    float* o = s.out + pix * 3;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// pixels [0, n_lr) belong to the LR batch, [n_lr, n_lr + n_hr) to the HR batch
__global__ void __launch_bounds__(256) gather_patch_pairs_kernel(Side lr, Side hr, const int32_t* __restrict__ windows, int n_windows,
                                                                 const int32_t* __restrict__ order, int64_t offset, int64_t n_lr, int64_t n_hr) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_lr + n_hr; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < n_lr) gather_pixel(lr, windows, n_windows, order, offset, i);
        else gather_pixel(hr, windows, n_windows, order, offset, i - n_lr);
    }
}

// sr_gather_warp_patches: the classifier fit's augmented batch straight from the frame stack.  Workgroups (x, b) share batch element b: its
// window and its sixteen parameters are read once per thread, then each thread takes whole pixels -- the two coordinates are computed once
// and serve the three channels.  The taps are clamped to the PATCH, so the window's neighbours in the frame never enter the result.
struct WarpSrc {
    const void* src;
    int u8, N, H, W, swap, ph, pw;
};

__device__ __forceinline__ void load_tap(const WarpSrc& s, int64_t pix, float (&v)[3]) {
    if (s.u8) {
        const uint8_t* p = static_cast<const uint8_t*>(s.src) + pix * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = __fdiv_rn((float)p[c], 255.0f);
    } else {
        const float* p = static_cast<const float*>(s.src) + pix * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = p[c];
    }
}

__global__ void __launch_bounds__(256) gather_warp_patches_kernel(WarpSrc s, const int32_t* __restrict__ windows, int n_windows,
                                                                  const int32_t* __restrict__ order, int64_t offset, const float* __restrict__ prm,
                                                                  float* __restrict__ y) {
    const int b = blockIdx.y;
    const int k = clampi(order[offset + b], 0, n_windows - 1);
    const int img = clampi(windows[3 * (int64_t)k], 0, s.N - 1);
    const int y0 = clampi(windows[3 * (int64_t)k + 1], 0, s.H - s.ph), x0 = clampi(windows[3 * (int64_t)k + 2], 0, s.W - s.pw);
    const float* p = prm + (int64_t)b * WARP_PRM;
    float hi[6], lo[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) { hi[q] = p[q]; lo[q] = p[6 + q]; }
    const bool flip = p[12] != 0.f;
    const int64_t origin = ((int64_t)img * s.H + y0) * s.W + x0;          // the window's first pixel in the stack
    const int per = s.ph * s.pw;
    float* yo = y + (int64_t)b * per * 3;
    for (int pix = blockIdx.x * 256 + threadIdx.x; pix < per; pix += gridDim.x * 256) {
        const int oy = pix / s.pw;
        int ox = pix - oy * s.pw;
        if (flip) ox = s.pw - 1 - ox;
        const WarpTaps t = warp_taps(hi, lo, oy, ox, s.ph, s.pw);          // indices within the patch: 0 .. ph - 1, 0 .. pw - 1
        float v00[3], v01[3], v10[3], v11[3];
        load_tap(s, origin + (int64_t)t.ya * s.W + t.xa, v00);
        load_tap(s, origin + (int64_t)t.ya * s.W + t.xb, v01);
        load_tap(s, origin + (int64_t)t.yb * s.W + t.xa, v10);
        load_tap(s, origin + (int64_t)t.yb * s.W + t.xb, v11);
        float* o = yo + (int64_t)pix * 3;
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = bilerp(v00[c], v01[c], v10[c], v11[c], t.ty, t.tx);
        o[0] = s.swap ? r[2] : r[0];
        o[1] = r[1];
        o[2] = s.swap ? r[0] : r[2];
    }
}

// -> nullptr when the side is usable, else what is wrong with it
const char* side_problem(const sr_patch_side& s, int ph, int pw) {
    if (!s.src || !s.out) return "gather_patch_pairs: null stack or batch";
    if (s.dtype != SR_DTYPE_U8 && s.dtype != SR_DTYPE_F32) return "gather_patch_pairs: a stack is uint8 or fp32";
    if (s.N < 1 || s.H < 1 || s.W < 1) return "gather_patch_pairs: empty stack";
    if (s.H >= (1 << 20) || s.W >= (1 << 20)) return "gather_patch_pairs: image too large";
    if (s.pad_h < 0 || s.pad_w < 0 || s.pad_h > s.H - 1 || s.pad_w > s.W - 1) return "gather_patch_pairs: reflect padding needs 0 <= pad <= size - 1";
    if (ph > s.H + s.pad_h || pw > s.W + s.pad_w) return "gather_patch_pairs: the patch is larger than the padded image";
    if (!std::isfinite(s.mul) || !std::isfinite(s.add)) return "gather_patch_pairs: mul and add must be finite";
    return nullptr;
}

Side make_side(const sr_patch_side& s, int ph, int pw, int oscale) {
    return Side{s.src, s.out, s.dtype == SR_DTYPE_U8, s.N, s.H, s.W, s.pad_h, s.pad_w, s.swap_rb != 0, ph, pw, oscale, s.mul, s.add,
                !(s.mul == 1.f && s.add == 0.f)};
}

}  // namespace

extern "C" {

int sr_gather_patch_pairs(sr_ctx* ctx, const sr_patch_side* lr, const sr_patch_side* hr, const int32_t* windows, int n_windows,
                          const int32_t* order, int64_t n_order, int64_t offset, int B, int patch_h, int patch_w, int scale, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!lr || !windows || !order) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: null pointer");
    if (B < 1 || patch_h < 1 || patch_w < 1 || scale < 1 || scale > 64 || n_windows < 1)
        return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: B, patch, scale (<= 64) and n_windows must be >= 1");
    if (offset < 0 || n_order < 1 || offset > n_order - B) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: the batch reaches outside the order array");
    if ((int64_t)patch_h * scale >= (1 << 24) || (int64_t)patch_w * scale >= (1 << 24)) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: patch too large");
    const int PH = patch_h * scale, PW = patch_w * scale;
    if (const char* why = side_problem(*lr, patch_h, patch_w)) return ctx->fail(SR_ERR_INVALID, why);
    if (hr) {
        if (const char* why = side_problem(*hr, PH, PW)) return ctx->fail(SR_ERR_INVALID, why);
        if (hr->N != lr->N) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: the two stacks hold different numbers of images");
        if (hr->out == lr->out) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: the two batches must not alias");
    }
    const int64_t n_lr = (int64_t)B * patch_h * patch_w, n_hr = hr ? (int64_t)B * PH * PW : 0;
    if ((n_lr + n_hr) * 3 >= ((int64_t)1 << 31)) return ctx->fail(SR_ERR_INVALID, "gather_patch_pairs: a batch holds fewer than 2^31 values");
    const Side a = make_side(*lr, patch_h, patch_w, 1);
    const Side b = hr ? make_side(*hr, PH, PW, scale) : a;       // n_hr == 0: never dereferenced
    const int64_t g = (n_lr + n_hr + 255) / 256;
    hipLaunchKernelGGL(gather_patch_pairs_kernel, dim3((unsigned)(g > 8192 ? 8192 : g)), dim3(256), 0, static_cast<hipStream_t>(stream), a, b, windows,
                       n_windows, order, offset, n_lr, n_hr);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_gather_warp_patches(sr_ctx* ctx, const void* src, int dtype, int N, int H, int W, const int32_t* windows, int n_windows, const int32_t* order,
                           int64_t n_order, int64_t offset, int B, int patch_h, int patch_w, int swap_rb, const float* params, float* y, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!src || !windows || !order || !params || !y) return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: null pointer");
    if (dtype != SR_DTYPE_U8 && dtype != SR_DTYPE_F32) return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: the stack is uint8 or fp32");
    if (N < 1 || H < 1 || W < 1 || B < 1 || patch_h < 1 || patch_w < 1 || n_windows < 1)
        return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: N, H, W, B, patch and n_windows must be >= 1");
    if (patch_h > H || patch_w > W) return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: the patch is larger than the frame");
    if (offset < 0 || n_order < 1 || offset > n_order - B) return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: the batch reaches outside the order array");
    if (patch_h >= (1 << 24) || patch_w >= (1 << 24)) return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: patch too large");      // exact as fp32
    const int64_t vals = (int64_t)patch_h * patch_w * 3;
    if (B > 65535 || vals >= ((int64_t)1 << 31) || B * vals >= ((int64_t)1 << 31))
        return ctx->fail(SR_ERR_INVALID, "gather_warp_patches: a batch holds at most 65535 patches and fewer than 2^31 values");
    const WarpSrc s{src, dtype == SR_DTYPE_U8, N, H, W, swap_rb != 0, patch_h, patch_w};
    const int per = patch_h * patch_w;
    const unsigned gx = (unsigned)std::min((per + 255) / 256, 1024);
    hipLaunchKernelGGL(gather_warp_patches_kernel, dim3(gx, (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), s, windows, n_windows, order,
                       offset, params, y);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
