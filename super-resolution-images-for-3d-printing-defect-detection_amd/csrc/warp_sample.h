// warp_sample.h -- the sampling arithmetic of the augmentation warp, defined once for sr_affine_warp (head_train.hip) and
// sr_gather_warp_patches (patch_dataset.hip): the two kernels must give the same bits for the same patch, so neither restates it.
//   coord     one sample coordinate as an fp32 double-float sum of the host's fp64 parameters split into hi + lo halves -> floor and fraction.
//   warp_taps both coordinates of an output pixel -> the four clamped tap indices and the two fractions.
//   bilerp    the bilinear combination of the four taps (scipy order=1).
#pragma once
#include <hip/hip_runtime.h>

constexpr int WARP_PRM = 16;          // per image: hi(a00 a01 a10 a11 o0 o1), lo(same), flip, 3 unused

// The error-free transformations below hold only if every operation is rounded on its own.  __fmul_rn / __fadd_rn are plain operators to the
// compiler, which had fused the products into the sums that follow them (s - h * u as one fma): the sum's error term then no longer belongs to
// the rounded product, and the coordinate was off by half an ulp of its magnitude -- 3e-5 of a pixel at 592 pixels, within the tests' bound
// at 128.  Contraction is therefore switched off for the operators written here; the two fmas that are meant are spelled out.
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
#pragma clang fp contract(off)
    s = a + b;
    const float bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}

// ah * u + bh * v + oh (+ the lo halves) for integer u, v -> floor and fraction in [0, 1)
__device__ __forceinline__ void coord(const float* h, const float* l, int k, float u, float v, int lim, int& i0, float& t) {
#pragma clang fp contract(off)
    const float p1 = h[2 * k] * u, e1 = __fmaf_rn(h[2 * k], u, -p1);
    const float p2 = h[2 * k + 1] * v, e2 = __fmaf_rn(h[2 * k + 1], v, -p2);
    float s, t1, s2, t2;
    two_sum(p1, p2, s, t1);
    two_sum(s, h[4 + k], s2, t2);
    const float lo = ((t1 + t2) + (e1 + e2)) + ((l[2 * k] * u + l[2 * k + 1] * v) + l[4 + k]);
    float f = floorf(s2);
    float fr = (s2 - f) + lo;
    if (fr < 0.f) { f = f - 1.f; fr = fr + 1.f; }
    if (fr >= 1.f) { f = f + 1.f; fr = fr - 1.f; }
    f = fminf(fmaxf(f, -1.f), (float)lim);          // beyond the border both taps clamp to the edge; keeps the int conversion in range
    i0 = (int)f;
    t = fr;
}

struct WarpTaps {
    int ya, yb, xa, xb;       // tap rows / columns, clamped to [0, H - 1] / [0, W - 1]
    float ty, tx;             // fractions towards yb / xb
};

// output pixel (oy, ox) of an H x W image (ox already mirrored where the image is flipped) -> its four taps
__device__ __forceinline__ WarpTaps warp_taps(const float* hi, const float* lo, int oy, int ox, int H, int W) {
    WarpTaps t;
    int y0, x0;
    coord(hi, lo, 0, (float)oy, (float)ox, H, y0, t.ty);
    coord(hi, lo, 1, (float)oy, (float)ox, W, x0, t.tx);
    t.ya = min(max(y0, 0), H - 1);
    t.yb = min(max(y0 + 1, 0), H - 1);
    t.xa = min(max(x0, 0), W - 1);
    t.xb = min(max(x0 + 1, 0), W - 1);
    return t;
}

// The roundings are spelled out and contraction is off: left to the compiler, which products fuse into an fma depends on how the caller's
// loop was vectorised, and two callers would round differently.  A row is wx0 * a rounded, then one fma with tx * b; the two rows are
// combined by two rounded products and a rounded sum -- the form sr_affine_warp has always computed.  tx == 0 and ty == 0 return v00's bits.
__device__ __forceinline__ float bilerp(float v00, float v01, float v10, float v11, float ty, float tx) {
#pragma clang fp contract(off)          // governs the operators written here, not the bodies of __fmul_rn / __fadd_rn: hence plain * and +
    const float wy0 = 1.f - ty, wx0 = 1.f - tx;
    const float top = __fmaf_rn(tx, v01, wx0 * v00);
    const float bot = __fmaf_rn(tx, v11, wx0 * v10);
    const float a = wy0 * top, b = ty * bot;
    return a + b;
}
