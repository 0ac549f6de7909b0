// classic.hip -- the four non-resize baselines of the reference's classical study (classic_super_resolution_algorithms/
// classic_algorithms.py:23-108) on 2-D uint8 grayscale images, batched over B images of one size:
//   iterative back-projection, the db2 noise-sigma estimate + fast non-local means, edge-guided interpolation and
//   frequency-domain zero-padding (as a separable fp64 DFT operator).
// The resize steps reuse imgops.hip's tap tables (resize_taps_kernel) with sr_resize's rules, so every resize here is the one
// sr_resize computes.
#include "cgemm_f64.h"
#include "common.h"
#include "fp_sep.h"

#include <cmath>

__global__ void resize_taps_kernel(int n_src, int n_dst, int interp, int area_up, int T, int* idx, float* w, int* iw);   // imgops.hip

namespace {

inline unsigned cls_grid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

bool dims_ok(int64_t B, int64_t a, int64_t b) { return B > 0 && a > 0 && b > 0 && B * a * b < ((int64_t)1 << 40); }

// numpy's 'reflect' padding (edge not repeated), for any distance from the image: period 2 (n - 1)
__device__ inline int reflect_idx(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// pywt's 'symmetric' extension (edge repeated): period 2 n
__device__ inline int symmetric_idx(int i, int n) {
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// OpenCV BORDER_REFLECT_101 for the one-pixel reach of a 3x3 Sobel
__device__ inline int reflect101_idx(int i, int n) {
    if (n == 1) return 0;
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

// ------------------------------------------------------------------------------------------------
// Iterative back-projection (classic_algorithms.py:23-43).  hr = float32(hr_image); per iteration
//   diff = float32(lr) - resize(hr, (w, h), INTER_LINEAR);   hr += resize(diff, (W, H), INTER_LINEAR)
// then clip(hr, 0, 255).astype(uint8) (truncating).  The resizes are sr_resize's float32 path: horizontal taps first, each product
// and sum rounded as OpenCV's two passes round them; an exact 2x shrink is the 2 x 2 area mean, as OpenCV rewrites it.
// ------------------------------------------------------------------------------------------------
__global__ void ibp_init_kernel(const uint8_t* hr, int64_t n, float* est, uint8_t* y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        est[i] = (float)hr[i];
        if (y) y[i] = hr[i];                                // iterations == 0: the clipped first argument
    }
}

// LR pass: the down-resize of the estimate, gathered through its tap tables, subtracted from LR
__global__ void ibp_lr_kernel(const float* est, const uint8_t* lr, int B, int H, int W, int h, int w, int TX, int TY, const int* ix, const float* wx,
                              const int* iy, const float* wy, float* diff) {
    const int64_t n = (int64_t)B * h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % w);
        const int64_t t = i / w;
        const int oy = (int)(t % h);
        const int64_t b = t / h;
        float acc = 0.f;
        for (int j = 0; j < TY; ++j) {
            const float* row = est + (b * H + iy[oy * TY + j]) * W;
            float r = 0.f;
            for (int k = 0; k < TX; ++k) r = add_sep(r, mul_sep(row[ix[ox * TX + k]], wx[ox * TX + k]));
            acc = add_sep(acc, mul_sep(r, wy[oy * TY + j]));
        }
        diff[i] = sub_sep((float)lr[i], acc);
    }
}

// HR pass: the 2-tap linear up-resize of diff added into the estimate; the last iteration also writes the clipped, truncated uint8
__global__ void ibp_hr_kernel(const float* diff, int B, int H, int W, int h, int w, const int* ix, const float* wx, const int* iy, const float* wy,
                              float* est, uint8_t* y) {
    const int64_t n = (int64_t)B * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % W);
        const int64_t t = i / W;
        const int oy = (int)(t % H);
        const int64_t b = t / H;
        float acc = 0.f;
        for (int j = 0; j < 2; ++j) {
            const float* row = diff + (b * h + iy[oy * 2 + j]) * w;
            const float r = add_sep(add_sep(0.f, mul_sep(row[ix[ox * 2]], wx[ox * 2])), mul_sep(row[ix[ox * 2 + 1]], wx[ox * 2 + 1]));
            acc = add_sep(acc, mul_sep(r, wy[oy * 2 + j]));
        }
        const float e = add_sep(est[i], acc);
        est[i] = e;
        if (y) y[i] = (uint8_t)fminf(fmaxf(e, 0.f), 255.f);  // astype(uint8) truncates toward zero
    }
}

// ------------------------------------------------------------------------------------------------
// Noise sigma (skimage estimate_sigma on the uint8 values, 0..255 units): the dd band of pywt.dwtn(x, 'db2') in 'symmetric' mode,
//   d[o] = sum_j dec_hi[j] * x[2 o + 1 - j]   per axis (axis 0 first), (n + 3) / 2 outputs per axis,
// then median(|d| over the non-zero coefficients) / norm.ppf(0.75).  db2's high-pass has two vanishing moments, so it annihilates a
// constant exactly in real arithmetic; each pass is evaluated as sum_j dec_hi[j] * (x_j - x_3) (the dropped (sum dec_hi) * x_3 is
// ~1e-16 * x_3) so that a flat region gives exactly zero, the value that the "non-zero" rule exists to drop.
// ------------------------------------------------------------------------------------------------
__constant__ double DB2_DEC_HI[4] = {-0.48296291314469025, 0.836516303737469, -0.22414386804185735, -0.12940952255092145};

__global__ void db2_hh_abs_kernel(const uint8_t* x, int B, int h, int w, int oh, int ow, double* d) {
    const int64_t n = (int64_t)B * oh * ow;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int o1 = (int)(i % ow);
        const int64_t t = i / ow;
        const int o0 = (int)(t % oh);
        const int64_t b = t / oh;
        const uint8_t* img = x + b * h * w;
        int r[4], c[4];
        for (int j = 0; j < 4; ++j) { r[j] = symmetric_idx(2 * o0 + 1 - j, h); c[j] = symmetric_idx(2 * o1 + 1 - j, w); }
        double col[4];                                       // the axis-0 pass at the four columns the axis-1 pass reads
        for (int q = 0; q < 4; ++q) {
            const double base = (double)img[(int64_t)r[3] * w + c[q]];
            double s = 0.0;
            for (int j = 0; j < 3; ++j) s = add_sep(s, mul_sep(DB2_DEC_HI[j], (double)img[(int64_t)r[j] * w + c[q]] - base));
            col[q] = s;
        }
        double s = 0.0;
        for (int j = 0; j < 3; ++j) s = add_sep(s, mul_sep(DB2_DEC_HI[j], sub_sep(col[j], col[3])));
        d[i] = fabs(s);
    }
}

// exact k-th smallest (0-based) of the non-zero entries of v[0..n): most-significant-digit radix select on the IEEE bit patterns
// (non-negative doubles order as their bit patterns), 8 bits per pass; one workgroup
__device__ double select_kth_nonzero(const double* v, int64_t n, int64_t k, unsigned* hist, unsigned long long* sh) {
    unsigned long long prefix = 0, mask = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned long long u = (unsigned long long)__double_as_longlong(v[i]);
            if (u != 0 && (u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t cum = 0;
            int dg = 255;
            for (int q = 0; q < 256; ++q) {
                if (cum + hist[q] > k) { dg = q; break; }
                cum += hist[q];
            }
            k -= cum;
            sh[0] = (unsigned long long)dg;
            sh[1] = (unsigned long long)k;
        }
        __syncthreads();
        prefix |= sh[0] << shift;
        mask |= 255ull << shift;
        k = (int64_t)sh[1];
        __syncthreads();
    }
    return __longlong_as_double((long long)prefix);
}

__global__ void __launch_bounds__(1024) median_sigma_kernel(const double* d, int64_t per, double* sigma) {
    __shared__ unsigned hist[256];
    __shared__ unsigned long long sh[2];
    __shared__ unsigned long long cnt;
    const double* v = d + (int64_t)blockIdx.x * per;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    unsigned long long c = 0;
    for (int64_t i = threadIdx.x; i < per; i += blockDim.x) c += v[i] != 0.0;
    atomicAdd(&cnt, c);
    __syncthreads();
    const int64_t nz = (int64_t)cnt;
    if (nz == 0) {                                           // numpy's median of nothing: NaN
        if (threadIdx.x == 0) sigma[blockIdx.x] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double lo = select_kth_nonzero(v, per, (nz - 1) / 2, hist, sh);
    const double hi = (nz & 1) ? lo : select_kth_nonzero(v, per, nz / 2, hist, sh);
    if (threadIdx.x == 0) sigma[blockIdx.x] = __ddiv_rn(mul_sep(add_sep(lo, hi), 0.5), 0.6744897501960817);   // even count: the mean of the middle two
}

// ------------------------------------------------------------------------------------------------
// Non-local means, skimage's fast 2-D algorithm (denoise_nl_means(img_as_float(x), h, patch_size, patch_distance, fast_mode=True)),
// reduced per output pixel p of the reflect-padded image P = x / 255 to
//   y[p] = sum_t w(p,t) P[p+t] / sum_t w(p,t),   t in [-d, d]^2,
//   D = sum_{k in [-s, s]^2} (P[p+k] - P[p+t+k])^2,  dist = D / (h^2 patch^2),  w = exp(-dist) if dist <= 5 else 0
// (the alpha = 0.5 double visits of the t_col == 0 shifts give every shift one visit).  The squared differences of the uint8 values
// are integers: D * 255^2 is summed exactly in int32, and only the cutoff test and exp run in fp64.
// One 256-thread workgroup per 32 x 32 output tile: the uint8 tile plus its (s + d) halo in LDS; per shift the squared differences
// over the (32 + 2s)^2 patch region, a horizontal then a vertical box sum, and the weight of each of a thread's four pixels.
// ------------------------------------------------------------------------------------------------
constexpr int NLM_TILE = 32, NLM_MAX_S = 4, NLM_MAX_D = 12;
constexpr int NLM_MAX_TS = NLM_TILE + 2 * (NLM_MAX_S + NLM_MAX_D), NLM_MAX_RS = NLM_TILE + 2 * NLM_MAX_S;

__global__ void __launch_bounds__(256) nlm_kernel(const uint8_t* x, int h, int w, int s, int dmax, const double* sigma, double h_scale,
                                                  float* y) {
    __shared__ int tile[NLM_MAX_TS * NLM_MAX_TS];
    __shared__ int sq[NLM_MAX_RS * NLM_MAX_RS];
    __shared__ int hs[NLM_MAX_RS * NLM_TILE];
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * NLM_TILE, x0 = blockIdx.x * NLM_TILE;
    const int R = s + dmax, TS = NLM_TILE + 2 * R, RS = NLM_TILE + 2 * s, P = 2 * s + 1;
    const uint8_t* img = x + (int64_t)b * h * w;
    for (int i = threadIdx.x; i < TS * TS; i += blockDim.x) {
        const int r = i / TS, c = i - r * TS;
        tile[i] = img[(int64_t)reflect_idx(y0 - R + r, h) * w + reflect_idx(x0 - R + c, w)];
    }
    const double hh = h_scale * sigma[b];
    const double h2s2 = hh * hh * (double)P * (double)P;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    double sw[4] = {0, 0, 0, 0}, swp[4] = {0, 0, 0, 0};
    __syncthreads();
    for (int dy = -dmax; dy <= dmax; ++dy) {
        for (int dx = -dmax; dx <= dmax; ++dx) {
            for (int i = threadIdx.x; i < RS * RS; i += blockDim.x) {          // region origin (-s, -s) of the tile's outputs = tile index dmax
                const int r = i / RS, c = i - r * RS;
                const int dd = tile[(r + dmax) * TS + c + dmax] - tile[(r + dmax + dy) * TS + c + dmax + dx];
                sq[i] = dd * dd;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < RS * NLM_TILE; i += blockDim.x) {
                const int r = i >> 5, c = i & 31;
                int a = 0;
                for (int k = 0; k < P; ++k) a += sq[r * RS + c + k];
                hs[i] = a;
            }
            __syncthreads();
            for (int q = 0; q < 4; ++q) {
                const int r = ty + 8 * q;
                int D = 0;
                for (int k = 0; k < P; ++k) D += hs[(r + k) * NLM_TILE + tx];
                const double dist = __ddiv_rn(__ddiv_rn((double)D, 65025.0), h2s2);
                if (dist <= 5.0) {
                    const double wt = exp(-dist);
                    sw[q] += wt;
                    swp[q] += wt * (double)tile[(r + R + dy) * TS + tx + R + dx];
                }
            }
            // (the next shift's first barrier orders these hs reads before hs is written again)
        }
    }
    for (int q = 0; q < 4; ++q) {
        const int oy = y0 + ty + 8 * q, ox = x0 + tx;
        if (oy < h && ox < w) y[((int64_t)b * h + oy) * w + ox] = (float)(swp[q] / 255.0 / sw[q]);
    }
}

// ------------------------------------------------------------------------------------------------
// Edge-guided interpolation (classic_algorithms.py:64-85): edges = hypot(Sobel_x, Sobel_y) (cv2.Sobel(x, CV_64F, ...), ksize 3,
// BORDER_REFLECT_101; the components are integers, the magnitude fp64), then per HR pixel
//   up   = cv2.resize(x, (W, H), INTER_LINEAR) on uint8: 11-bit fixed-point taps, VResizeLinear<uchar>'s rounding
//   up_e = cv2.resize(edges, (W, H)) on float64: double arithmetic with the float tap weights
//   out  = clip(addWeighted(float32(up), 1.0, float32(up_e), weight, 0), 0, 255).astype(uint8)
// addWeighted on 32F images casts its weights to float and computes src1 * a + src2 * b + g in float (each step rounded).
// ------------------------------------------------------------------------------------------------
__global__ void sobel_mag_kernel(const uint8_t* x, int B, int h, int w, double* e) {
    const int64_t n = (int64_t)B * h * w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % w);
        const int64_t t = i / w;
        const int r = (int)(t % h);
        const uint8_t* img = x + (t / h) * h * w;
        const int rm = reflect101_idx(r - 1, h), rp = reflect101_idx(r + 1, h), cm = reflect101_idx(c - 1, w), cp = reflect101_idx(c + 1, w);
        auto at = [&](int rr, int cc) { return (int)img[(int64_t)rr * w + cc]; };
        const int gx = (at(rm, cp) - at(rm, cm)) + 2 * (at(r, cp) - at(r, cm)) + (at(rp, cp) - at(rp, cm));
        const int gy = (at(rp, cm) - at(rm, cm)) + 2 * (at(rp, c) - at(rm, c)) + (at(rp, cp) - at(rm, cp));
        e[i] = hypot((double)gx, (double)gy);
    }
}

__global__ void egi_hr_kernel(const uint8_t* x, const double* e, int B, int h, int w, int H, int W, const int* ix, const float* wx, const int* iwx,
                              const int* iy, const float* wy, const int* iwy, float weight, uint8_t* y, float* up_e) {
    const int64_t n = (int64_t)B * H * W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ox = (int)(i % W);
        const int64_t t = i / W;
        const int oy = (int)(t % H);
        const int64_t b = t / H;
        long long rows[2];
        double erow[2];
        for (int j = 0; j < 2; ++j) {
            const int64_t ro = (b * h + iy[oy * 2 + j]) * w;
            rows[j] = (long long)x[ro + ix[ox * 2]] * iwx[ox * 2] + (long long)x[ro + ix[ox * 2 + 1]] * iwx[ox * 2 + 1];
            erow[j] = add_sep(mul_sep(e[ro + ix[ox * 2]], (double)wx[ox * 2]), mul_sep(e[ro + ix[ox * 2 + 1]], (double)wx[ox * 2 + 1]));
        }
        const long long v = (((iwy[oy * 2] * (rows[0] >> 4)) >> 16) + ((iwy[oy * 2 + 1] * (rows[1] >> 4)) >> 16) + 2) >> 2;   // VResizeLinear<uchar>
        const float up = (float)min(max(v, 0ll), 255ll);
        const float ue = (float)add_sep(mul_sep(erow[0], (double)wy[oy * 2]), mul_sep(erow[1], (double)wy[oy * 2 + 1]));
        if (up_e) up_e[i] = ue;
        const float s = add_sep(add_sep(mul_sep(up, 1.0f), mul_sep(ue, weight)), 0.0f);
        y[i] = (uint8_t)fminf(fmaxf(s, 0.f), 255.f);
    }
}

// ------------------------------------------------------------------------------------------------
// Frequency extrapolation (classic_algorithms.py:87-108): abs(ifft2(ifftshift(zero-pad(fftshift(fft2(x)))))) is the separable linear map
//   Y = | A_H X A_W^T |,   A_{N,n}[y, x] = (1/N) sum_{k = -(n/2)}^{n-1-n/2} exp(2 pi i k (y n - x N) / (N n)),
// with the phase reduced exactly in integers (m = k (y n - x N) mod N n).  A is real for odd n (the imaginary parts cancel pairwise).
// The operators are built once per shape and kept on the context; the two products are fp64 FMA GEMMs, abs in the second's epilogue.
// ------------------------------------------------------------------------------------------------
__global__ void dft_operator_kernel(int N, int n, double* re, double* im) {
    const int64_t total = (int64_t)N * n;
    const int64_t Nn = (int64_t)N * n;
    const int k0 = -(n / 2), k1 = n - 1 - n / 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t yy = i / n, xx = i % n;
        const int64_t base = yy * n - xx * N;
        double sr = 0.0, si = 0.0;
        for (int k = k0; k <= k1; ++k) {
            int64_t m = ((int64_t)k * base) % Nn;
            if (m < 0) m += Nn;
            double sn, cs;
            sincospi(2.0 * (double)m / (double)Nn, &sn, &cs);
            sr += cs;
            si += sn;
        }
        re[i] = sr / (double)N;
        if (im) im[i] = si / (double)N;
    }
}

__global__ void u8_to_f64_kernel(const uint8_t* x, int64_t n, double* y) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = (double)x[i];
}

// A_{N,n} of one shape: [N][n] real parts, then (n even) [N][n] imaginary parts; built once per context and shape
int dft_operator(sr_ctx* ctx, int N, int n, hipStream_t st, const double** re, const double** im) {
    const int64_t key = ((int64_t)N << 32) | (uint32_t)n;
    auto it = ctx->dft_ops.find(key);
    if (it == ctx->dft_ops.end()) {
        const bool cplx = (n % 2) == 0;
        const int64_t nel = (int64_t)N * n;
        double* p = static_cast<double*>(ctx->dalloc(sizeof(double) * (size_t)nel * (cplx ? 2 : 1)));
        if (!p) return SR_ERR_OOM;
        hipLaunchKernelGGL(dft_operator_kernel, dim3(cls_grid(nel)), dim3(256), 0, st, N, n, p, cplx ? p + nel : nullptr);
        SR_HIP(ctx, hipGetLastError());
        SR_HIP(ctx, hipStreamSynchronize(st));      // once per shape: later calls may come on other streams
        it = ctx->dft_ops.emplace(key, p).first;
    }
    *re = it->second;
    *im = (n % 2) == 0 ? it->second + (int64_t)N * n : nullptr;
    return SR_OK;
}

struct Taps { int* ix; float* wx; int* iwx; int* iy; float* wy; int* iwy; };

// one axis pair of tap tables in `base` (with fixed-point weights when `fixed`); returns the first byte after them
char* build_taps(char* base, int Hs, int Ws, int Hd, int Wd, int interp, int TX, int TY, bool fixed, Taps* t, hipStream_t st) {
    t->ix = reinterpret_cast<int*>(base);
    t->wx = reinterpret_cast<float*>(t->ix + (size_t)Wd * TX);
    t->iwx = reinterpret_cast<int*>(t->wx + (size_t)Wd * TX);
    t->iy = t->iwx + (fixed ? (size_t)Wd * TX : 0);
    t->wy = reinterpret_cast<float*>(t->iy + (size_t)Hd * TY);
    t->iwy = reinterpret_cast<int*>(t->wy + (size_t)Hd * TY);
    if (!fixed) { t->iwx = nullptr; }
    hipLaunchKernelGGL(resize_taps_kernel, dim3((Wd + 255) / 256), dim3(256), 0, st, Ws, Wd, interp, 0, TX, t->ix, t->wx, t->iwx);
    hipLaunchKernelGGL(resize_taps_kernel, dim3((Hd + 255) / 256), dim3(256), 0, st, Hs, Hd, interp, 0, TY, t->iy, t->wy, fixed ? t->iwy : nullptr);
    char* end = reinterpret_cast<char*>(t->iwy + (fixed ? (size_t)Hd * TY : 0));
    if (!fixed) t->iwy = nullptr;
    return end;
}

size_t taps_bytes(int Hd, int Wd, int TX, int TY) { return ((size_t)Wd * TX + (size_t)Hd * TY) * 12; }

}  // namespace

extern "C" {

int sr_back_projection(sr_ctx* ctx, const uint8_t* hr_u8, const uint8_t* lr_u8, int B, int H, int W, int h, int w, int iterations, uint8_t* y_u8,
                       float* y_f32, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!hr_u8 || !lr_u8 || !y_u8) return ctx->fail(SR_ERR_INVALID, "back_projection: null tensor");
    if (!dims_ok(B, H, W) || !dims_ok(B, h, w)) return ctx->fail(SR_ERR_INVALID, "back_projection: empty or oversized batch");
    if (H < h || W < w) return ctx->fail(SR_ERR_INVALID, "back_projection: the first image must be at least the size of the second (HR estimate, LR observation)");
    if (iterations < 0) return ctx->fail(SR_ERR_INVALID, "back_projection: iterations must be >= 0");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nH = (int64_t)B * H * W, nL = (int64_t)B * h * w;
    // down-resize with sr_resize's rules: INTER_LINEAR, or the 2 x 2 area mean when both axes halve exactly
    const int down = (W == 2 * w && H == 2 * h) ? 3 : 1;
    const int TXd = down == 3 ? (int)ceil((double)W / w) + 2 : 2, TYd = down == 3 ? (int)ceil((double)H / h) + 2 : 2;
    const size_t tb = taps_bytes(h, w, TXd, TYd) + taps_bytes(H, W, 2, 2) + 64;
    const size_t wb = sizeof(float) * (size_t)(nL + (y_f32 ? 0 : nH));
    char* tabs = static_cast<char*>(ctx->arena(ctx->cls_tab, tb, st));
    float* work = static_cast<float*>(ctx->arena(ctx->cls_work, wb, st));
    if (!tabs || !work) return SR_ERR_OOM;
    Taps td, tu;
    char* next = build_taps(tabs, H, W, h, w, down, TXd, TYd, false, &td, st);
    next = reinterpret_cast<char*>(((uintptr_t)next + 15) & ~(uintptr_t)15);
    build_taps(next, h, w, H, W, 1, 2, 2, false, &tu, st);
    float* diff = work;
    float* est = y_f32 ? y_f32 : work + nL;
    hipLaunchKernelGGL(ibp_init_kernel, dim3(cls_grid(nH)), dim3(256), 0, st, hr_u8, nH, est, iterations == 0 ? y_u8 : nullptr);
    for (int it = 0; it < iterations; ++it) {
        hipLaunchKernelGGL(ibp_lr_kernel, dim3(cls_grid(nL)), dim3(256), 0, st, est, lr_u8, B, H, W, h, w, TXd, TYd, td.ix, td.wx, td.iy, td.wy, diff);
        hipLaunchKernelGGL(ibp_hr_kernel, dim3(cls_grid(nH)), dim3(256), 0, st, diff, B, H, W, h, w, tu.ix, tu.wx, tu.iy, tu.wy, est,
                           it == iterations - 1 ? y_u8 : nullptr);
    }
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_noise_sigma(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, double* sigma_f64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x_u8 || !sigma_f64) return ctx->fail(SR_ERR_INVALID, "noise_sigma: null tensor");
    if (!dims_ok(B, h, w)) return ctx->fail(SR_ERR_INVALID, "noise_sigma: empty or oversized batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int oh = (h + 3) / 2, ow = (w + 3) / 2;
    const int64_t per = (int64_t)oh * ow, n = (int64_t)B * per;
    double* d = static_cast<double*>(ctx->arena(ctx->cls_work, sizeof(double) * (size_t)n, st));
    if (!d) return SR_ERR_OOM;
    hipLaunchKernelGGL(db2_hh_abs_kernel, dim3(cls_grid(n)), dim3(256), 0, st, x_u8, B, h, w, oh, ow, d);
    hipLaunchKernelGGL(median_sigma_kernel, dim3(B), dim3(1024), 0, st, d, per, sigma_f64);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_nl_means(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int patch, int distance, const double* sigma_f64, double h_scale, float* y_f32,
                void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x_u8 || !sigma_f64 || !y_f32) return ctx->fail(SR_ERR_INVALID, "nl_means: null tensor");
    if (!dims_ok(B, h, w) || B > 65535) return ctx->fail(SR_ERR_INVALID, "nl_means: empty or oversized batch (B <= 65535)");
    if (patch < 1 || patch % 2 == 0 || patch / 2 > NLM_MAX_S)
        return ctx->fail(SR_ERR_INVALID, "nl_means: patch_size must be odd and at most " + std::to_string(2 * NLM_MAX_S + 1));
    if (distance < 0 || distance > NLM_MAX_D) return ctx->fail(SR_ERR_INVALID, "nl_means: patch_distance must be in [0, " + std::to_string(NLM_MAX_D) + "]");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((w + NLM_TILE - 1) / NLM_TILE, (h + NLM_TILE - 1) / NLM_TILE, B);
    hipLaunchKernelGGL(nlm_kernel, grid, dim3(256), 0, st, x_u8, h, w, patch / 2, distance, sigma_f64, h_scale, y_f32);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_edge_guided(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int H, int W, float weight, uint8_t* y_u8, float* up_e_f32, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x_u8 || !y_u8) return ctx->fail(SR_ERR_INVALID, "edge_guided: null tensor");
    if (!dims_ok(B, h, w) || !dims_ok(B, H, W)) return ctx->fail(SR_ERR_INVALID, "edge_guided: empty or oversized batch");
    if (H < h || W < w) return ctx->fail(SR_ERR_INVALID, "edge_guided: the output must be at least the input's size (an up-scaler)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t nL = (int64_t)B * h * w, nH = (int64_t)B * H * W;
    char* tabs = static_cast<char*>(ctx->arena(ctx->cls_tab, taps_bytes(H, W, 2, 2), st));
    double* e = static_cast<double*>(ctx->arena(ctx->cls_work, sizeof(double) * (size_t)nL, st));
    if (!tabs || !e) return SR_ERR_OOM;
    Taps t;
    build_taps(tabs, h, w, H, W, 1, 2, 2, true, &t, st);
    hipLaunchKernelGGL(sobel_mag_kernel, dim3(cls_grid(nL)), dim3(256), 0, st, x_u8, B, h, w, e);
    hipLaunchKernelGGL(egi_hr_kernel, dim3(cls_grid(nH)), dim3(256), 0, st, x_u8, e, B, h, w, H, W, t.ix, t.wx, t.iwx, t.iy, t.wy, t.iwy, weight, y_u8, up_e_f32);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_freq_extrapolate(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int H, int W, double* y_f64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x_u8 || !y_f64) return ctx->fail(SR_ERR_INVALID, "freq_extrapolate: null tensor");
    if (!dims_ok(B, h, w) || !dims_ok(B, H, W) || B > 65535) return ctx->fail(SR_ERR_INVALID, "freq_extrapolate: empty or oversized batch (B <= 65535)");
    if (H < h || W < w) return ctx->fail(SR_ERR_INVALID, "freq_extrapolate: the output size must be at least the input size (zero-padding a spectrum)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const double *ahr, *ahi, *awr, *awi;
    if (int rc = dft_operator(ctx, H, h, st, &ahr, &ahi)) return rc;
    if (int rc = dft_operator(ctx, W, w, st, &awr, &awi)) return rc;
    const int64_t nx = (int64_t)B * h * w, nt = (int64_t)B * h * W;
    const bool t_cplx = awi != nullptr;
    double* xd = static_cast<double*>(ctx->arena(ctx->cls_fft, sizeof(double) * (size_t)(nx + nt * (t_cplx ? 2 : 1)), st));
    if (!xd) return SR_ERR_OOM;
    double* tr = xd + nx;
    double* ti = t_cplx ? tr + nt : nullptr;
    hipLaunchKernelGGL(u8_to_f64_kernel, dim3(cls_grid(nx)), dim3(256), 0, st, x_u8, nx, xd);
    // T = X . A_W^T  (M = h, K = w, N = W; B(k, j) = A_W[j][k])
    cgemm_dispatch<CG_STORE>(false, t_cplx, dim3((W + GT - 1) / GT, (h + GT - 1) / GT, B), st, h, W, w, xd, nullptr, w, 1, (int64_t)h * w, awr, awi, 1, w, 0,
                          tr, ti, (int64_t)h * W);
    // Y = | A_H . T |  (M = H, K = h, N = W)
    cgemm_dispatch<CG_ABS>(ahi != nullptr, t_cplx, dim3((W + GT - 1) / GT, (H + GT - 1) / GT, B), st, H, W, h, ahr, ahi, h, 1, 0, tr, ti, W, 1, (int64_t)h * W,
                         y_f64, nullptr, (int64_t)H * W);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
