// metrics.hip -- the image-quality scores of the reference's classical study (skimage's peak_signal_noise_ratio / structural_similarity
// and classic_super_resolution_algorithms/profiling_methods.py:45-167), for B pairs (hr, sr) of one shape [H, W] or [H, W, 3], each image
// uint8 or float32.  Per pair nine fp64 numbers (SR_SCORE_* in include/sr355.h): psnr, ssim, mae, rmse, grad_mse, epi, hf_ratio, kl_luma,
// kl_color.
//
//   1. scale-flag pass: per image, max(gray) > 1.5 (_ensure_gray_f32 divides that image by 255 before its Sobel).  A separate cheap pass,
//      so that the Sobel magnitudes are final when they are summed (keeping sum M, sum M^2, sum M_hr M_sr and scaling at the end would
//      lose grad_mse = 0 for identical images to cancellation).
//   2. pair-statistics pass: one 256-thread workgroup per 32 x 32 tile reads the tile of hr and sr with a 3-pixel halo (the SSIM window)
//      into LDS, and the gray tile with a 1-pixel BORDER_REFLECT_101 halo (the Sobel reach); it sums |d|, d^2, M_hr, M_sr, (M_hr - M_sr)^2
//      and the SSIM map over the centres whose 7 x 7 window lies inside the image (skimage's crop of 3), and counts the 256-bin gray and
//      3 x 64-bin colour histograms in LDS, merged into global int32 counts (integer atomics, one per non-empty bin per workgroup).
//      When both images are uint8 every box sum, Sobel component and squared difference is an exact int32; fp64 from there on.
//   3. high-frequency energy: |fftshift(fft2(gray))| summed over r > radius_frac (r_max + 1e-9) as the separable DFT F = A_H X A_W^T,
//      A_N[k, x] = exp(-2 pi i k x / N), by cgemm_f64.h's fp64 GEMMs (real x complex, then complex x complex with the masked |F| sum in the
//      epilogue, one partial per workgroup), in chunks of images that bound the intermediates.
//   4. finalize: one workgroup per pair sums the per-tile partials in a fixed order and applies the logs and divisions.
// No float atomics anywhere: a pair's scores are the same bits on every run and do not depend on B or on the other pairs.
//
//   5. (below the scores) the study's loop glue and similarity maps, entry points of their own: sr_rgb2gray_u8, sr_freq_to_u8 and
//      sr_ssim_map, the pair-statistics pass's SSIM part over the whole image with scipy's 'reflect' border.
#include "cgemm_f64.h"
#include "common.h"
#include "fp_sep.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace {

constexpr int MT = 32;                 // output tile edge
constexpr int MHW = 3;                 // SSIM half window (7 x 7)
constexpr int MR = MT + 2 * MHW;       // raw region edge (38)
constexpr int MG = MT + 2;             // gray region edge with the Sobel halo (34)
constexpr int NPART = 8;               // per-tile partials: sum |d|, sum d^2, sum M_hr, sum M_sr, sum (M_hr - M_sr)^2, sum S of channels 0..2
constexpr int LBINS = 256, CBINS = 64;
constexpr size_t FFT_CHUNK_BYTES = (size_t)256 << 20;   // cap on the DFT intermediates (X, T) of one chunk

inline unsigned met_grid(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

__device__ inline int refl101(int i, int n) {
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

__device__ inline float ld_val(const void* p, int dt, int64_t i) {
    return dt == SR_DTYPE_U8 ? (float)static_cast<const uint8_t*>(p)[i] : static_cast<const float*>(p)[i];
}

// OpenCV's 8-bit COLOR_RGB2GRAY of one interleaved RGB pixel: common.h's fixed-point statement with the channels in RGB order.  The one
// gray conversion of this file: the scores' gray-derived columns and sr_rgb2gray_u8 both go through it.
__device__ inline int gray_rgb_u8(const uint8_t* q) { return gray_bgr((int)q[2], (int)q[1], (int)q[0]); }

// the gray value the gray-derived columns see at pixel `pix` of one image, unscaled: the value itself for one channel; for uint8 RGB
// OpenCV's COLOR_RGB2GRAY fixed point (14-bit coefficients, rounded).  Float RGB never reaches here (gray_ok is false).
__device__ inline float gray_val(const void* img, int dt, int C, int64_t pix) {
    if (C == 1) return ld_val(img, dt, pix);
    return (float)gray_rgb_u8(static_cast<const uint8_t*>(img) + pix * 3);
}

// what np.histogram(range=(0, 255)) bins: uint8 as float32, float as clip(x, 0, 1) * 255 in float32
__device__ inline double hist_val(float x, int dt) {
    return dt == SR_DTYPE_U8 ? (double)x : (double)mul_sep(fminf(fmaxf(x, 0.f), 1.f), 255.f);
}

// np.histogram's bin of v in [0, 255] with `bins` equal bins: ((v - 0) / 255) * bins truncated, the right edge folded into the last bin,
// then the one-step corrections against the linspace edges i * (255 / bins) (exact products for 256 and 64 bins)
__device__ inline int hist_bin(double v, int bins) {
    const double step = 255.0 / bins;
    int i = (int)((v / 255.0) * bins);
    if (i >= bins) i = bins - 1;
    if (v < (double)i * step) --i;
    if (i != bins - 1 && v >= (double)(i + 1) * step) ++i;
    return i;
}

__device__ inline const void* image_of(const void* hr, int hr_dt, const void* sr, int sr_dt, int g, int64_t per, int* dt) {
    const int which = g & 1;
    *dt = which ? sr_dt : hr_dt;
    const void* base = which ? sr : hr;
    const int64_t off = (int64_t)(g >> 1) * per;
    return *dt == SR_DTYPE_U8 ? static_cast<const void*>(static_cast<const uint8_t*>(base) + off)
                              : static_cast<const void*>(static_cast<const float*>(base) + off);
}

// ------------------------------------------------------------------------------------------------
// 1. scale flags: flag[2 b + {0: hr, 1: sr}] = max(gray) > 1.5; grid (2 B, chunks), 16 pixels per thread, one integer atomic per workgroup
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gray_scale_flag_kernel(const void* hr, int hr_dt, const void* sr, int sr_dt, int C, int64_t HW, int* flag) {
    const int g = blockIdx.x;
    int dt;
    const void* img = image_of(hr, hr_dt, sr, sr_dt, g, HW * C, &dt);
    bool big = false;
    for (int64_t i = (int64_t)blockIdx.y * 256 * 16 + threadIdx.x, e = min((int64_t)(blockIdx.y + 1) * 256 * 16, HW); i < e; i += 256)
        big |= gray_val(img, dt, C, i) > 1.5f;
    if (__syncthreads_or(big) && threadIdx.x == 0) atomicOr(&flag[g], 1);
}

__device__ double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// ------------------------------------------------------------------------------------------------
// 2. pair statistics.  INT: both images uint8 (LDS and sums in int32); otherwise LDS holds float32 and the sums run in fp64.
//    part[(b * ntiles + tile) * NPART + k]; hist_l [B][2][256], hist_c [B][2][3][64] (zeroed before); gray_out / sobel_out [B][2][H][W]
//    (may be NULL): the unscaled gray image and the Sobel magnitude of _ensure_gray_f32's image.
// ------------------------------------------------------------------------------------------------
template <bool INT>
__global__ void __launch_bounds__(256) pair_stats_kernel(const void* hr, int hr_dt, const void* sr, int sr_dt, int H, int W, int C, int gray_ok,
                                                         const int* flag, const double* dr, double* part, int* hist_l, int* hist_c,
                                                         float* gray_out, float* sobel_out) {
    using S = typename std::conditional<INT, int, float>::type;
    __shared__ S raw[2][3][MR * MR];
    __shared__ S gry[2][MG * MG];
    __shared__ int hl[2][LBINS];
    __shared__ int hc[2][3][CBINS];
    __shared__ double red[256];
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * MT, x0 = blockIdx.x * MT;
    const int tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    int dts[2];
    const void* img[2] = {image_of(hr, hr_dt, sr, sr_dt, 2 * b, HW * C, &dts[0]), image_of(hr, hr_dt, sr, sr_dt, 2 * b + 1, HW * C, &dts[1])};

    for (int i = tid; i < 2 * LBINS; i += 256) (&hl[0][0])[i] = 0;
    for (int i = tid; i < 2 * 3 * CBINS; i += 256) (&hc[0][0][0])[i] = 0;
    for (int i = tid; i < MR * MR * C; i += 256) {                     // channel fastest: coalesced on interleaved RGB
        const int p = i / C, c = i - p * C;
        const int r = p / MR, cc = p - r * MR;
        const int y = y0 - MHW + r, x = x0 - MHW + cc;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const int64_t o = ((int64_t)y * W + x) * C + c;
        for (int k = 0; k < 2; ++k) raw[k][c][p] = in ? (S)ld_val(img[k], dts[k], o) : (S)0;
    }
    if (gray_ok)
        for (int i = tid; i < MG * MG; i += 256) {
            const int r = i / MG, cc = i - r * MG;
            const int y = y0 - 1 + r, x = x0 - 1 + cc;
            if (y > H || x > W) {                                         // beyond the reach of the image's last row / column
                gry[0][i] = gry[1][i] = (S)0;
                continue;
            }
            const int64_t pix = (int64_t)refl101(y, H) * W + refl101(x, W);
            for (int k = 0; k < 2; ++k) gry[k][i] = (S)gray_val(img[k], dts[k], C, pix);
        }
    __syncthreads();

    const bool scale[2] = {flag[2 * b] != 0, flag[2 * b + 1] != 0};
    const double R = dr[b];
    const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
    const double cov_norm = 49.0 / 48.0;
    double acc[NPART] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, r = p >> 5, cc = p & 31;
        const int y = y0 + r, x = x0 + cc;
        if (y >= H || x >= W) continue;
        const int rp = (r + MHW) * MR + cc + MHW;
        for (int c = 0; c < C; ++c) {
            if (INT) {
                const int d = (int)raw[0][c][rp] - (int)raw[1][c][rp];
                acc[0] += (double)abs(d);
                acc[1] += (double)(d * d);
            } else {
                const double d = (double)raw[0][c][rp] - (double)raw[1][c][rp];
                acc[0] += fabs(d);
                acc[1] += d * d;
            }
        }
        if (gray_ok) {
            double m[2];
            for (int k = 0; k < 2; ++k) {
                const S* g = &gry[k][(r + 1) * MG + cc + 1];
                if (INT) {
                    auto at = [&](int dy, int dx) { return (int)g[dy * MG + dx]; };
                    const int gx = (at(-1, 1) - at(-1, -1)) + 2 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1));
                    const int gy = (at(1, -1) - at(-1, -1)) + 2 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1));
                    m[k] = sqrt((double)(gx * gx + gy * gy));
                    if (scale[k]) m[k] /= 255.0;
                } else {
                    const bool sc = scale[k];
                    auto at = [&](int dy, int dx) { const float v = (float)g[dy * MG + dx]; return (double)(sc ? __fdiv_rn(v, 255.f) : v); };
                    const double gx = (at(-1, 1) - at(-1, -1)) + 2.0 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1));
                    const double gy = (at(1, -1) - at(-1, -1)) + 2.0 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1));
                    m[k] = sqrt(gx * gx + gy * gy);
                }
                const float gv = (float)g[0];
                atomicAdd(&hl[k][hist_bin(hist_val(gv, C == 1 ? dts[k] : SR_DTYPE_U8), LBINS)], 1);
                const int64_t o = ((int64_t)(2 * b + k) * H + y) * W + x;
                if (gray_out) gray_out[o] = gv;
                if (sobel_out) sobel_out[o] = (float)m[k];
            }
            acc[2] += m[0];
            acc[3] += m[1];
            acc[4] += (m[0] - m[1]) * (m[0] - m[1]);
        }
        if (C == 3)
            for (int k = 0; k < 2; ++k)
                for (int c = 0; c < 3; ++c) atomicAdd(&hc[k][c][hist_bin(hist_val((float)raw[k][c][rp], dts[k]), CBINS)], 1);
        if (y >= MHW && y < H - MHW && x >= MHW && x < W - MHW) {
            for (int c = 0; c < C; ++c) {
                double ux, uy, uxx, uyy, uxy;
                if (INT) {
                    int sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                    for (int i = 0; i < 7; ++i)
                        for (int j = 0; j < 7; ++j) {
                            const int a = raw[0][c][(r + i) * MR + cc + j], v = raw[1][c][(r + i) * MR + cc + j];
                            sa += a; sb += v; saa += a * a; sbb += v * v; sab += a * v;
                        }
                    ux = sa / 49.0; uy = sb / 49.0; uxx = saa / 49.0; uyy = sbb / 49.0; uxy = sab / 49.0;
                } else {
                    double sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                    for (int i = 0; i < 7; ++i)
                        for (int j = 0; j < 7; ++j) {
                            const double a = raw[0][c][(r + i) * MR + cc + j], v = raw[1][c][(r + i) * MR + cc + j];
                            sa += a; sb += v; saa += a * a; sbb += v * v; sab += a * v;
                        }
                    ux = sa / 49.0; uy = sb / 49.0; uxx = saa / 49.0; uyy = sbb / 49.0; uxy = sab / 49.0;
                }
                const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
                const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
                acc[5 + c] += (A1 * A2) / (B1 * B2);
            }
        }
    }
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    double* out = part + ((int64_t)b * gridDim.x * gridDim.y + tile) * NPART;
    for (int k = 0; k < NPART; ++k) {
        const double s = block_sum(acc[k], red);                         // (its barriers also order the LDS histogram adds before the merge)
        if (tid == 0) out[k] = s;
    }
    if (gray_ok)
        for (int i = tid; i < 2 * LBINS; i += 256) {
            const int v = (&hl[0][0])[i];
            if (v) atomicAdd(&hist_l[(int64_t)b * 2 * LBINS + i], v);
        }
    if (C == 3)
        for (int i = tid; i < 2 * 3 * CBINS; i += 256) {
            const int v = (&hc[0][0][0])[i];
            if (v) atomicAdd(&hist_c[(int64_t)b * 2 * 3 * CBINS + i], v);
        }
}

// ------------------------------------------------------------------------------------------------
// 3. the DFT operand: fp64 gray planes of images g0 .. g0 + n - 1 (image g = 2 b + {0: hr, 1: sr}), unscaled
// ------------------------------------------------------------------------------------------------
__global__ void gray_f64_kernel(const void* hr, int hr_dt, const void* sr, int sr_dt, int C, int64_t HW, int g0, int64_t n, double* X) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * HW; i += (int64_t)gridDim.x * blockDim.x) {
        int dt;
        const int64_t gi = i / HW;
        const void* img = image_of(hr, hr_dt, sr, sr_dt, g0 + (int)gi, HW * C, &dt);
        X[i] = (double)gray_val(img, dt, C, i - gi * HW);
    }
}

// (dft_full_operator, the cached N x N operator A_N[k][x] = exp(-2 pi i k x / N), lives in cgemm_f64.h: eda.hip shares it)

// ------------------------------------------------------------------------------------------------
// 4. finalize: one workgroup per pair -> out[b][9]
// ------------------------------------------------------------------------------------------------
__device__ inline double kl_term(int p, int q, double step, double n) {
    const double P = (double)p / step / n + 1e-12, Q = (double)q / step / n + 1e-12;
    return P * log(P / Q);
}

__global__ void __launch_bounds__(256) scores_finalize_kernel(const double* part, int ntiles, const int* hist_l, const int* hist_c, const double* hfp, int nhf,
                                                              const double* dr, int H, int W, int C, int gray_ok, double* out) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s[NPART];
    for (int k = 0; k < NPART; ++k) {
        double v = 0.0;
        for (int t = tid; t < ntiles; t += 256) v += part[((int64_t)b * ntiles + t) * NPART + k];
        s[k] = block_sum(v, red);
    }
    double hf[2] = {0.0, 0.0};
    if (gray_ok)
        for (int k = 0; k < 2; ++k) {
            double v = 0.0;
            for (int t = tid; t < nhf; t += 256) v += hfp[(int64_t)(2 * b + k) * nhf + t];
            hf[k] = block_sum(v, red);
        }
    const double npix = (double)H * W;
    double kl_l = 0.0, kl_c = 0.0;
    if (gray_ok) {
        const int* h = hist_l + (int64_t)b * 2 * LBINS;
        kl_l = block_sum(kl_term(h[tid], h[LBINS + tid], 255.0 / LBINS, npix), red);
    }
    if (C == 3) {
        const int* h = hist_c + (int64_t)b * 2 * 3 * CBINS;
        for (int c = 0; c < 3; ++c)
            kl_c += block_sum(tid < CBINS ? kl_term(h[c * CBINS + tid], h[3 * CBINS + c * CBINS + tid], 255.0 / CBINS, npix) : 0.0, red);
    }
    if (tid != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const double n = npix * C, mse = s[1] / n, R = dr[b];
    const double ncen = (double)(H - 2 * MHW) * (double)(W - 2 * MHW);
    double* o = out + (int64_t)b * SR_NUM_SCORES;
    o[SR_SCORE_PSNR] = 10.0 * log10((R * R) / mse);
    o[SR_SCORE_SSIM] = C == 1 ? s[5] / ncen : ((s[5] / ncen + s[6] / ncen) + s[7] / ncen) / 3.0;
    o[SR_SCORE_MAE] = s[0] / n;
    o[SR_SCORE_RMSE] = sqrt(mse + 1e-9);
    o[SR_SCORE_GRAD_MSE] = gray_ok ? s[4] / npix : nan;
    o[SR_SCORE_EPI] = gray_ok ? (s[3] + 1e-9) / (s[2] + 1e-9) : nan;
    o[SR_SCORE_HF_RATIO] = gray_ok ? (hf[1] + 1e-9) / (hf[0] + 1e-9) : nan;
    o[SR_SCORE_KL_LUMA] = gray_ok ? kl_l : nan;
    o[SR_SCORE_KL_COLOR] = C == 3 ? kl_c / 3.0 : nan;
}

// ------------------------------------------------------------------------------------------------
// 5. the classical study's loop glue (super_resolucion_clasica.ipynb cell 8) and the SSIM similarity maps (visualization_methods.py:553-591)
// ------------------------------------------------------------------------------------------------
// cv2.cvtColor(x, COLOR_RGB2GRAY) on B uint8 images, taken as one run of npix interleaved pixels: a thread converts four pixels.  VEC: both
// pointers are 4-byte aligned, so the twelve input bytes are three dword loads and the four gray bytes one dword store; a row length
// plays no part (the images are dense), and a misaligned tensor takes the byte path.
template <bool VEC>
__global__ void __launch_bounds__(256) rgb2gray_kernel(const uint8_t* x, uint8_t* y, int64_t npix) {
    const int64_t ngroups = (npix + 3) / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < ngroups; i += (int64_t)gridDim.x * 256) {
        const int64_t p = i * 4;
        if (VEC && p + 4 <= npix) {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(x + p * 3);
            const uint32_t w[3] = {q[0], q[1], q[2]};
            uint8_t px[12];
            for (int k = 0; k < 12; ++k) px[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            uint32_t o = 0;
            for (int k = 0; k < 4; ++k) o |= (uint32_t)gray_rgb_u8(px + 3 * k) << (8 * k);
            *reinterpret_cast<uint32_t*>(y + p) = o;
        } else {
            for (int k = 0; k < 4 && p + k < npix; ++k) y[p + k] = (uint8_t)gray_rgb_u8(x + (p + k) * 3);
        }
    }
}

// np.max's answer for two values: the larger one, a NaN once met stays
__device__ inline double max_nan(double m, double v) { return (v > m || v != v) ? v : m; }

__device__ double block_max(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = max_nan(red[threadIdx.x], red[threadIdx.x + w]);
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

constexpr int FQ_PER_WG = 256 * 16;   // elements of one image a workgroup of the two freq_to_u8 kernels covers

// pmax[b * nchunk + chunk] = max over the chunk's elements of image b; grid (nchunk, B)
__global__ void __launch_bounds__(256) freq_chunk_max_kernel(const double* f, int64_t per, double* pmax) {
    __shared__ double red[256];
    const double* img = f + (int64_t)blockIdx.y * per;
    const int64_t i0 = (int64_t)blockIdx.x * FQ_PER_WG, e = min(i0 + FQ_PER_WG, per);
    double m = img[i0];                                                // i0 < per: the grid has ceil(per / FQ_PER_WG) chunks
    for (int64_t i = i0 + threadIdx.x; i < e; i += 256) m = max_nan(m, img[i]);
    m = block_max(m, red);
    if (threadIdx.x == 0) pmax[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = m;
}

// cell 8's `(f / np.max(f) * 255.0).astype(np.uint8) if np.max(f) > 0 else f.astype(np.uint8)`: every workgroup folds the image's chunk
// maxima in one fixed order, then divides and multiplies in fp64 (correctly rounded, in that order) and truncates toward zero
__global__ void __launch_bounds__(256) freq_to_u8_kernel(const double* f, int64_t per, const double* pmax, uint8_t* y, double* mx_out) {
    __shared__ double red[256];
    const int b = blockIdx.y, nchunk = gridDim.x;
    double m = pmax[(int64_t)b * nchunk];
    for (int t = threadIdx.x; t < nchunk; t += 256) m = max_nan(m, pmax[(int64_t)b * nchunk + t]);
    const double mx = block_max(m, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) mx_out[b] = mx;
    const bool scale = mx > 0.0;
    const double* img = f + (int64_t)b * per;
    uint8_t* out = y + (int64_t)b * per;
    for (int64_t i = (int64_t)blockIdx.x * FQ_PER_WG + threadIdx.x, e = min((int64_t)(blockIdx.x + 1) * FQ_PER_WG, per); i < e; i += 256) {
        const double v = img[i];
        out[i] = (uint8_t)(long long)(scale ? mul_sep(__ddiv_rn(v, mx), 255.0) : v);
    }
}

// scipy.ndimage.uniform_filter's default mode='reflect' (d c b a | a b c d, NumPy's 'symmetric'): the edge pixel is repeated.  One
// reflection reaches every coordinate the 7 x 7 window asks for (-3 .. n + 2) because n >= 7.
__device__ inline int refl_sym(int i, int n) {
    if (i < 0) return -1 - i;
    if (i >= n) return 2 * n - 1 - i;
    return i;
}

constexpr int SPART = 3;   // per-tile partials of ssim_map_kernel: sum of S over the tile's cropped centres, per channel

// skimage's S over the WHOLE image and the per-tile sums behind mssim.  The tile, LDS layout, window loops and the order of every sum are
// pair_stats_kernel's, so the interior of the map and the mean are the numbers the ssim score is made of; the halo is resolved by
// refl_sym at load instead of being left out.  map [B,H,W,C]; part[(b * ntiles + tile) * SPART + c].
template <bool INT>
__global__ void __launch_bounds__(256) ssim_map_kernel(const void* a, int a_dt, const void* bimg, int b_dt, int H, int W, int C, const double* dr,
                                                       double* map, double* part) {
    using S = typename std::conditional<INT, int, float>::type;
    __shared__ S raw[2][3][MR * MR];
    __shared__ double red[256];
    const int b = blockIdx.z;
    const int y0 = blockIdx.y * MT, x0 = blockIdx.x * MT;
    const int tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    int dts[2];
    const void* img[2] = {image_of(a, a_dt, bimg, b_dt, 2 * b, HW * C, &dts[0]), image_of(a, a_dt, bimg, b_dt, 2 * b + 1, HW * C, &dts[1])};
    for (int i = tid; i < MR * MR * C; i += 256) {
        const int p = i / C, c = i - p * C;
        const int r = p / MR, cc = p - r * MR;
        const int y = y0 - MHW + r, x = x0 - MHW + cc;
        const bool used = y < H + MHW && x < W + MHW;                   // beyond the reach of the image's last row / column: never read
        const int64_t o = ((int64_t)refl_sym(y, H) * W + refl_sym(x, W)) * C + c;
        for (int k = 0; k < 2; ++k) raw[k][c][p] = used ? (S)ld_val(img[k], dts[k], o) : (S)0;
    }
    __syncthreads();

    const double R = dr[b];
    const double C1 = (0.01 * R) * (0.01 * R), C2 = (0.03 * R) * (0.03 * R);
    const double cov_norm = 49.0 / 48.0;
    double acc[SPART] = {0, 0, 0};
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, r = p >> 5, cc = p & 31;
        const int y = y0 + r, x = x0 + cc;
        if (y >= H || x >= W) continue;
        const bool centre = y >= MHW && y < H - MHW && x >= MHW && x < W - MHW;
        for (int c = 0; c < C; ++c) {
            double ux, uy, uxx, uyy, uxy;
            if (INT) {
                int sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                for (int i = 0; i < 7; ++i)
                    for (int j = 0; j < 7; ++j) {
                        const int u = raw[0][c][(r + i) * MR + cc + j], v = raw[1][c][(r + i) * MR + cc + j];
                        sa += u; sb += v; saa += u * u; sbb += v * v; sab += u * v;
                    }
                ux = sa / 49.0; uy = sb / 49.0; uxx = saa / 49.0; uyy = sbb / 49.0; uxy = sab / 49.0;
            } else {
                double sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
                for (int i = 0; i < 7; ++i)
                    for (int j = 0; j < 7; ++j) {
                        const double u = raw[0][c][(r + i) * MR + cc + j], v = raw[1][c][(r + i) * MR + cc + j];
                        sa += u; sb += v; saa += u * u; sbb += v * v; sab += u * v;
                    }
                ux = sa / 49.0; uy = sb / 49.0; uxx = saa / 49.0; uyy = sbb / 49.0; uxy = sab / 49.0;
            }
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
            const double s = (A1 * A2) / (B1 * B2);
            map[(((int64_t)b * H + y) * W + x) * C + c] = s;
            if (centre) acc[c] += s;
        }
    }
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    double* out = part + ((int64_t)b * gridDim.x * gridDim.y + tile) * SPART;
    for (int k = 0; k < SPART; ++k) {
        const double s = block_sum(acc[k], red);
        if (tid == 0) out[k] = s;
    }
}

// mssim: the tiles' sums in one fixed order, then scores_finalize_kernel's expression; one workgroup per pair
__global__ void __launch_bounds__(256) ssim_mean_kernel(const double* part, int ntiles, int H, int W, int C, double* mean) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s[SPART];
    for (int k = 0; k < SPART; ++k) {
        double v = 0.0;
        for (int t = tid; t < ntiles; t += 256) v += part[((int64_t)b * ntiles + t) * SPART + k];
        s[k] = block_sum(v, red);
    }
    if (tid != 0) return;
    const double ncen = (double)(H - 2 * MHW) * (double)(W - 2 * MHW);
    mean[b] = C == 1 ? s[0] / ncen : ((s[0] / ncen + s[1] / ncen) + s[2] / ncen) / 3.0;
}

}  // namespace

extern "C" {

int sr_rgb2gray_u8(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, uint8_t* y_u8, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!x_u8 || !y_u8) return ctx->fail(SR_ERR_INVALID, "rgb2gray_u8: null tensor");
    if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W >= ((int64_t)1 << 40)) return ctx->fail(SR_ERR_INVALID, "rgb2gray_u8: empty or oversized batch");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t npix = (int64_t)B * H * W;
    const bool vec = ((reinterpret_cast<uintptr_t>(x_u8) | reinterpret_cast<uintptr_t>(y_u8)) & 3) == 0;
    const int rec = ctx->prof_open("rgb2gray_u8", 0.0, (double)npix * 4.0, st);
    if (vec)
        hipLaunchKernelGGL(rgb2gray_kernel<true>, dim3(met_grid((npix + 3) / 4)), dim3(256), 0, st, x_u8, y_u8, npix);
    else
        hipLaunchKernelGGL(rgb2gray_kernel<false>, dim3(met_grid((npix + 3) / 4)), dim3(256), 0, st, x_u8, y_u8, npix);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_freq_to_u8(sr_ctx* ctx, const double* f_f64, int B, int H, int W, uint8_t* y_u8, double* max_f64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!f_f64 || !y_u8 || !max_f64) return ctx->fail(SR_ERR_INVALID, "freq_to_u8: null tensor");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)B * H * W >= ((int64_t)1 << 40)) return ctx->fail(SR_ERR_INVALID, "freq_to_u8: empty or oversized batch (1 <= B <= 65535)");
    const int64_t per = (int64_t)H * W;
    if (per > (int64_t)FQ_PER_WG * 65535) return ctx->fail(SR_ERR_INVALID, "freq_to_u8: images above 2^28 pixels are not supported");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned nchunk = (unsigned)((per + FQ_PER_WG - 1) / FQ_PER_WG);
    double* pmax = static_cast<double*>(ctx->arena(ctx->met_work, sizeof(double) * (size_t)B * nchunk, st));
    if (!pmax) return SR_ERR_OOM;
    const int rec = ctx->prof_open("freq_to_u8", 0.0, (double)B * per * (8.0 + 8.0 + 1.0), st);      // f read by both kernels, y written once
    hipLaunchKernelGGL(freq_chunk_max_kernel, dim3(nchunk, B), dim3(256), 0, st, f_f64, per, pmax);
    hipLaunchKernelGGL(freq_to_u8_kernel, dim3(nchunk, B), dim3(256), 0, st, f_f64, per, pmax, y_u8, max_f64);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_ssim_map(sr_ctx* ctx, const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int C, const double* data_range_f64,
                double* map_f64, double* mean_f64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!a || !b || !data_range_f64 || !map_f64 || !mean_f64) return ctx->fail(SR_ERR_INVALID, "ssim_map: null tensor");
    if ((a_dtype != SR_DTYPE_U8 && a_dtype != SR_DTYPE_F32) || (b_dtype != SR_DTYPE_U8 && b_dtype != SR_DTYPE_F32))
        return ctx->fail(SR_ERR_INVALID, "ssim_map: images must be uint8 or float32");
    if (C != 1 && C != 3) return ctx->fail(SR_ERR_INVALID, "ssim_map: C must be 1 (gray) or 3 (RGB)");
    if (B < 1 || B > 65535 || (int64_t)B * H * W * C >= ((int64_t)1 << 40)) return ctx->fail(SR_ERR_INVALID, "ssim_map: empty or oversized batch (1 <= B <= 65535)");
    if (H < 7 || W < 7) return ctx->fail(SR_ERR_INVALID, "ssim_map: H and W must be at least 7 (the SSIM window)");
    if ((int64_t)H * W > (int64_t)65535 * 4096) return ctx->fail(SR_ERR_INVALID, "ssim_map: images above 2^28 pixels are not supported");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 tgrid((W + MT - 1) / MT, (H + MT - 1) / MT, B);
    const int ntiles = (int)(tgrid.x * tgrid.y);
    double* part = static_cast<double*>(ctx->arena(ctx->met_work, sizeof(double) * (size_t)B * ntiles * SPART, st));
    if (!part) return SR_ERR_OOM;
    const int rec = ctx->prof_open("ssim_map", 0.0, (double)B * H * W * C * ((a_dtype == SR_DTYPE_U8 ? 1 : 4) + (b_dtype == SR_DTYPE_U8 ? 1 : 4) + 8.0), st);
    if (a_dtype == SR_DTYPE_U8 && b_dtype == SR_DTYPE_U8)
        hipLaunchKernelGGL(ssim_map_kernel<true>, tgrid, dim3(256), 0, st, a, a_dtype, b, b_dtype, H, W, C, data_range_f64, map_f64, part);
    else
        hipLaunchKernelGGL(ssim_map_kernel<false>, tgrid, dim3(256), 0, st, a, a_dtype, b, b_dtype, H, W, C, data_range_f64, map_f64, part);
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(B), dim3(256), 0, st, part, ntiles, H, W, C, mean_f64);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_classic_scores(sr_ctx* ctx, const void* hr, int hr_dtype, const void* sr, int sr_dtype, int B, int H, int W, int C, const double* data_range_f64,
                      double hf_radius_frac, double* scores_f64, float* gray_f32, float* sobel_f32, int* hist_luma_i32, int* hist_color_i32, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!hr || !sr || !data_range_f64 || !scores_f64) return ctx->fail(SR_ERR_INVALID, "classic_scores: null tensor");
    if ((hr_dtype != SR_DTYPE_U8 && hr_dtype != SR_DTYPE_F32) || (sr_dtype != SR_DTYPE_U8 && sr_dtype != SR_DTYPE_F32))
        return ctx->fail(SR_ERR_INVALID, "classic_scores: images must be uint8 or float32");
    if (C != 1 && C != 3) return ctx->fail(SR_ERR_INVALID, "classic_scores: C must be 1 (gray) or 3 (RGB)");
    if (B < 1 || B > 65535 || (int64_t)B * H * W * C >= ((int64_t)1 << 40)) return ctx->fail(SR_ERR_INVALID, "classic_scores: empty or oversized batch (1 <= B <= 65535)");
    if (H < 7 || W < 7) return ctx->fail(SR_ERR_INVALID, "classic_scores: H and W must be at least 7 (the SSIM window)");
    if ((int64_t)H * W > (int64_t)65535 * 4096) return ctx->fail(SR_ERR_INVALID, "classic_scores: images above 2^28 pixels are not supported");
    if (!std::isfinite(hf_radius_frac)) return ctx->fail(SR_ERR_INVALID, "classic_scores: hf_radius_frac must be finite");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int gray_ok = C == 1 || (hr_dtype == SR_DTYPE_U8 && sr_dtype == SR_DTYPE_U8);
    const int64_t HW = (int64_t)H * W;
    const dim3 tgrid((W + MT - 1) / MT, (H + MT - 1) / MT, B);
    const int ntiles = (int)(tgrid.x * tgrid.y);
    const dim3 fgrid((W + GT - 1) / GT, (H + GT - 1) / GT, 1);
    const int nhf = (int)(fgrid.x * fgrid.y);

    // work: flags [2B] int, partials [B][ntiles][NPART], hf partials [2B][nhf], histograms (when the caller passes none)
    const size_t b_flag = align256(sizeof(int) * 2 * (size_t)B), b_part = align256(sizeof(double) * (size_t)B * ntiles * NPART);
    const size_t b_hf = align256(sizeof(double) * 2 * (size_t)B * nhf);
    const size_t b_hl = align256(sizeof(int) * (size_t)B * 2 * LBINS), b_hc = align256(sizeof(int) * (size_t)B * 2 * 3 * CBINS);
    char* wk = static_cast<char*>(ctx->arena(ctx->met_work, b_flag + b_part + b_hf + b_hl + b_hc, st));
    if (!wk) return SR_ERR_OOM;
    int* flag = reinterpret_cast<int*>(wk);
    double* part = reinterpret_cast<double*>(wk + b_flag);
    double* hfp = reinterpret_cast<double*>(wk + b_flag + b_part);
    int* hl = hist_luma_i32 ? hist_luma_i32 : reinterpret_cast<int*>(wk + b_flag + b_part + b_hf);
    int* hc = hist_color_i32 ? hist_color_i32 : reinterpret_cast<int*>(wk + b_flag + b_part + b_hf + b_hl);
    SR_HIP(ctx, hipMemsetAsync(flag, 0, sizeof(int) * 2 * (size_t)B, st));
    if (gray_ok) SR_HIP(ctx, hipMemsetAsync(hl, 0, sizeof(int) * (size_t)B * 2 * LBINS, st));
    if (C == 3) SR_HIP(ctx, hipMemsetAsync(hc, 0, sizeof(int) * (size_t)B * 2 * 3 * CBINS, st));

    const int prec = ctx->prof_open("classic_scores_stats", 0.0, (double)B * HW * C * ((hr_dtype == SR_DTYPE_U8 ? 1 : 4) + (sr_dtype == SR_DTYPE_U8 ? 1 : 4)), st);
    if (gray_ok)
        hipLaunchKernelGGL(gray_scale_flag_kernel, dim3(2 * B, (unsigned)((HW + 4095) / 4096)), dim3(256), 0, st, hr, hr_dtype, sr, sr_dtype, C, HW, flag);
    if (hr_dtype == SR_DTYPE_U8 && sr_dtype == SR_DTYPE_U8)
        hipLaunchKernelGGL(pair_stats_kernel<true>, tgrid, dim3(256), 0, st, hr, hr_dtype, sr, sr_dtype, H, W, C, gray_ok, flag, data_range_f64, part, hl, hc,
                           gray_f32, sobel_f32);
    else
        hipLaunchKernelGGL(pair_stats_kernel<false>, tgrid, dim3(256), 0, st, hr, hr_dtype, sr, sr_dtype, H, W, C, gray_ok, flag, data_range_f64, part, hl, hc,
                           gray_f32, sobel_f32);
    ctx->prof_close(prec, st);
    SR_HIP(ctx, hipGetLastError());

    if (gray_ok) {
        const double *ahr, *ahi, *awr, *awi;
        if (int rc = dft_full_operator(ctx, H, st, &ahr, &ahi)) return rc;
        if (int rc = dft_full_operator(ctx, W, st, &awr, &awi)) return rc;
        const int nimg = 2 * B;
        const size_t per_img = sizeof(double) * (size_t)HW * 3;          // X, then T's real and imaginary parts
        const int chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((size_t)nimg, 32768), FFT_CHUNK_BYTES / per_img));   // grid z <= 65535
        double* xb = static_cast<double*>(ctx->arena(ctx->met_fft, per_img * (size_t)chunk, st));
        if (!xb) return SR_ERR_OOM;
        double* tr = xb + (int64_t)chunk * HW;
        double* ti = tr + (int64_t)chunk * HW;
        const int drec = ctx->prof_open("classic_scores_dft", (double)nimg * (4.0 * H * (double)W * W + 8.0 * (double)H * H * W),
                                        (double)nimg * HW * 8.0 * 5.0, st);      // the gray planes and the intermediates T, written and read once
        const int cy = H / 2, cx = W / 2;
        const double mask_r = hf_radius_frac * (sqrt((double)cy * cy + (double)cx * cx) + 1e-9);
        for (int g0 = 0; g0 < nimg; g0 += chunk) {
            const int n = std::min(chunk, nimg - g0);
            hipLaunchKernelGGL(gray_f64_kernel, dim3(met_grid((int64_t)n * HW)), dim3(256), 0, st, hr, hr_dtype, sr, sr_dtype, C, HW, g0, (int64_t)n, xb);
            // T = X . A_W^T  (M = H, N = W, K = W; B(k, j) = A_W[j][k])
            cgemm_dispatch<CG_STORE>(false, true, dim3(fgrid.x, fgrid.y, n), st, H, W, W, xb, nullptr, W, 1, HW, awr, awi, 1, W, 0, tr, ti, HW);
            // sum over the mask of |A_H . T|  (M = H, N = W, K = H), one partial per workgroup
            cgemm_dispatch<CG_MASKED_ABS_SUM>(true, true, dim3(fgrid.x, fgrid.y, n), st, H, W, H, ahr, ahi, H, 1, 0, tr, ti, W, 1, HW,
                                              hfp + (int64_t)g0 * nhf, nullptr, nhf, mask_r);
        }
        ctx->prof_close(drec, st);
    }
    hipLaunchKernelGGL(scores_finalize_kernel, dim3(B), dim3(256), 0, st, part, ntiles, hl, hc, hfp, nhf, data_range_f64, H, W, C, gray_ok, scores_f64);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
