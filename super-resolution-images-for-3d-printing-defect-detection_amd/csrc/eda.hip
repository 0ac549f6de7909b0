// eda.hip -- the per-pair image statistics and the global accumulators of the reference's exploratory data analysis (data/EDA.ipynb:
// ImageDatasetAnalyzer, cell 87582ba8, and MetricsAggregator.collect, cell eb5cc926), for B aligned pairs (lr, hr) of uint8 BGR images
// [H, W, 3].  The contract (gray, blurs, HSV, Canny, GLCM, moments, DCT) is stated once in include/sr355.h and restated in NumPy in
// tests/eda_ref.py.  Image g = 2 b + k, k = 0 for lr and 1 for hr, everywhere below.
//
//   1. planes pass (eda_planes_kernel): one 256-thread workgroup per 32 x 32 tile reads the BGR tile with a 2-pixel BORDER_REFLECT_101 halo
//      into LDS once and produces everything that is pointwise or a small stencil: gray, S, V, the 3 x 3 and 5 x 5 blurs, the Laplacian,
//      the 3 x 3 Sobel pair (one pair serves skimage's sobel and Canny: scipy 'reflect' and replicated borders agree at reach 1), Canny's
//      magnitude and non-maximum suppression (labels 0 none / 1 weak survivor / 2 strong), the channels' power sums.  Every sum but one
//      is an integer: wave reduction, LDS, then one 64-bit integer atomic per workgroup and quantity -> order-independent, exact.  The
//      Sobel-magnitude sum is fp64: one partial per tile, summed in a fixed order by the finalize kernel.
//   2. hysteresis (canny_hysteresis_kernel): one 1024-thread workgroup per image compacts the weak survivors into a list, then sweeps the
//      list ("weak with a strong 8-neighbour becomes strong") until a sweep changes nothing.  The label map stays in global memory (int per
//      pixel, L2-resident; a 478 x 478 map is 223 KB as bytes and does not fit a CU's 160 KB LDS), read and written with relaxed
//      agent-scope atomics so that a sweep sees the previous sweep's labels; the fixed point is unique, so the order within a sweep
//      does not matter.
//   3. ringing (eda_ring_kernel): 5 x 5 dilation of the edge map per tile, integer sums of gray over dilated-and-not-edge.
//   4. co-occurrence (glcm_count_kernel): integer atomics.  With 64 levels all four angles' matrices (64 KB) live in LDS per workgroup,
//      which counts a band of rows and then adds its non-zero cells to the image's global matrix; with 256 levels one angle alone is
//      256 KB, so the workgroups add straight into the image's global matrices (1 MB per image for four angles: L2-resident, no return
//      value needed, and natural images spread their pairs along the diagonal so that contention stays low).  glcm_props_kernel then
//      reduces each matrix to five integer sums and the |i - j| histogram, from which contrast, homogeneity and correlation follow in
//      fp64 (correlation as an exact integer ratio).
//   5. DCT: D = C_H X C_W^T by cgemm_f64.h's real fp64 GEMM, operators built on the device once per size; blocking sums in a fixed order.
//   6. finalize: one workgroup per pair; central moments and variances from the integer power sums in 128-bit integers, one division.
// The panel entry (sr_eda_pair_panels: create_advanced_visualizations and save_visual_example of cell 769cc582, per pair and unsummed) runs the
// accumulate entry's kernels with a store in place of the sum, plus one pixel kernel for the colour-noise map and the difference map.
// The accumulate entry adds |fftshift(fft2(gray))| (the DFT operators of metrics.hip), the 5-tap Sobel magnitude of hr, the normed
// 256-level co-occurrence matrix of lr and the saturation histograms into caller-owned buffers, pair after pair in batch order.
// No float atomics anywhere: a pair's row is the same bits on every run and for any B.
#include "cgemm_f64.h"
#include "common.h"
#include "fp_sep.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int ET = 32;                 // tile edge
constexpr int EHALO = 2;               // the 5 x 5 blur's reach; Canny's suppression reads the Sobel of the 1-pixel ring, which reads one more
constexpr int ER = ET + 2 * EHALO;     // 36
constexpr int EMG = ET + 2;            // magnitude region edge (34)
constexpr int MAX_DIM = 4096;
constexpr int64_t MAX_PIX = (int64_t)1 << 22;   // N^4 255^4 < 2^127: the fourth central moment's numerator fits __int128
constexpr size_t EDA_CHUNK_BYTES = (size_t)256 << 20;

// per-image integer accumulators
enum { A_SAT = 0, A_VAL, A_RMS, A_LAP1, A_LAP2, A_CN, A_POW, A_RING_N = A_POW + 12, A_RING_1, A_RING_2, NACC };

typedef unsigned long long u64;
typedef long long i64;
typedef __int128 i128;

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

inline unsigned grid1d(int64_t n) {
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

__device__ inline int r101(int i, int n) {
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

__device__ inline int clampi(int i, int lo, int hi) { return i < lo ? lo : (i > hi ? hi : i); }

// 8-bit COLOR_BGR2HSV's V and S: V = max, S = (diff * sdiv[V] + 2^11) >> 12, sdiv[v] = round(255 * 2^12 / v) (never a tie), sdiv[0] = 0
__device__ inline void hsv_sv(int b, int g, int r, int* s, int* v) {
    const int mx = max(b, max(g, r)), mn = min(b, min(g, r));
    const int sdiv = mx ? (2 * (255 << 12) + mx) / (2 * mx) : 0;
    *v = mx;
    *s = ((mx - mn) * sdiv + (1 << 11)) >> 12;
}

__device__ inline i64 wave_sum(i64 v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// adds each thread's vals[0 .. n) into acc[0 .. n): wave reduction, 64-bit LDS atomics, one global atomic per quantity (all integer)
template <int NV>
__device__ inline void block_accumulate(const i64 (&vals)[NV], u64* lacc, u64* acc) {
    for (int k = (int)threadIdx.x; k < NV; k += (int)blockDim.x) lacc[k] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const i64 s = wave_sum(vals[k]);
        if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&lacc[k], (u64)s);
    }
    __syncthreads();
    for (int k = (int)threadIdx.x; k < NV; k += (int)blockDim.x)
        if (lacc[k]) atomicAdd(&acc[k], lacc[k]);
}

__device__ inline double block_sum_f64(double v, double* red) {
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

// one channel's BGR tile [ER][ER] origin (y0 - EHALO, x0 - EHALO) with its BORDER_REFLECT_101 halo -> raw[c][ER * ER], all 256 threads
__device__ inline void load_bgr_tile(const uint8_t* img, int H, int W, int y0, int x0, uint8_t (*raw)[ER * ER]) {
    for (int i = (int)threadIdx.x; i < ER * ER * 3; i += 256) {                     // channel fastest: coalesced on interleaved BGR
        const int p = i / 3, c = i - p * 3;
        const int r = p / ER, cc = p - r * ER;
        // beyond one tile's reach past the last row / column nothing is used: keep the reflected index inside the image
        const int y = r101(min(y0 - EHALO + r, H + 1), H), x = r101(min(x0 - EHALO + cc, W + 1), W);
        raw[c][p] = img[((int64_t)y * W + x) * 3 + c];
    }
}

// the 5 x 5 binomial blur at the tile position rp5 points to (row pitch ER): the exact integer sum rounded half up once
__device__ inline int blur5_at(const uint8_t* rp5) {
    int t = 0;
    for (int dy = -2; dy <= 2; ++dy) {
        const uint8_t* row = rp5 + dy * ER;
        const int h = row[-2] + 4 * row[-1] + 6 * row[0] + 4 * row[1] + row[2];
        t += h * (dy == 0 ? 6 : (dy == -1 || dy == 1 ? 4 : 1));
    }
    return (t + 128) >> 8;
}

__device__ inline double i128_to_double(i128 v) {
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)(-v) : (unsigned __int128)v;
    const double d = (double)(u64)(u >> 64) * 18446744073709551616.0 + (double)(u64)u;       // both terms >= 0: no cancellation
    return neg ? -d : d;
}

// ------------------------------------------------------------------------------------------------
// 1. planes pass.  grid (tiles x, tiles y, 2 B).  gray [2B][H][W] and lab [2B][H][W] are always written; the other planes when not NULL.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eda_planes_kernel(const uint8_t* lr, const uint8_t* hr, int H, int W, u64* acc, double* sob_part, uint8_t* gray,
                                                         int* lab, uint8_t* sat_out, uint8_t* val_out, uint8_t* blur3_out, uint8_t* blur5_out) {
    __shared__ uint8_t raw[3][ER * ER];
    __shared__ uint8_t gry[ER * ER];
    __shared__ unsigned short mag[EMG * EMG];
    __shared__ u64 lacc[NACC];
    __shared__ double red[256];
    const int g = blockIdx.z, tid = threadIdx.x;
    const int y0 = blockIdx.y * ET, x0 = blockIdx.x * ET;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* img = ((g & 1) ? hr : lr) + (int64_t)(g >> 1) * HW * 3;

    load_bgr_tile(img, H, W, y0, x0, raw);
    __syncthreads();
    for (int i = tid; i < ER * ER; i += 256) gry[i] = (uint8_t)gray_bgr(raw[0][i], raw[1][i], raw[2][i]);
    __syncthreads();

    // gray with replicated borders at image position (y, x), |y - tile| within the halo: the clamped position lies inside the tile region
    auto gc = [&](int y, int x) { return (int)gry[(clampi(y, 0, H - 1) - y0 + EHALO) * ER + clampi(x, 0, W - 1) - x0 + EHALO]; };
    auto sobel = [&](int y, int x, int* dx, int* dy) {
        const int a = gc(y - 1, x - 1), b = gc(y - 1, x), c = gc(y - 1, x + 1), d = gc(y, x - 1), e = gc(y, x + 1), f = gc(y + 1, x - 1),
                  h = gc(y + 1, x), k = gc(y + 1, x + 1);
        *dx = (c + 2 * e + k) - (a + 2 * d + f);
        *dy = (f + 2 * h + k) - (a + 2 * b + c);
    };
    for (int i = tid; i < EMG * EMG; i += 256) {
        const int r = i / EMG, cc = i - r * EMG;
        const int y = y0 - 1 + r, x = x0 - 1 + cc;
        int m = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            int dx, dy;
            sobel(y, x, &dx, &dy);
            m = abs(dx) + abs(dy);
        }
        mag[i] = (unsigned short)m;
    }
    __syncthreads();

    i64 v[A_RING_N];
#pragma unroll
    for (int k = 0; k < A_RING_N; ++k) v[k] = 0;
    double sob = 0.0;
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, r = p >> 5, cc = p & 31;
        const int y = y0 + r, x = x0 + cc;
        if (y >= H || x >= W) continue;
        const int rp = (r + EHALO) * ER + cc + EHALO;
        const int64_t o = (int64_t)g * HW + (int64_t)y * W + x;
        const int gv = gry[rp];
        gray[o] = (uint8_t)gv;
        int s, vv;
        hsv_sv(raw[0][rp], raw[1][rp], raw[2][rp], &s, &vv);
        v[A_SAT] += s;
        v[A_VAL] += vv;
        if (sat_out) sat_out[o] = (uint8_t)s;
        if (val_out) val_out[o] = (uint8_t)vv;
        // 3 x 3 binomial blur and the Laplacian of gray (BORDER_REFLECT_101: the halo as loaded)
        const uint8_t* gp = &gry[rp];
        const int b3 = ((gp[-ER - 1] + 2 * gp[-ER] + gp[-ER + 1]) + 2 * (gp[-1] + 2 * gp[0] + gp[1]) + (gp[ER - 1] + 2 * gp[ER] + gp[ER + 1]) + 8) >> 4;
        const int d3 = gv - b3;
        v[A_RMS] += d3 * d3;
        if (blur3_out) blur3_out[o] = (uint8_t)b3;
        const int lap = gp[-ER] + gp[-1] + gp[1] + gp[ER] - 4 * gv;
        v[A_LAP1] += lap;
        v[A_LAP2] += lap * lap;
        // 5 x 5 binomial blur per channel, power sums
        for (int c = 0; c < 3; ++c) {
            const uint8_t* rp5 = &raw[c][rp];
            const int b5 = blur5_at(rp5);
            const i64 xv = rp5[0];
            v[A_CN] += abs((int)xv - b5);
            if (blur5_out) blur5_out[o * 3 + c] = (uint8_t)b5;
            v[A_POW + 4 * c + 0] += xv;
            v[A_POW + 4 * c + 1] += xv * xv;
            v[A_POW + 4 * c + 2] += xv * xv * xv;
            v[A_POW + 4 * c + 3] += xv * xv * xv * xv;
        }
        // Sobel pair: skimage's magnitude, then Canny's suppression
        int dx, dy;
        sobel(y, x, &dx, &dy);
        sob += sqrt((double)(dx * dx + dy * dy) * 0.5) / 1020.0;
        int label = 0;
        const unsigned short* mp = &mag[(r + 1) * EMG + cc + 1];
        const int m = mp[0];
        if (y > 0 && y < H - 1 && x > 0 && x < W - 1 && m > 100) {
            const int ax = abs(dx), ay = abs(dy) << 15;
            const int tg22x = ax * 13573;
            bool keep;
            if (ay < tg22x) keep = m > mp[-1] && m >= mp[1];
            else if (ay > tg22x + (ax << 16)) keep = m > mp[-EMG] && m >= mp[EMG];
            else {
                const int sg = (dx ^ dy) < 0 ? -1 : 1;
                keep = m > mp[-EMG - sg] && m > mp[EMG + sg];
            }
            if (keep) label = m > 200 ? 2 : 1;
        }
        lab[o] = label;
    }
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double ssum = block_sum_f64(sob, red);
    if (tid == 0) sob_part[(int64_t)g * gridDim.x * gridDim.y + tile] = ssum;
    block_accumulate(v, lacc, acc + (int64_t)g * NACC);
}

// ------------------------------------------------------------------------------------------------
// 2. hysteresis: grid 2 B, 1024 threads.  list [2B][H W] work.
// ------------------------------------------------------------------------------------------------
__device__ inline int lab_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(1024) canny_hysteresis_kernel(int* lab, int* list, int H, int W) {
    __shared__ int n_weak;
    const int64_t HW = (int64_t)H * W;
    int* L = lab + (int64_t)blockIdx.x * HW;
    int* wl = list + (int64_t)blockIdx.x * HW;
    if (threadIdx.x == 0) n_weak = 0;
    __syncthreads();
    for (int64_t p = threadIdx.x; p < HW; p += 1024)
        if (L[p] == 1) wl[atomicAdd(&n_weak, 1)] = (int)p;           // weak survivors are interior pixels: all eight neighbours exist
    __syncthreads();
    const int n = n_weak;
    int changed;
    do {
        changed = 0;
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int p = wl[i];
            if (p < 0) continue;
            const int* c = L + p;
            const bool hit = lab_load(c - W - 1) == 2 || lab_load(c - W) == 2 || lab_load(c - W + 1) == 2 || lab_load(c - 1) == 2 || lab_load(c + 1) == 2 ||
                             lab_load(c + W - 1) == 2 || lab_load(c + W) == 2 || lab_load(c + W + 1) == 2;
            if (hit) {
                __hip_atomic_store(L + p, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                wl[i] = -1;                                            // this thread's own slot: promoted, never looked at again
                changed = 1;
            }
        }
        changed = __syncthreads_or(changed);
    } while (changed);
}

// ------------------------------------------------------------------------------------------------
// 3. ringing region: dilate(E, 5 x 5) and not E.  grid (tiles x, tiles y, 2 B)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eda_ring_kernel(const int* lab, const uint8_t* gray, int H, int W, u64* acc, uint8_t* edges_out) {
    __shared__ uint8_t e[ER * ER];
    __shared__ u64 lacc[3];
    const int g = blockIdx.z, tid = threadIdx.x;
    const int y0 = blockIdx.y * ET, x0 = blockIdx.x * ET;
    const int64_t HW = (int64_t)H * W;
    const int* L = lab + (int64_t)g * HW;
    for (int i = tid; i < ER * ER; i += 256) {
        const int r = i / ER, cc = i - r * ER;
        const int y = y0 - EHALO + r, x = x0 - EHALO + cc;
        e[i] = (y >= 0 && y < H && x >= 0 && x < W && L[(int64_t)y * W + x] == 2) ? 1 : 0;      // outside the image: nothing to dilate from
    }
    __syncthreads();
    i64 v[3] = {0, 0, 0};
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, r = p >> 5, cc = p & 31;
        const int y = y0 + r, x = x0 + cc;
        if (y >= H || x >= W) continue;
        const int rp = (r + EHALO) * ER + cc + EHALO;
        const int64_t o = (int64_t)g * HW + (int64_t)y * W + x;
        if (edges_out) edges_out[o] = e[rp] ? 255 : 0;
        if (e[rp]) continue;
        int any = 0;
        for (int dy = -2; dy <= 2; ++dy)
            for (int dx = -2; dx <= 2; ++dx) any |= e[rp + dy * ER + dx];
        if (any) {
            const i64 gv = gray[o];
            v[0] += 1;
            v[1] += gv;
            v[2] += gv * gv;
        }
    }
    block_accumulate(v, lacc, acc + (int64_t)g * NACC + A_RING_N);
}

// ------------------------------------------------------------------------------------------------
// 4. co-occurrence counts of image `b * img_stride` of gray (lr: stride 2), before symmetrisation: out [B][nang][L][L] (zeroed before).
//    Pixel (r, c) pairs with (r + dr, c + dc), (dr, dc) = (0, 1), (1, 1), (1, 0), (1, -1) for the angles 0, 45, 90, 135 deg of `mask`.
//    levels 0: the gray values themselves (256 levels).  grid (bands, B); LDSM: the matrices of the band in LDS (nang L L <= 16384).
// ------------------------------------------------------------------------------------------------
__device__ inline int quantise(int gv, int levels) {
    return levels ? (int)mul_sep(__fdiv_rn((float)gv, 255.f), (float)(levels - 1)) : gv;
}

template <bool LDSM>
__global__ void __launch_bounds__(256) glcm_count_kernel(const uint8_t* gray, int img_stride, int H, int W, int levels, int mask, int* out) {
    __shared__ int m[LDSM ? 16384 : 1];
    const int L = levels ? levels : 256;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* G = gray + (int64_t)b * img_stride * HW;
    int nang = 0, dr[4], dc[4];
    const int odr[4] = {0, 1, 1, 1}, odc[4] = {1, 1, 0, -1};
    for (int a = 0; a < 4; ++a)
        if (mask >> a & 1) { dr[nang] = odr[a]; dc[nang] = odc[a]; ++nang; }
    const int LL = L * L;
    int* dst = out + (int64_t)b * nang * LL;
    if (LDSM) {
        for (int i = tid; i < nang * LL; i += 256) m[i] = 0;
        __syncthreads();
    }
    const int rows = (H + gridDim.x - 1) / gridDim.x;
    const int ra = blockIdx.x * rows, rb = min(H, ra + rows);
    for (int64_t p = (int64_t)ra * W + tid; p < (int64_t)rb * W; p += 256) {
        const int r = (int)(p / W), c = (int)(p - (int64_t)r * W);
        const int i = quantise(G[p], levels);
        for (int a = 0; a < nang; ++a) {
            const int r2 = r + dr[a], c2 = c + dc[a];
            if (r2 >= H || c2 < 0 || c2 >= W) continue;
            const int j = quantise(G[(int64_t)r2 * W + c2], levels);
            if (LDSM) atomicAdd(&m[a * LL + i * L + j], 1);
            else atomicAdd(&dst[a * LL + i * L + j], 1);
        }
    }
    if (LDSM) {
        __syncthreads();
        for (int i = tid; i < nang * LL; i += 256)
            if (m[i]) atomicAdd(&dst[i], m[i]);
    }
}

// graycoprops of the symmetric normed matrix P = (C + C^T) / T, T = 2 sum C, from one pass over C: grid (nang, B) -> props [B][nang][3]
//   contrast     sum (i - j)^2 P = sum (i - j)^2 C / sum C
//   homogeneity  sum P / (1 + (i - j)^2) = sum_d n_d / (1 + d^2) / sum C, n_d the count of cells with |i - j| = d (d ascending)
//   correlation  (sum i j P - mu^2) / var with mu = S1 / T, S1 = sum (i + j) C: (2 T sum ij C - S1^2) / (T sum (i^2 + j^2) C - S1^2), exact
//                integers; 1 where the variance is 0 (skimage's std < 1e-15 rule: a non-zero integer variance gives std >= 1 / T)
__global__ void __launch_bounds__(256) glcm_props_kernel(const int* counts, int L, double* props) {
    __shared__ int nd[256];
    __shared__ u64 lacc[5];
    const int a = blockIdx.x, b = blockIdx.y, nang = gridDim.x, tid = threadIdx.x;
    const int* C = counts + ((int64_t)b * nang + a) * L * L;
    nd[tid] = 0;
    __syncthreads();
    i64 v[5] = {0, 0, 0, 0, 0};                  // sum C, sum (i - j)^2 C, sum (i + j) C, sum (i^2 + j^2) C, sum i j C
    for (int q = tid; q < L * L; q += 256) {
        const i64 c = C[q];
        if (!c) continue;
        const int i = q / L, j = q - i * L, d = abs(i - j);
        v[0] += c;
        v[1] += c * d * d;
        v[2] += c * (i + j);
        v[3] += c * (i * i + j * j);
        v[4] += c * i * j;
        atomicAdd(&nd[d], (int)c);
    }
    __shared__ u64 tot[5];
    if (tid < 5) tot[tid] = 0;
    block_accumulate(v, lacc, tot);
    __syncthreads();
    if (tid != 0) return;
    const i64 n = (i64)tot[0], T = 2 * n;
    double hom = 0.0;
    for (int d = 0; d < L; ++d) hom += (double)nd[d] / (double)(1 + d * d);
    const i128 s1 = (i128)(i64)tot[2];
    const i128 var = (i128)T * (i64)tot[3] - s1 * s1, cov = (i128)(2 * T) * (i64)tot[4] - s1 * s1;
    double* o = props + ((int64_t)b * nang + a) * 3;
    o[0] = (double)(i64)tot[1] / (double)n;
    o[1] = hom / (double)n;
    o[2] = var == 0 ? 1.0 : i128_to_double(cov) / i128_to_double(var);
}

// ------------------------------------------------------------------------------------------------
// 5. DCT-II, orthonormal: C_N[k][x] = s_k cos(pi (2 x + 1) k / (2 N)), s_0 = sqrt(1 / N), s_k = sqrt(2 / N); the phase reduced in integers
// ------------------------------------------------------------------------------------------------
__global__ void dct_operator_kernel(int N, double* op) {
    const int64_t total = (int64_t)N * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = i / N, x = i - k * N;
        const int64_t m = ((2 * x + 1) * k) % (4 * (int64_t)N);
        op[i] = sqrt((k == 0 ? 1.0 : 2.0) / (double)N) * cospi((double)m / (double)(2 * (int64_t)N));
    }
}

int dct_operator(sr_ctx* ctx, int N, hipStream_t st, const double** op) {
    const int64_t key = -(((int64_t)1 << 32) + N);
    auto it = ctx->dft_ops.find(key);
    if (it == ctx->dft_ops.end()) {
        const int64_t nel = (int64_t)N * N;
        double* p = static_cast<double*>(ctx->dalloc(sizeof(double) * (size_t)nel));
        if (!p) return SR_ERR_OOM;
        hipLaunchKernelGGL(dct_operator_kernel, dim3(grid1d(nel)), dim3(256), 0, st, N, p);
        SR_HIP(ctx, hipGetLastError());
        SR_HIP(ctx, hipStreamSynchronize(st));      // once per size: later calls may come on other streams
        it = ctx->dft_ops.emplace(key, p).first;
    }
    *op = it->second;
    return SR_OK;
}

// fp64 planes of images g0 .. g0 + n - 1 of gray [2B][H W]
__global__ void gray_to_f64_kernel(const uint8_t* gray, int64_t off, int64_t n, double* X) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) X[i] = (double)gray[off + i];
}

// blk[g][0] = sum |D[7::8, :]|, blk[g][1] = sum |D[:, 7::8]|: one workgroup per image, each thread its cells in index order, then a fixed tree
__global__ void __launch_bounds__(256) dct_blocking_kernel(const double* D, int H, int W, double* blk) {
    __shared__ double red[256];
    const double* d = D + (int64_t)blockIdx.x * H * W;
    double sr = 0.0, sc = 0.0;
    for (int64_t q = threadIdx.x; q < (int64_t)H * W; q += 256) {
        const int i = (int)(q / W), j = (int)(q - (int64_t)i * W);
        const double a = fabs(d[q]);
        if ((i & 7) == 7) sr += a;
        if ((j & 7) == 7) sc += a;
    }
    const double a = block_sum_f64(sr, red), b = block_sum_f64(sc, red);
    if (threadIdx.x == 0) { blk[2 * blockIdx.x] = a; blk[2 * blockIdx.x + 1] = b; }
}

// ------------------------------------------------------------------------------------------------
// 6. finalize: grid B -> stats [B][SR_NUM_EDA_STATS]
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) eda_finalize_kernel(const u64* acc, const double* sob_part, int ntiles, const double* props, int nang, const double* blk,
                                                           const double* scores, int H, int W, double* stats) {
    __shared__ double red[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double sob[2];
    for (int k = 0; k < 2; ++k) {
        double v = 0.0;
        for (int t = tid; t < ntiles; t += 256) v += sob_part[(int64_t)(2 * b + k) * ntiles + t];
        sob[k] = block_sum_f64(v, red);
    }
    if (tid != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const i64 N = (i64)H * W;
    const double dn = (double)N;
    double* o = stats + (int64_t)b * SR_NUM_EDA_STATS;
    o[SR_EDA_PSNR] = scores[(int64_t)b * SR_NUM_SCORES + SR_SCORE_PSNR];
    o[SR_EDA_SSIM] = scores[(int64_t)b * SR_NUM_SCORES + SR_SCORE_SSIM];
    for (int q = 0; q < 3; ++q) {
        double s = 0.0;
        for (int a = 0; a < nang; ++a) s += props[((int64_t)b * nang + a) * 3 + q];
        o[SR_EDA_GLCM_CONTRAST + q] = s / (double)nang;
    }
    const int nr = H / 8, nc = W / 8;            // rows 7, 15, ... below H
    for (int k = 0; k < 2; ++k) {
        const i64* A = reinterpret_cast<const i64*>(acc) + (int64_t)(2 * b + k) * NACC;
        o[SR_EDA_RMS_NOISE_LR + k] = sqrt((double)A[A_RMS] / dn);
        const i128 lapn = (i128)N * A[A_LAP2] - (i128)A[A_LAP1] * A[A_LAP1];
        o[SR_EDA_LAP_VAR_LR + k] = i128_to_double(lapn) / (dn * dn);
        const double mr = nr ? blk[2 * (2 * b + k)] / ((double)nr * W) : nan, mc = nc ? blk[2 * (2 * b + k) + 1] / ((double)nc * H) : nan;
        o[SR_EDA_BLOCKING_LR + k] = (mr + mc) / 2.0;
        o[SR_EDA_COLOR_NOISE_LR + k] = (double)A[A_CN] / (3.0 * dn);
        const i64 rn = A[A_RING_N];
        const i128 rv = (i128)rn * A[A_RING_2] - (i128)A[A_RING_1] * A[A_RING_1];
        o[SR_EDA_RINGING_LR + k] = rn ? sqrt(i128_to_double(rv)) / (double)rn : 0.0;
        o[SR_EDA_SATURATION_MEAN_LR + k] = (double)A[A_SAT] / dn;
        o[SR_EDA_BRIGHTNESS_MEAN_LR + k] = (double)A[A_VAL] / dn;
        o[SR_EDA_SOBEL_MEAN_LR + k] = sob[k] / dn;
        for (int c = 0; c < 3; ++c) {
            const i128 s1 = A[A_POW + 4 * c], s2 = A[A_POW + 4 * c + 1], s3 = A[A_POW + 4 * c + 2], s4 = A[A_POW + 4 * c + 3], n = N;
            const i128 n2 = n * s2 - s1 * s1;
            const i128 n3 = n * n * s3 - 3 * n * s1 * s2 + 2 * s1 * s1 * s1;
            const i128 n4 = n * n * n * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 * s1 * s1 * s1;
            const double d2 = i128_to_double(n2);
            o[SR_EDA_CH0_SKEW_LR + 2 * c + k] = n2 == 0 ? nan : i128_to_double(n3) / (d2 * sqrt(d2));
            o[SR_EDA_CH0_KURT_LR + 2 * c + k] = n2 == 0 ? nan : i128_to_double(n4) / (d2 * d2) - 3.0;
            o[SR_EDA_CH0_MEAN_LR + 2 * c + k] = (double)A[A_POW + 4 * c] / dn;
            o[SR_EDA_CH0_STD_LR + 2 * c + k] = sqrt(d2) / dn;
        }
    }
    o[SR_EDA_EDGE_DIFF] = o[SR_EDA_SOBEL_MEAN_HR] - o[SR_EDA_SOBEL_MEAN_LR];
}

__global__ void fill_f64_kernel(double* p, int n, double v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ------------------------------------------------------------------------------------------------
// the accumulate entry's kernels
// ------------------------------------------------------------------------------------------------
// gray planes [2B][H W] and the saturation histograms.  NB 50: np.histogram(S, linspace(0, 256, 51)), bin = S * 25 / 128 (edges i * 5.12), all pairs
// into one sat_counts [2][50] (the accumulate entry); NB 256: the counts per value of S, pair b into sat_counts [b][2][256] (the panel entry; NULL:
// gray alone).  grid (chunks, 2 B)
template <int NB>
__global__ void __launch_bounds__(256) gray_sat_hist_kernel(const uint8_t* lr, const uint8_t* hr, int64_t HW, uint8_t* gray, u64* sat_counts) {
    __shared__ int h[NB];
    const int g = blockIdx.y, tid = threadIdx.x;
    const uint8_t* img = ((g & 1) ? hr : lr) + (int64_t)(g >> 1) * HW * 3;
    if (tid < NB) h[tid] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * 4096 + tid, e = min((int64_t)(blockIdx.x + 1) * 4096, HW); i < e; i += 256) {
        const int b = img[3 * i], gg = img[3 * i + 1], r = img[3 * i + 2];
        gray[(int64_t)g * HW + i] = (uint8_t)gray_bgr(b, gg, r);
        int s, v;
        hsv_sv(b, gg, r, &s, &v);
        atomicAdd(&h[NB == 256 ? s : s * 25 / 128], 1);
    }
    __syncthreads();
    if (!sat_counts) return;
    u64* dst = sat_counts + (NB == 256 ? (int64_t)(g >> 1) * 2 * NB : 0) + (g & 1) * NB;
    if (tid < NB && h[tid]) atomicAdd(&dst[tid], (u64)h[tid]);
}

// hypot of the ksize-5 Sobel pair (1 4 6 4 1 x -1 -2 0 2 1, BORDER_REFLECT_101) of each hr gray image.  STORE false: grad [H][W] += it, in batch
// order; STORE true: grad [B][H][W] = it, pair by pair (the panel entry).  The same expression either way, and 0.0 + v is v: a zeroed sum of one
// pair holds the stored bits.
template <bool STORE>
__global__ void __launch_bounds__(256) grad5_kernel(const uint8_t* gray, int B, int H, int W, double* grad) {
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    int ys[5], xs[5];
    for (int t = 0; t < 5; ++t) { ys[t] = r101(y + t - 2, H); xs[t] = r101(x + t - 2, W); }
    const int sm[5] = {1, 4, 6, 4, 1}, df[5] = {-1, -2, 0, 2, 1};
    double s = STORE ? 0.0 : grad[p];
    for (int b = 0; b < B; ++b) {
        const uint8_t* G = gray + (int64_t)(2 * b + 1) * HW;
        int gx = 0, gy = 0;
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 5; ++j) {
                const int v = G[(int64_t)ys[i] * W + xs[j]];
                gx += sm[i] * df[j] * v;
                gy += df[i] * sm[j] * v;
            }
        const double m = sqrt((double)((i64)gx * gx + (i64)gy * gy));
        if (STORE) grad[(int64_t)b * HW + p] = m;
        else s += m;
    }
    if (!STORE) grad[p] = s;
}

// (C_b + C_b^T) / T, T = 2 H (W - 1).  STORE false: glcm [256][256] += it, pair after pair; STORE true: glcm [B][256][256] = it (the panel entry)
template <bool STORE>
__global__ void __launch_bounds__(256) glcm_normed_kernel(const int* counts, int B, double T, double* glcm) {
    const int i = blockIdx.x, j = threadIdx.x;
    double s = STORE ? 0.0 : glcm[i * 256 + j];
    for (int b = 0; b < B; ++b) {
        const int* C = counts + (int64_t)b * 65536;
        const double v = (double)(C[i * 256 + j] + C[j * 256 + i]) / T;
        if (STORE) glcm[(int64_t)b * 65536 + i * 256 + j] = v;
        else s += v;
    }
    if (!STORE) glcm[i * 256 + j] = s;
}

// fftshift(|F|) of images g0 .. g0 + n - 1 (absf [n][H][W]); image g0 + i is pair (g0 + i) >> 1's lr (even) or hr (odd), and a chunk may begin or
// end between the two.  STORE false: out_{lr,hr} [H][W] += it, in image order; STORE true: out_{lr,hr} [B][H][W] = it, a NULL side skipped (the
// panel entry).
template <bool STORE>
__global__ void __launch_bounds__(256) fft_shift_kernel(const double* absf, int g0, int n, int H, int W, double* out_lr, double* out_hr) {
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int64_t src = (int64_t)((y + (H + 1) / 2) % H) * W + (x + (W + 1) / 2) % W;
    if (STORE) {
        for (int i = 0; i < n; ++i) {
            double* o = ((g0 + i) & 1) ? out_hr : out_lr;
            if (o) o[(int64_t)((g0 + i) >> 1) * HW + p] = absf[(int64_t)i * HW + src];
        }
        return;
    }
    double s[2] = {out_lr[p], out_hr[p]};
    for (int i = 0; i < n; ++i) s[(g0 + i) & 1] += absf[(int64_t)i * HW + src];
    out_lr[p] = s[0];
    out_hr[p] = s[1];
}

// ------------------------------------------------------------------------------------------------
// the panel entry's own kernels
// ------------------------------------------------------------------------------------------------
// per pixel of pair b: noise [B][H][W] = (sum over B, G, R of |lr - blur5(lr)|) / 3.0 (the planes pass's blur; NULL: not stored), its integer sum
// over the image into cn_acc [B] (one integer atomic per workgroup: exact, order-independent), diff [B][H][W] = the 14-bit gray of |lr - hr| per
// channel (NULL: not computed).  grid (tiles x, tiles y, B)
__global__ void __launch_bounds__(256) eda_panel_pixel_kernel(const uint8_t* lr, const uint8_t* hr, int H, int W, double* noise, u64* cn_acc, uint8_t* diff) {
    __shared__ uint8_t raw[3][ER * ER];
    __shared__ u64 lacc[1];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int y0 = blockIdx.y * ET, x0 = blockIdx.x * ET;
    const int64_t HW = (int64_t)H * W;
    load_bgr_tile(lr + (int64_t)b * HW * 3, H, W, y0, x0, raw);
    __syncthreads();
    i64 v[1] = {0};
    for (int q = 0; q < 4; ++q) {
        const int p = tid + 256 * q, r = p >> 5, cc = p & 31;
        const int y = y0 + r, x = x0 + cc;
        if (y >= H || x >= W) continue;
        const int rp = (r + EHALO) * ER + cc + EHALO;
        const int64_t o = (int64_t)b * HW + (int64_t)y * W + x;
        int cn = 0, ad[3];
        for (int c = 0; c < 3; ++c) {
            const uint8_t* rp5 = &raw[c][rp];
            cn += abs((int)rp5[0] - blur5_at(rp5));
            if (diff) ad[c] = abs((int)rp5[0] - (int)hr[o * 3 + c]);
        }
        v[0] += cn;
        if (noise) noise[o] = (double)cn / 3.0;
        if (diff) diff[o] = (uint8_t)gray_bgr(ad[0], ad[1], ad[2]);
    }
    block_accumulate(v, lacc, cn_acc + b);
}

// scalars [B][SR_NUM_EDA_PANEL_SCALARS]: the expressions eda_finalize_kernel forms for glcm_contrast (one angle: (0.0 + c) / 1.0 is c) and color_noise_lr
__global__ void eda_panel_scalars_kernel(const double* props, const u64* cn_acc, int B, int H, int W, double* scalars) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double dn = (double)((i64)H * W);
    scalars[(int64_t)b * SR_NUM_EDA_PANEL_SCALARS + SR_EDA_PANEL_GLCM_CONTRAST] = props[(int64_t)b * 3];
    scalars[(int64_t)b * SR_NUM_EDA_PANEL_SCALARS + SR_EDA_PANEL_NOISE_MEAN] = (double)(i64)cn_acc[b] / (3.0 * dn);
}

// |fftshift(fft2(gray))| of images 0 .. nimg - 1 of gray [nimg][H W] (lr and hr interleaved) by the DFT operators of metrics.hip, in chunks of
// images: summed into out_{lr,hr} [H][W] (STORE false) or stored per pair (STORE true).  A chunk counts images, so it may end inside a pair.
template <bool STORE>
int dft_magnitudes(sr_ctx* ctx, const uint8_t* gray, int nimg, int H, int W, double* out_lr, double* out_hr, hipStream_t st) {
    const int64_t HW = (int64_t)H * W;
    const double *ahr, *ahi, *awr, *awi;
    if (int rc = dft_full_operator(ctx, H, st, &ahr, &ahi)) return rc;
    if (int rc = dft_full_operator(ctx, W, st, &awr, &awi)) return rc;
    const size_t per_img = sizeof(double) * (size_t)HW * 4;          // X, T's real and imaginary parts, |F|
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nimg, EDA_CHUNK_BYTES / per_img));
    double* xb = static_cast<double*>(ctx->arena(ctx->eda_dct, per_img * (size_t)chunk, st));
    if (!xb) return SR_ERR_OOM;
    double* tr = xb + (int64_t)chunk * HW;
    double* ti = tr + (int64_t)chunk * HW;
    double* fa = ti + (int64_t)chunk * HW;
    const dim3 fgrid((W + GT - 1) / GT, (H + GT - 1) / GT, 1);
    for (int g0 = 0; g0 < nimg; g0 += chunk) {
        const int n = std::min(chunk, nimg - g0);
        hipLaunchKernelGGL(gray_to_f64_kernel, dim3(grid1d((int64_t)n * HW)), dim3(256), 0, st, gray, (int64_t)g0 * HW, (int64_t)n * HW, xb);
        cgemm_dispatch<CG_STORE>(false, true, dim3(fgrid.x, fgrid.y, n), st, H, W, W, xb, nullptr, W, 1, HW, awr, awi, 1, W, 0, tr, ti, HW);
        cgemm_dispatch<CG_ABS>(true, true, dim3(fgrid.x, fgrid.y, n), st, H, W, H, ahr, ahi, H, 1, 0, tr, ti, W, 1, HW, fa, nullptr, HW);
        hipLaunchKernelGGL(fft_shift_kernel<STORE>, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, fa, g0, n, H, W, out_lr, out_hr);
    }
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int check_shape(sr_ctx* ctx, const char* who, int B, int H, int W) {
    if (B < 1 || B > 32767) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": empty or oversized batch (1 <= B <= 32767)");
    if (H < 7 || W < 7) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": H and W must be at least 7 (the SSIM window)");
    if (H > MAX_DIM || W > MAX_DIM || (int64_t)H * W > MAX_PIX)
        return ctx->fail(SR_ERR_INVALID, std::string(who) + ": images above 4096 pixels a side or 2^22 pixels are not supported (the DCT / DFT operators and the "
                                                             "128-bit moment sums are sized for that)");
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_eda_pair_stats(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, int glcm_levels, int angle_mask, double* stats_f64,
                      uint8_t* gray_u8, uint8_t* sat_u8, uint8_t* val_u8, uint8_t* blur3_u8, uint8_t* blur5_u8, uint8_t* edges_u8, int* glcm_i32,
                      double* dct_f64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!lr_u8 || !hr_u8 || !stats_f64) return ctx->fail(SR_ERR_INVALID, "eda_pair_stats: null tensor");
    if (int rc = check_shape(ctx, "eda_pair_stats", B, H, W)) return rc;
    if (glcm_levels != 64 && glcm_levels != 256) return ctx->fail(SR_ERR_INVALID, "eda_pair_stats: glcm_levels must be 64 or 256");
    if (angle_mask < 1 || angle_mask > 15) return ctx->fail(SR_ERR_INVALID, "eda_pair_stats: angle_mask must name at least one of the four angles (bits 0..3)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int nimg = 2 * B, L = glcm_levels, nang = __builtin_popcount((unsigned)angle_mask);
    const dim3 tgrid((W + ET - 1) / ET, (H + ET - 1) / ET, nimg);
    const int ntiles = (int)(tgrid.x * tgrid.y);

    const size_t b_acc = al256(sizeof(u64) * (size_t)nimg * NACC), b_sob = al256(sizeof(double) * (size_t)nimg * ntiles), b_props = al256(sizeof(double) * B * 12);
    const size_t b_blk = al256(sizeof(double) * 2 * (size_t)nimg), b_sc = al256(sizeof(double) * (size_t)B * SR_NUM_SCORES), b_dr = al256(sizeof(double) * (size_t)B);
    const size_t b_gray = gray_u8 ? 0 : al256((size_t)nimg * HW), b_lab = al256(sizeof(int) * (size_t)nimg * HW);
    const size_t b_glcm = glcm_i32 ? 0 : al256(sizeof(int) * (size_t)B * nang * L * L);
    char* wk = static_cast<char*>(ctx->arena(ctx->eda_work, b_acc + b_sob + b_props + b_blk + b_sc + b_dr + b_gray + 2 * b_lab + b_glcm, st));
    if (!wk) return SR_ERR_OOM;
    u64* acc = reinterpret_cast<u64*>(wk); wk += b_acc;
    double* sob = reinterpret_cast<double*>(wk); wk += b_sob;
    double* props = reinterpret_cast<double*>(wk); wk += b_props;
    double* blk = reinterpret_cast<double*>(wk); wk += b_blk;
    double* scores = reinterpret_cast<double*>(wk); wk += b_sc;
    double* dr = reinterpret_cast<double*>(wk); wk += b_dr;
    uint8_t* gray = gray_u8 ? gray_u8 : reinterpret_cast<uint8_t*>(wk); wk += b_gray;
    int* lab = reinterpret_cast<int*>(wk); wk += b_lab;
    int* list = reinterpret_cast<int*>(wk); wk += b_lab;
    int* glcm = glcm_i32 ? glcm_i32 : reinterpret_cast<int*>(wk);

    // psnr, ssim: sr_classic_scores' columns (channel order changes neither), hr first as the notebook passes them
    hipLaunchKernelGGL(fill_f64_kernel, dim3((B + 255) / 256), dim3(256), 0, st, dr, B, 255.0);
    if (int rc = sr_classic_scores(ctx, hr_u8, SR_DTYPE_U8, lr_u8, SR_DTYPE_U8, B, H, W, 3, dr, 0.6, scores, nullptr, nullptr, nullptr, nullptr, stream)) return rc;

    SR_HIP(ctx, hipMemsetAsync(acc, 0, sizeof(u64) * (size_t)nimg * NACC, st));
    SR_HIP(ctx, hipMemsetAsync(glcm, 0, sizeof(int) * (size_t)B * nang * L * L, st));
    int rec = ctx->prof_open("eda_planes", 0.0, (double)nimg * HW * 3.0, st);
    hipLaunchKernelGGL(eda_planes_kernel, tgrid, dim3(256), 0, st, lr_u8, hr_u8, H, W, acc, sob, gray, lab, sat_u8, val_u8, blur3_u8, blur5_u8);
    ctx->prof_close(rec, st);
    rec = ctx->prof_open("eda_canny_hysteresis", 0.0, 0.0, st);
    hipLaunchKernelGGL(canny_hysteresis_kernel, dim3(nimg), dim3(1024), 0, st, lab, list, H, W);
    ctx->prof_close(rec, st);
    hipLaunchKernelGGL(eda_ring_kernel, tgrid, dim3(256), 0, st, lab, gray, H, W, acc, edges_u8);
    rec = ctx->prof_open("eda_glcm", 0.0, 0.0, st);
    const dim3 ggrid((unsigned)std::min(16, (H + 31) / 32), B);
    if (nang * L * L <= 16384) hipLaunchKernelGGL(glcm_count_kernel<true>, ggrid, dim3(256), 0, st, gray, 2, H, W, L, angle_mask, glcm);
    else hipLaunchKernelGGL(glcm_count_kernel<false>, ggrid, dim3(256), 0, st, gray, 2, H, W, L, angle_mask, glcm);
    hipLaunchKernelGGL(glcm_props_kernel, dim3(nang, B), dim3(256), 0, st, glcm, L, props);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());

    // D = C_H X C_W^T in chunks of images
    const double *ch, *cw;
    if (int rc = dct_operator(ctx, H, st, &ch)) return rc;
    if (int rc = dct_operator(ctx, W, st, &cw)) return rc;
    const size_t per_img = sizeof(double) * (size_t)HW * (dct_f64 ? 2 : 3);           // X, T and D (D in the caller's buffer when given)
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)nimg, EDA_CHUNK_BYTES / per_img));
    double* xb = static_cast<double*>(ctx->arena(ctx->eda_dct, per_img * (size_t)chunk, st));
    if (!xb) return SR_ERR_OOM;
    double* tb = xb + (int64_t)chunk * HW;
    rec = ctx->prof_open("eda_dct", (double)nimg * (2.0 * H * (double)W * W + 2.0 * (double)H * H * W), (double)nimg * HW * 8.0 * 5.0, st);
    const dim3 fgrid((W + GT - 1) / GT, (H + GT - 1) / GT, 1);
    for (int g0 = 0; g0 < nimg; g0 += chunk) {
        const int n = std::min(chunk, nimg - g0);
        double* db = dct_f64 ? dct_f64 + (int64_t)g0 * HW : tb + (int64_t)chunk * HW;
        hipLaunchKernelGGL(gray_to_f64_kernel, dim3(grid1d((int64_t)n * HW)), dim3(256), 0, st, gray, (int64_t)g0 * HW, (int64_t)n * HW, xb);
        // T = X . C_W^T  (M = H, N = W, K = W; B(k, j) = C_W[j][k])
        cgemm_dispatch<CG_STORE>(false, false, dim3(fgrid.x, fgrid.y, n), st, H, W, W, xb, nullptr, W, 1, HW, cw, nullptr, 1, W, 0, tb, nullptr, HW);
        // D = C_H . T  (M = H, N = W, K = H)
        cgemm_dispatch<CG_STORE>(false, false, dim3(fgrid.x, fgrid.y, n), st, H, W, H, ch, nullptr, H, 1, 0, tb, nullptr, W, 1, HW, db, nullptr, HW);
        hipLaunchKernelGGL(dct_blocking_kernel, dim3(n), dim3(256), 0, st, db, H, W, blk + 2 * (int64_t)g0);
    }
    ctx->prof_close(rec, st);
    hipLaunchKernelGGL(eda_finalize_kernel, dim3(B), dim3(256), 0, st, acc, sob, ntiles, props, nang, blk, scores, H, W, stats_f64);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_eda_accumulate(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, double* fft_lr_sum_f64, double* fft_hr_sum_f64,
                      double* grad_hr_sum_f64, double* glcm_sum_f64, int64_t* sat_counts_i64, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!lr_u8 || !hr_u8 || !fft_lr_sum_f64 || !fft_hr_sum_f64 || !grad_hr_sum_f64 || !glcm_sum_f64 || !sat_counts_i64)
        return ctx->fail(SR_ERR_INVALID, "eda_accumulate: null tensor");
    if (int rc = check_shape(ctx, "eda_accumulate", B, H, W)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int nimg = 2 * B;
    const size_t b_gray = al256((size_t)nimg * HW), b_glcm = al256(sizeof(int) * (size_t)B * 65536);
    char* wk = static_cast<char*>(ctx->arena(ctx->eda_work, b_gray + b_glcm, st));
    if (!wk) return SR_ERR_OOM;
    uint8_t* gray = reinterpret_cast<uint8_t*>(wk);
    int* glcm = reinterpret_cast<int*>(wk + b_gray);

    hipLaunchKernelGGL(gray_sat_hist_kernel<50>, dim3((unsigned)((HW + 4095) / 4096), nimg), dim3(256), 0, st, lr_u8, hr_u8, HW, gray,
                       reinterpret_cast<u64*>(sat_counts_i64));
    hipLaunchKernelGGL(grad5_kernel<false>, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, gray, B, H, W, grad_hr_sum_f64);
    SR_HIP(ctx, hipMemsetAsync(glcm, 0, sizeof(int) * (size_t)B * 65536, st));
    hipLaunchKernelGGL(glcm_count_kernel<false>, dim3((unsigned)std::min(16, (H + 31) / 32), B), dim3(256), 0, st, gray, 2, H, W, 0, 1, glcm);
    hipLaunchKernelGGL(glcm_normed_kernel<false>, dim3(256), dim3(256), 0, st, glcm, B, 2.0 * (double)H * (double)(W - 1), glcm_sum_f64);
    SR_HIP(ctx, hipGetLastError());

    return dft_magnitudes<false>(ctx, gray, nimg, H, W, fft_lr_sum_f64, fft_hr_sum_f64, st);
}

int sr_eda_pair_panels(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, double* spec_lr_f64, double* spec_hr_f64,
                       double* grad_hr_f64, double* glcm_lr_f64, double* noise_lr_f64, uint8_t* diff_u8, int64_t* sat_hist_i64, double* scalars_f64,
                       void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!lr_u8 || !hr_u8) return ctx->fail(SR_ERR_INVALID, "eda_pair_panels: null tensor");
    if (int rc = check_shape(ctx, "eda_pair_panels", B, H, W)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t HW = (int64_t)H * W;
    const int nimg = 2 * B;
    const bool want_spec = spec_lr_f64 || spec_hr_f64, want_glcm = glcm_lr_f64 || scalars_f64;
    const bool want_gray = want_spec || grad_hr_f64 || want_glcm || sat_hist_i64;
    const size_t b_gray = want_gray ? al256((size_t)nimg * HW) : 0, b_glcm = want_glcm ? al256(sizeof(int) * (size_t)B * 65536) : 0;
    const size_t b_props = al256(sizeof(double) * (size_t)B * 3), b_cn = al256(sizeof(u64) * (size_t)B);
    char* wk = static_cast<char*>(ctx->arena(ctx->eda_work, b_gray + b_glcm + b_props + b_cn, st));
    if (!wk) return SR_ERR_OOM;
    uint8_t* gray = reinterpret_cast<uint8_t*>(wk); wk += b_gray;
    int* glcm = reinterpret_cast<int*>(wk); wk += b_glcm;
    double* props = reinterpret_cast<double*>(wk); wk += b_props;
    u64* cn = reinterpret_cast<u64*>(wk);

    int rec = ctx->prof_open("eda_panel_planes", 0.0, (double)nimg * HW * 3.0, st);
    if (want_gray) {
        if (sat_hist_i64) SR_HIP(ctx, hipMemsetAsync(sat_hist_i64, 0, sizeof(int64_t) * (size_t)B * 512, st));
        hipLaunchKernelGGL(gray_sat_hist_kernel<256>, dim3((unsigned)((HW + 4095) / 4096), nimg), dim3(256), 0, st, lr_u8, hr_u8, HW, gray,
                           reinterpret_cast<u64*>(sat_hist_i64));
    }
    if (noise_lr_f64 || diff_u8 || scalars_f64) {
        SR_HIP(ctx, hipMemsetAsync(cn, 0, sizeof(u64) * (size_t)B, st));
        hipLaunchKernelGGL(eda_panel_pixel_kernel, dim3((W + ET - 1) / ET, (H + ET - 1) / ET, B), dim3(256), 0, st, lr_u8, hr_u8, H, W, noise_lr_f64, cn, diff_u8);
    }
    if (grad_hr_f64) hipLaunchKernelGGL(grad5_kernel<true>, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, st, gray, B, H, W, grad_hr_f64);
    ctx->prof_close(rec, st);
    if (want_glcm) {
        rec = ctx->prof_open("eda_panel_glcm", 0.0, 0.0, st);
        SR_HIP(ctx, hipMemsetAsync(glcm, 0, sizeof(int) * (size_t)B * 65536, st));
        hipLaunchKernelGGL(glcm_count_kernel<false>, dim3((unsigned)std::min(16, (H + 31) / 32), B), dim3(256), 0, st, gray, 2, H, W, 0, 1, glcm);
        if (glcm_lr_f64) hipLaunchKernelGGL(glcm_normed_kernel<true>, dim3(256), dim3(256), 0, st, glcm, B, 2.0 * (double)H * (double)(W - 1), glcm_lr_f64);
        if (scalars_f64) {
            // 256 levels quantise to themselves ((uint8)(float32(g) / 255 * 255) is g for every g), so these are sr_eda_pair_stats' counts
            hipLaunchKernelGGL(glcm_props_kernel, dim3(1, B), dim3(256), 0, st, glcm, 256, props);
            hipLaunchKernelGGL(eda_panel_scalars_kernel, dim3((B + 255) / 256), dim3(256), 0, st, props, cn, B, H, W, scalars_f64);
        }
        ctx->prof_close(rec, st);
    }
    SR_HIP(ctx, hipGetLastError());
    if (!want_spec) return SR_OK;

    rec = ctx->prof_open("eda_panel_dft", (double)nimg * 8.0 * (H * (double)W * W + (double)H * H * W), (double)nimg * HW * 8.0 * 7.0, st);
    const int rc = dft_magnitudes<true>(ctx, gray, nimg, H, W, spec_lr_f64, spec_hr_f64, st);
    ctx->prof_close(rec, st);
    return rc;
}

}  // extern "C"
