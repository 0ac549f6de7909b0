// degrade.hip -- the stages of the reference's dataset synthesis (data/common_methods.py::degrade_image) on B uint8 BGR images [H, W, 3] of
// one shape: Gaussian blur, horizontal motion blur, the noise stage and a baseline-JPEG round trip.  (The resize between them is sr_resize.)
// The contracts are stated once in include/sr355.h and restated in NumPy in tests/degrade_ref.py.  Per-image parameters come in a device
// int32 table [B][SR_DEG_PARAMS]; a stage whose flag is 0 in a row copies that image through.  All arithmetic is integer except the noise
// stage's one fp32 multiply and add, which are rounded separately; there is no reduction anywhere, so a result is the same bits on every run
// and for any B.
//
//   gauss   one 256-thread workgroup per 32 x 32 tile: the BGR tile with a 3-pixel BORDER_REFLECT_101 halo in LDS as bytes, the horizontal
//           pass into LDS as uint16 (at most 255 * 256), the vertical pass and the one rounding from there.  The taps are padded to 7
//           with zeros, so that the three kernel sizes share the code.
//   motion  a horizontal box: one thread per output byte, the row's neighbours from L1 / L2.
//   noise   one thread per four consecutive elements = one Philox4x32-10 block; Box-Muller in fp32 per pair of words.
//   jpeg    kernel 1: one wave per 16 x 16 MCU (four to a workgroup).  Colour conversion of the edge-replicated tile into LDS, h2v2
//           down-sampling, then the six 8 x 8 blocks' DCTs with one lane per block row / column: forward rows, a transpose through LDS,
//           forward columns + quantisation + dequantisation + inverse columns in registers (libjpeg's inverse starts with the columns, which
//           the lane already holds), a transpose, inverse rows + range limit -> planar Y and half-resolution Cb / Cr in global memory.
//           kernel 2: one thread per output pixel: triangle ("fancy") chroma up-sampling, which reads across MCU borders, and YCbCr -> BGR.
// A bad row (a kernel size, tap set, deviation or quality outside the contract) is never acted on: the image is copied through and the
// first such row is recorded in the context's status words, which sr_degrade_status reads back (the stage entries themselves only launch).
#include "common.h"
#include "fp_sep.h"

#include <algorithm>
#include <string>

namespace {

constexpr int DEG_MIN = 16, DEG_MAX = 4096;
constexpr int GT_ = 32, GR = 3, GE = GT_ + 2 * GR;          // gauss tile, halo, tile edge with halo (38)
enum { ST_GAUSS = 1, ST_MOTION, ST_NOISE, ST_JPEG };

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

__device__ inline int r101(int i, int n) {
    if (i < 0) return -i;
    if (i >= n) return 2 * n - 2 - i;
    return i;
}

__device__ inline void flag_bad_row(int* status, int stage, int row, int value) {
    if (atomicCAS(&status[0], 0, stage) == 0) { status[1] = row; status[2] = value; }
}

// ------------------------------------------------------------------------------------------------
// Gaussian blur.  grid (tiles x, tiles y, B)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) degrade_gauss_kernel(const uint8_t* x, int H, int W, const int* params, int* status, uint8_t* y) {
    __shared__ uint8_t raw[3][GE * GE];
    __shared__ unsigned short hp[3][GE * GT_];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int y0 = blockIdx.y * GT_, x0 = blockIdx.x * GT_;
    const int* row = params + (int64_t)b * SR_DEG_PARAMS;
    const uint8_t* img = x + (int64_t)b * H * W * 3;
    uint8_t* out = y + (int64_t)b * H * W * 3;
    int k = row[SR_DEG_GAUSS_KSIZE];
    int T[7] = {0, 0, 0, 0, 0, 0, 0};
    if (k != 0) {
        bool ok = k == 3 || k == 5 || k == 7;
        int sum = 0;
        if (ok)
            for (int i = 0; i < k; ++i) {
                const int t = row[SR_DEG_GAUSS_TAP0 + i];
                ok = ok && t >= 0 && t <= 256;
                sum += t;
                T[GR - k / 2 + i] = t;
            }
        if (!ok || sum != 256) {
            if (tid == 0 && blockIdx.x == 0 && blockIdx.y == 0) flag_bad_row(status, ST_GAUSS, b, k);
            k = 0;
        }
    }
    if (k == 0) {                                                        // copy through (uniform over the workgroup)
        for (int i = tid; i < GT_ * GT_ * 3; i += 256) {
            const int p = i / 3, c = i - p * 3, yy = y0 + p / GT_, xx = x0 + p % GT_;
            if (yy < H && xx < W) out[((int64_t)yy * W + xx) * 3 + c] = img[((int64_t)yy * W + xx) * 3 + c];
        }
        return;
    }
    for (int i = tid; i < GE * GE * 3; i += 256) {                       // channel fastest: coalesced on interleaved BGR
        const int p = i / 3, c = i - p * 3;
        const int r = p / GE, cc = p - r * GE;
        // past the image's last row / column + halo nothing is used: keep the reflected index inside the image (H, W >= 16 > halo)
        const int yy = r101(min(y0 - GR + r, H - 1 + GR), H), xx = r101(min(x0 - GR + cc, W - 1 + GR), W);
        raw[c][p] = img[((int64_t)yy * W + xx) * 3 + c];
    }
    __syncthreads();
    for (int i = tid; i < GE * GT_ * 3; i += 256) {
        const int c = i / (GE * GT_), p = i - c * (GE * GT_);
        const int r = p / GT_, cc = p - r * GT_;
        const uint8_t* s = &raw[c][r * GE + cc];
        int a = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) a += T[j] * s[j];
        hp[c][p] = (unsigned short)a;                                    // <= 255 * 256
    }
    __syncthreads();
    for (int i = tid; i < GT_ * GT_ * 3; i += 256) {
        const int p = i / 3, c = i - p * 3;
        const int r = p / GT_, cc = p - r * GT_;
        const int yy = y0 + r, xx = x0 + cc;
        if (yy >= H || xx >= W) continue;
        const unsigned short* s = &hp[c][r * GT_ + cc];
        int a = 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) a += T[j] * s[j * GT_];
        out[((int64_t)yy * W + xx) * 3 + c] = (uint8_t)((a + 32768) >> 16);
    }
}

// ------------------------------------------------------------------------------------------------
// motion blur: (2 sum + size) / (2 size) over `size` horizontal neighbours.  grid-stride over the B H W 3 bytes
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) degrade_motion_kernel(const uint8_t* x, int B, int H, int W, const int* params, int* status, uint8_t* y) {
    const int64_t per = (int64_t)H * W * 3, total = per * B;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int b = (int)(i / per);
        const int64_t e = i - (int64_t)b * per;
        int size = params[(int64_t)b * SR_DEG_PARAMS + SR_DEG_MOTION_SIZE];
        if (size != 0 && size != 5 && size != 7 && size != 9) {
            if (e == 0) flag_bad_row(status, ST_MOTION, b, size);
            size = 0;
        }
        if (size == 0) { y[i] = x[i]; continue; }
        const int64_t p = e / 3;
        const int c = (int)(e - p * 3), yy = (int)(p / W), xx = (int)(p - (int64_t)yy * W);
        const uint8_t* rowp = x + (int64_t)b * per + (int64_t)yy * W * 3 + c;
        const int r = size >> 1;
        int s = 0;
        for (int j = -r; j <= r; ++j) s += rowp[r101(xx + j, W) * 3];
        y[i] = (uint8_t)((2 * s + size) / (2 * size));
    }
}

// ------------------------------------------------------------------------------------------------
// noise.  grid (ceil(ceil(n / 4) / 256), B), n = H W 3
// ------------------------------------------------------------------------------------------------
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

__global__ void __launch_bounds__(256) degrade_noise_kernel(const uint8_t* x, int n, const int* params, const float* field, unsigned long long seed, int* status,
                                                            uint8_t* y, float* z_out) {
    const int b = blockIdx.y;
    const int64_t e0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (e0 >= n) return;
    const int cnt = (int)min((int64_t)4, (int64_t)n - e0);
    const int* row = params + (int64_t)b * SR_DEG_PARAMS;
    const uint8_t* in = x + (int64_t)b * n + e0;
    uint8_t* out = y + (int64_t)b * n + e0;
    int on = row[SR_DEG_NOISE_ON];
    const float sd = __int_as_float(row[SR_DEG_NOISE_STD]);
    if (on && !field && !(sd >= 0.f && sd <= 3.0e38f)) {                  // negative, infinite or NaN
        if (e0 == 0) flag_bad_row(status, ST_NOISE, b, row[SR_DEG_NOISE_STD]);
        on = 0;
    }
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (field) {
        for (int k = 0; k < cnt; ++k) nz[k] = field[(int64_t)b * n + e0 + k];
    } else if (on || z_out) {
        uint32_t w[4];
        philox4x32_10((uint32_t)(e0 >> 2), 0u, (uint32_t)b, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        float z[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float u1 = (float)((w[2 * h] >> 8) + 1u) * 0x1p-24f;    // (0, 1], exact
            const float u2 = (float)(w[2 * h + 1] >> 8) * 0x1p-24f;       // [0, 1), exact
            const float rad = sqrtf(-2.f * logf(u1));
            float sn, cs;
            sincospif(2.f * u2, &sn, &cs);
            z[2 * h] = rad * cs;
            z[2 * h + 1] = rad * sn;
        }
        for (int k = 0; k < cnt; ++k) {
            if (z_out) z_out[(int64_t)b * n + e0 + k] = z[k];
            nz[k] = mul_sep(sd, z[k]);
        }
    }
    for (int k = 0; k < cnt; ++k) {
        if (!on) { out[k] = in[k]; continue; }
        const float v = fminf(fmaxf(add_sep((float)in[k], nz[k]), 0.f), 255.f);
        out[k] = (uint8_t)(int)v;
    }
}

// ------------------------------------------------------------------------------------------------
// JPEG round trip
// ------------------------------------------------------------------------------------------------
// ITU-T T.81 Annex K tables K.1 (luminance) and K.2 (chrominance), row-major
__constant__ uint8_t annex_k[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// the "islow" DCT's 13-bit constants
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633;
constexpr int F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995, F_3_072711026 = 25172;

__device__ inline int descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// one pass of the forward transform on d[0..8); FIRST: the row pass, which keeps 2 extra bits
template <bool FIRST>
__device__ inline void fdct8(int (&d)[8]) {
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int sh = FIRST ? 13 - 2 : 13 + 2;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * F_0_541196100;
    d[2] = descale(z1 + t13 * F_0_765366865, sh);
    d[6] = descale(z1 - t12 * F_1_847759065, sh);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int a4 = t4 * F_0_298631336, a5 = t5 * F_2_053119869, a6 = t6 * F_3_072711026, a7 = t7 * F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5;
    z4 = z4 * -F_0_390180644 + z5;
    d[7] = descale(a4 + z1 + z3, sh);
    d[5] = descale(a5 + z2 + z4, sh);
    d[3] = descale(a6 + z2 + z3, sh);
    d[1] = descale(a7 + z1 + z4, sh);
}

// one pass of the inverse transform; FIRST: the column pass
template <bool FIRST>
__device__ inline void idct8(int (&c)[8]) {
    int z2 = c[2], z3 = c[6];
    int z1 = (z2 + z3) * F_0_541196100;
    const int e2 = z1 - z3 * F_1_847759065, e3 = z1 + z2 * F_0_765366865;
    const int e0 = (c[0] + c[4]) * 8192, e1 = (c[0] - c[4]) * 8192;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int o0 = c[7], o1 = c[5], o2 = c[3], o3 = c[1];
    z1 = o0 + o3;
    z2 = o1 + o2;
    z3 = o0 + o2;
    int z4 = o1 + o3;
    const int z5 = (z3 + z4) * F_1_175875602;
    o0 *= F_0_298631336;
    o1 *= F_2_053119869;
    o2 *= F_3_072711026;
    o3 *= F_1_501321110;
    z1 *= -F_0_899976223;
    z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5;
    z4 = z4 * -F_0_390180644 + z5;
    o0 += z1 + z3;
    o1 += z2 + z4;
    o2 += z2 + z3;
    o3 += z1 + z4;
    constexpr int sh = FIRST ? 13 - 2 : 13 + 2 + 3;
    c[0] = descale(t10 + o3, sh); c[7] = descale(t10 - o3, sh);
    c[1] = descale(t11 + o2, sh); c[6] = descale(t11 - o2, sh);
    c[2] = descale(t12 + o1, sh); c[5] = descale(t12 - o1, sh);
    c[3] = descale(t13 + o0, sh); c[4] = descale(t13 - o0, sh);
}

__device__ inline int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// kernel 1.  grid (ceil(mx my / 4), B), 256 threads: wave w of workgroup g owns MCU 4 g + w of image blockIdx.y.
// yp [B][16 my][16 mx], cbp / crp [B][8 my][8 mx] decoded planes; qy / qcb / qcr the quantised coefficients in the same layouts (or NULL).
__global__ void __launch_bounds__(256) degrade_jpeg_mcu_kernel(const uint8_t* x, int H, int W, int mx, int my, const int* params, int* status, uint8_t* yp, uint8_t* cbp,
                                                               uint8_t* crp, int16_t* qy, int16_t* qcb, int16_t* qcr) {
    __shared__ int qt[2][64];
    __shared__ int blk[4][6][8][9];               // per wave: the six blocks' samples, then the transforms' workspace (rows padded to 9 words)
    __shared__ uint8_t cfull[4][2][16][16];       // per wave: full-resolution Cb, Cr of the tile
    const int b = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int q = params[(int64_t)b * SR_DEG_PARAMS + SR_DEG_JPEG_QUALITY];
    if (q < 1 || q > 100) {                       // 0: copied through by kernel 2; anything else outside 1..100 is a bad row, copied as well
        if (q != 0 && tid == 0 && blockIdx.x == 0) flag_bad_row(status, ST_JPEG, b, q);
        return;                                   // uniform over the workgroup
    }
    if (tid < 128) {
        const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
        const int v = ((int)annex_k[tid >> 6][tid & 63] * scale + 50) / 100;
        qt[tid >> 6][tid & 63] = v < 1 ? 1 : (v > 255 ? 255 : v);
    }
    const int nm = mx * my, mcu_raw = blockIdx.x * 4 + wv;
    const bool live = mcu_raw < nm;               // a wave past the last MCU repeats the last one's work and stores nothing (the barriers stay uniform)
    const int mcu = live ? mcu_raw : nm - 1;
    const int mj = mcu / mx, mi = mcu - mj * mx;
    const uint8_t* img = x + (int64_t)b * H * W * 3;

    // BGR -> YCbCr of the tile, the image's last row / column repeated beyond it
    for (int i = 0; i < 4; ++i) {
        const int p = lane + 64 * i, ty = p >> 4, tx = p & 15;
        const int sy = min(16 * mj + ty, H - 1), sx = min(16 * mi + tx, W - 1);
        const uint8_t* px = img + ((int64_t)sy * W + sx) * 3;
        const int bb = px[0], gg = px[1], rr = px[2];
        const int yv = (19595 * rr + 38470 * gg + 7471 * bb + 32768) >> 16;
        const int cb = (-11059 * rr - 21709 * gg + 32768 * bb + (128 << 16) + 32767) >> 16;
        const int cr = (32768 * rr - 27439 * gg - 5329 * bb + (128 << 16) + 32767) >> 16;
        blk[wv][(ty >> 3) * 2 + (tx >> 3)][ty & 7][tx & 7] = yv - 128;
        cfull[wv][0][ty][tx] = (uint8_t)cb;
        cfull[wv][1][ty][tx] = (uint8_t)cr;
    }
    __syncthreads();
    // h2v2: (a + b + c + d + bias) >> 2, bias 1, 2, 1, 2 ... along the row; chroma rows past the image's last one repeat that row's result
    {
        const int cr_ = lane >> 3, cc_ = lane & 7;
        const int real_rows = (H + 1) / 2 - 8 * mj;                      // >= 1: an MCU row starts inside the image
        const int lr = min(cr_, real_rows - 1);
        for (int ch = 0; ch < 2; ++ch) {
            const uint8_t(*c)[16] = cfull[wv][ch];
            const int s = c[2 * lr][2 * cc_] + c[2 * lr][2 * cc_ + 1] + c[2 * lr + 1][2 * cc_] + c[2 * lr + 1][2 * cc_ + 1] + 1 + (cc_ & 1);
            blk[wv][4 + ch][cr_][cc_] = (s >> 2) - 128;
        }
    }
    __syncthreads();
    const int bk = lane >> 3, ln = lane & 7;      // lanes 0..47: block and its row / column
    int d[8];
    if (lane < 48) {                              // forward rows, in place (a lane touches its own row only)
        for (int j = 0; j < 8; ++j) d[j] = blk[wv][bk][ln][j];
        fdct8<true>(d);
        for (int j = 0; j < 8; ++j) blk[wv][bk][ln][j] = d[j];
    }
    __syncthreads();
    if (lane < 48) {                              // forward columns, quantise, dequantise, inverse columns, in place (own column only)
        for (int j = 0; j < 8; ++j) d[j] = blk[wv][bk][j][ln];
        fdct8<false>(d);
        const int* tq = qt[bk >= 4];
        int16_t* qo = nullptr;
        if (live) {
            if (bk < 4 && qy) qo = qy + ((int64_t)b * 16 * my + 16 * mj + (bk >> 1) * 8) * (16 * mx) + 16 * mi + (bk & 1) * 8 + ln;
            if (bk == 4 && qcb) qo = qcb + ((int64_t)b * 8 * my + 8 * mj) * (8 * mx) + 8 * mi + ln;
            if (bk == 5 && qcr) qo = qcr + ((int64_t)b * 8 * my + 8 * mj) * (8 * mx) + 8 * mi + ln;
        }
        const int pitch = bk < 4 ? 16 * mx : 8 * mx;
        for (int j = 0; j < 8; ++j) {
            const int qv = tq[j * 8 + ln], div = qv * 8;                 // the transform's output carries a factor 8
            const int a = d[j] < 0 ? -d[j] : d[j];
            const int m = (a + (div >> 1)) / div;                        // round half away from zero
            const int qc = d[j] < 0 ? -m : m;
            if (qo) qo[(int64_t)j * pitch] = (int16_t)qc;
            d[j] = qc * qv;
        }
        idct8<true>(d);
        for (int j = 0; j < 8; ++j) blk[wv][bk][j][ln] = d[j];
    }
    __syncthreads();
    if (lane < 48 && live) {                      // inverse rows, range limit, 8 bytes per lane
        for (int j = 0; j < 8; ++j) d[j] = blk[wv][bk][ln][j];
        idct8<false>(d);
        uint32_t lo = 0, hi = 0;
        for (int j = 0; j < 4; ++j) {
            lo |= (uint32_t)clamp255(d[j] + 128) << (8 * j);
            hi |= (uint32_t)clamp255(d[j + 4] + 128) << (8 * j);
        }
        uint8_t* o;
        if (bk < 4) o = yp + ((int64_t)b * 16 * my + 16 * mj + (bk >> 1) * 8 + ln) * (16 * mx) + 16 * mi + (bk & 1) * 8;
        else o = (bk == 4 ? cbp : crp) + ((int64_t)b * 8 * my + 8 * mj + ln) * (8 * mx) + 8 * mi;
        *reinterpret_cast<uint2*>(o) = make_uint2(lo, hi);               // 8-byte aligned: plane bases are, pitches and offsets are multiples of 8
    }
}

// kernel 2.  grid (ceil(W / 64), ceil(H / 4), B), block (64, 4)
__global__ void __launch_bounds__(256) degrade_jpeg_color_kernel(const uint8_t* x, int H, int W, int mx, int my, const int* params, const uint8_t* yp, const uint8_t* cbp,
                                                                 const uint8_t* crp, uint8_t* y) {
    const int b = blockIdx.z, xx = blockIdx.x * 64 + threadIdx.x, yy = blockIdx.y * 4 + threadIdx.y;
    if (xx >= W || yy >= H) return;
    const int64_t o = (((int64_t)b * H + yy) * W + xx) * 3;
    const int q = params[(int64_t)b * SR_DEG_PARAMS + SR_DEG_JPEG_QUALITY];
    if (q < 1 || q > 100) {
        y[o] = x[o]; y[o + 1] = x[o + 1]; y[o + 2] = x[o + 2];
        return;
    }
    const int hc = (H + 1) >> 1, wc = (W + 1) >> 1;                      // the chroma planes' real part
    const int cy = yy >> 1, cx = xx >> 1;
    const int fy = (yy & 1) ? min(cy + 1, hc - 1) : max(cy - 1, 0);      // the further row; the edge rows take themselves
    const int nx = (xx & 1) ? min(cx + 1, wc - 1) : max(cx - 1, 0);      // the further column, likewise
    const int rnd = (xx & 1) ? 7 : 8;
    const int lum = yp[((int64_t)b * 16 * my + yy) * (16 * mx) + xx];
    int cv[2];
    for (int ch = 0; ch < 2; ++ch) {
        const uint8_t* c = (ch ? crp : cbp) + (int64_t)b * 8 * my * 8 * mx;
        const uint8_t *rn = c + (int64_t)cy * (8 * mx), *rf = c + (int64_t)fy * (8 * mx);
        const int here = 3 * rn[cx] + rf[cx], there = 3 * rn[nx] + rf[nx];
        cv[ch] = (3 * here + there + rnd) >> 4;
    }
    const int u = cv[0] - 128, v = cv[1] - 128;
    y[o] = (uint8_t)clamp255(lum + ((116130 * u + 32768) >> 16));
    y[o + 1] = (uint8_t)clamp255(lum + ((-22554 * u - 46802 * v + 32768) >> 16));
    y[o + 2] = (uint8_t)clamp255(lum + ((91881 * v + 32768) >> 16));
}

int check_call(sr_ctx* ctx, const char* who, const void* x, const void* params, const void* y, int B, int H, int W) {
    if (!x || !params || !y) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": null tensor");
    if (B < 1 || B > 32767) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": empty or oversized batch (1 <= B <= 32767)");
    if (H < DEG_MIN || W < DEG_MIN || H > DEG_MAX || W > DEG_MAX)
        return ctx->fail(SR_ERR_INVALID, std::string(who) + ": H and W must lie in 16 .. 4096, got " + std::to_string(H) + " x " + std::to_string(W));
    return SR_OK;
}

int status_words(sr_ctx* ctx, hipStream_t st, int** out) {
    if (!ctx->deg_status) {
        ctx->deg_status = static_cast<int*>(ctx->dalloc(4 * sizeof(int)));
        if (!ctx->deg_status) return SR_ERR_OOM;
        SR_HIP(ctx, hipMemsetAsync(ctx->deg_status, 0, 4 * sizeof(int), st));
        SR_HIP(ctx, hipStreamSynchronize(st));       // once per context: later calls may come on other streams
    }
    *out = ctx->deg_status;
    return SR_OK;
}

}  // namespace

extern "C" {

int sr_degrade_gauss(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (int rc = check_call(ctx, "degrade_gauss", x_u8, params_i32, y_u8, B, H, W)) return rc;
    if (x_u8 == y_u8) return ctx->fail(SR_ERR_INVALID, "degrade_gauss: the blur cannot run in place");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status;
    if (int rc = status_words(ctx, st, &status)) return rc;
    const int rec = ctx->prof_open("degrade_gauss", 0.0, 2.0 * B * H * (double)W * 3.0, st);
    hipLaunchKernelGGL(degrade_gauss_kernel, dim3((W + GT_ - 1) / GT_, (H + GT_ - 1) / GT_, B), dim3(256), 0, st, x_u8, H, W, params_i32, status, y_u8);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_degrade_motion(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (int rc = check_call(ctx, "degrade_motion", x_u8, params_i32, y_u8, B, H, W)) return rc;
    if (x_u8 == y_u8) return ctx->fail(SR_ERR_INVALID, "degrade_motion: the blur cannot run in place");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status;
    if (int rc = status_words(ctx, st, &status)) return rc;
    const int64_t total = (int64_t)B * H * W * 3;
    const int rec = ctx->prof_open("degrade_motion", 0.0, 2.0 * (double)total, st);
    hipLaunchKernelGGL(degrade_motion_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1 << 20)), dim3(256), 0, st, x_u8, B, H, W, params_i32, status, y_u8);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_degrade_noise(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, const float* field_f32, uint64_t seed, uint8_t* y_u8,
                     float* z_f32, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (int rc = check_call(ctx, "degrade_noise", x_u8, params_i32, y_u8, B, H, W)) return rc;
    if (field_f32 && z_f32) return ctx->fail(SR_ERR_INVALID, "degrade_noise: the raw z output belongs to the kernel's own generator, not to a supplied field");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status;
    if (int rc = status_words(ctx, st, &status)) return rc;
    const int n = H * W * 3;                                                 // <= 3 * 2^24
    const int rec = ctx->prof_open("degrade_noise", 0.0, 2.0 * B * (double)n, st);
    hipLaunchKernelGGL(degrade_noise_kernel, dim3(((n + 3) / 4 + 255) / 256, B), dim3(256), 0, st, x_u8, n, params_i32, field_f32, (unsigned long long)seed, status, y_u8,
                       z_f32);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_degrade_jpeg(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, int16_t* coef_y_i16, int16_t* coef_cb_i16,
                    int16_t* coef_cr_i16, uint8_t* plane_y_u8, uint8_t* plane_cb_u8, uint8_t* plane_cr_u8, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (int rc = check_call(ctx, "degrade_jpeg", x_u8, params_i32, y_u8, B, H, W)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int* status;
    if (int rc = status_words(ctx, st, &status)) return rc;
    const int mx = (W + 15) / 16, my = (H + 15) / 16;
    const size_t b_y = al256((size_t)B * 256 * mx * my), b_c = al256((size_t)B * 64 * mx * my);
    char* wk = static_cast<char*>(ctx->arena(ctx->deg_work, b_y + 2 * b_c, st));
    if (!wk) return SR_ERR_OOM;
    uint8_t* yp = plane_y_u8 ? plane_y_u8 : reinterpret_cast<uint8_t*>(wk);
    uint8_t* cbp = plane_cb_u8 ? plane_cb_u8 : reinterpret_cast<uint8_t*>(wk + b_y);
    uint8_t* crp = plane_cr_u8 ? plane_cr_u8 : reinterpret_cast<uint8_t*>(wk + b_y + b_c);
    if (((uintptr_t)yp | (uintptr_t)cbp | (uintptr_t)crp) & 7) return ctx->fail(SR_ERR_INVALID, "degrade_jpeg: the raw plane outputs must be 8-byte aligned");
    int rec = ctx->prof_open("degrade_jpeg_mcu", 0.0, (double)B * H * W * 4.5, st);
    hipLaunchKernelGGL(degrade_jpeg_mcu_kernel, dim3((mx * my + 3) / 4, B), dim3(256), 0, st, x_u8, H, W, mx, my, params_i32, status, yp, cbp, crp, coef_y_i16,
                       coef_cb_i16, coef_cr_i16);
    ctx->prof_close(rec, st);
    rec = ctx->prof_open("degrade_jpeg_color", 0.0, (double)B * H * W * 4.5, st);
    hipLaunchKernelGGL(degrade_jpeg_color_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, st, x_u8, H, W, mx, my, params_i32, yp, cbp, crp, y_u8);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_degrade_status(sr_ctx* ctx, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!ctx->deg_status) return SR_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int h[4] = {0, 0, 0, 0};
    SR_HIP(ctx, hipMemcpyAsync(h, ctx->deg_status, sizeof(h), hipMemcpyDeviceToHost, st));
    SR_HIP(ctx, hipStreamSynchronize(st));
    if (h[0] == 0) return SR_OK;
    SR_HIP(ctx, hipMemsetAsync(ctx->deg_status, 0, sizeof(h), st));
    static const char* const stage[] = {"", "degrade_gauss: kernel size must be 3, 5 or 7 with taps in 0..256 that sum to 256", "degrade_motion: size must be 5, 7 or 9",
                                        "degrade_noise: the deviation must be finite and not negative", "degrade_jpeg: quality must lie in 1 .. 100"};
    const int s = h[0] >= ST_GAUSS && h[0] <= ST_JPEG ? h[0] : 0;
    return ctx->fail(SR_ERR_INVALID, std::string(stage[s]) + " (row " + std::to_string(h[1]) + " of the parameter table holds " + std::to_string(h[2]) +
                                         "; that image was copied through)");
}

}  // extern "C"
