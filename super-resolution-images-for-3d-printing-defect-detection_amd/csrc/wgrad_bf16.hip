// wgrad_bf16.hip -- the bf16-storage pieces of a mixed-precision training step (EDSR_model.py:127-176 trained with bf16 activations and activation
// gradients, fp32 master weights / gradients / optimiser; include/sr355.h, DESIGN.md "Mixed-precision training"):
//   * wgrad3_bf16_kernel: dW[ky,kx,ci,co] = scale * sum over pixels of X[b, y+ky-1, x+kx-1, ci] * dY[b,y,x,co] of a 3x3 SAME conv on bf16 X and dY, fp32 out, on
//     v_mfma_f32_32x32x16_bf16.  The reduction axis is the pixel axis and both tensors are channel-contiguous, so both MFMA operands (8 consecutive pixels of one
//     channel per lane) are transposes of what memory holds: the tiles are staged PIXEL-major, as they lie in memory, and read with ds_read_b64_tr_b16.
//   * relu_bwd / space_to_depth on bf16 (selects and permutations: bit-exact), and the fused clip + MSE loss + loss gradient.
#include "common.h"
#include "fp_sep.h"

#include <cmath>

namespace {

// ---- weight gradient.  wgrad3_tile_kernel's scheme (train_ops.hip) on bf16 operands: a workgroup owns a (32-cin block, 32-cout block) pair and a run of image tiles; the
// x tile with its one-pixel zero halo and the dy tile are staged into LDS, [pixel][32 channels] bf16 = 64 bytes per pixel; every group of 16 consecutive dy pixels meets
// the nine shifted groups of x pixels in nine fp32 accumulator tiles; the four waves' tiles are summed through LDS in wave order, the runs of tiles (pixel splits) by
// wgrad_bf16_finish_kernel in split order -- no atomics, two runs give the same bits.
//
// The tile is 8 rows x 16 pixels: a group of 16 reduction pixels is exactly one tile row, so it never straddles an image row, and the x operand of tap (ky, kx) is the
// 16 consecutive halo-tile pixels that start (ky, kx) further on -- a constant byte offset from the centre tap's address.  Out-of-image pixels are staged as zeros.
//
// One ds_read_b64_tr_b16 hands lane 16 g + i (g = 0..3) channel i of a 4-pixel x 16-channel block whose row q, channels 4 p .. 4 p + 3 lane 16 g + 4 q + p addresses.
// Group g takes channels 16 (g & 1) .. + 15 of pixels 8 (g >> 1) + 4 r .. + 3 for read r = 0, 1: lane l then holds channel l & 31, pixels 8 (l >> 5) + 0 .. 7 of the
// group in eight bf16 -- the A / B operand of the 32x32x16 MFMA.  A 32-lane half reads 4 pixels x 64 bytes = one whole 256-byte bank row: conflict-free.  The
// instruction needs EXEC all ones: every loop around it has a workgroup-uniform trip count and no lane leaves early.
constexpr int WB_TH = 8, WB_TW = 16, WB_PH = WB_TH + 2, WB_PW = WB_TW + 2, WB_NPIX = WB_TH * WB_TW;
constexpr int WB_XT_BYTES = WB_PH * WB_PW * 64, WB_DT_BYTES = WB_NPIX * 64;
constexpr int WB_MAX_SPLIT = 64;          // pixel splits per (cin block, cout block) pair at most
static_assert(WB_XT_BYTES + WB_DT_BYTES >= 4 * 1024 * (int)sizeof(float), "the waves' reduction fits the two tiles' space");

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x4 lds_read_tr(const bf16_t* p) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
    return __builtin_bit_cast(bf16x4, v);
}

__device__ __forceinline__ bf16x8 join8(bf16x4 a, bf16x4 b) { return __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7); }

// 8 channels from c of one pixel (src at the pixel's channel c), zero beyond C
__device__ __forceinline__ u16x8 stage8(const uint16_t* src, int c, int C, bool vec) {
    u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (vec) return *reinterpret_cast<const u16x8*>(src);        // C a multiple of 8: all eight are the tensor's own
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c + e < C ? src[e] : (uint16_t)0;
    return v;
}

__global__ void __launch_bounds__(256) wgrad3_bf16_kernel(const uint16_t* x, int64_t x_cs, const uint16_t* dy, int64_t dy_cs, int B, int H, int W, int Cin, int Cout, int nci,
                                                          int nco, int tiles_per_wg, int tilesX, int tilesY, float* partial, double* bpart) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[WB_XT_BYTES + WB_DT_BYTES];
    uint16_t* xt = reinterpret_cast<uint16_t*>(smem);                     // [WB_PH * WB_PW pixels][32 channels]
    uint16_t* dt = reinterpret_cast<uint16_t*>(smem + WB_XT_BYTES);       // [WB_NPIX pixels][32 channels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, k = lane >> 5;
    const int cob = blockIdx.x % nco, cib = blockIdx.x / nco;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int ntile = B * tilesY * tilesX;
    const int t0 = blockIdx.y * tiles_per_wg, t1 = min(ntile, t0 + tiles_per_wg);
    const bool vec_x = (Cin & 7) == 0 && (x_cs & 7) == 0 && ((uintptr_t)x & 15) == 0, vec_y = (Cout & 7) == 0 && (dy_cs & 7) == 0 && ((uintptr_t)dy & 15) == 0;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const bool do_b = bpart != nullptr && cib == 0;
    double bsum = 0.0;                                             // cout tid & 31, pixel group tid >> 5
    // this lane's share of a transposed read: pixel q of the 4-pixel block of its 16-lane group, channels 4 p .. 4 p + 3 of the group's 16
    const int tg = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int tr_pix = 8 * (tg >> 1) + tq, tr_ch = 16 * (tg & 1) + 4 * tp;
    for (int tile = t0; tile < t1; ++tile) {                       // (workgroup-uniform bounds)
        int tt = tile;
        const int tx = tt % tilesX; tt /= tilesX;
        const int ty = tt % tilesY;
        const int b = tt / tilesY;
        const int y0 = ty * WB_TH, x0 = tx * WB_TW;
        __syncthreads();                                           // the previous tile's operands have been read
        for (int u = tid; u < WB_PH * WB_PW * 4; u += 256) {
            const int pix = u >> 2, sl = u & 3;
            const int py = pix / WB_PW, px = pix - py * WB_PW;
            const int gy = y0 + py - 1, gx = x0 + px - 1;
            const int c = ci0 + sl * 8;
            u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W && c < Cin) v = stage8(x + (((int64_t)b * H + gy) * W + gx) * x_cs + c, c, Cin, vec_x);
            *reinterpret_cast<u16x8*>(xt + pix * 32 + sl * 8) = v;
        }
        for (int u = tid; u < WB_NPIX * 4; u += 256) {
            const int pix = u >> 2, sl = u & 3;
            const int py = pix / WB_TW, px = pix - py * WB_TW;
            const int gy = y0 + py, gx = x0 + px;
            const int c = co0 + sl * 8;
            u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (gy < H && gx < W && c < Cout) v = stage8(dy + (((int64_t)b * H + gy) * W + gx) * dy_cs + c, c, Cout, vec_y);
            *reinterpret_cast<u16x8*>(dt + pix * 32 + sl * 8) = v;
        }
        __syncthreads();
        if (do_b) {
            const int co = tid & 31;
            for (int p = tid >> 5; p < WB_NPIX; p += 8) bsum += (double)__uint_as_float((uint32_t)dt[p * 32 + co] << 16);
        }
        static_assert(WB_TH % 4 == 0, "every wave takes the same number of tile rows");
#pragma unroll
        for (int rr = 0; rr < WB_TH / 4; ++rr) {                   // one group of 16 pixels = one tile row; a constant trip count: no lane-dependent branch, EXEC stays all ones
            const int row = wave + 4 * rr;
            const bf16_t* db0 = reinterpret_cast<const bf16_t*>(dt) + (row * WB_TW + tr_pix) * 32 + tr_ch;
            const bf16x8 bv = join8(lds_read_tr(db0), lds_read_tr(db0 + 4 * 32));
            const bf16_t* xb0 = reinterpret_cast<const bf16_t*>(xt) + (row * WB_PW + tr_pix) * 32 + tr_ch;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const bf16_t* xb = xb0 + (ky * WB_PW + kx) * 32;
                    const bf16x8 av = join8(lds_read_tr(xb), lds_read_tr(xb + 4 * 32));
                    acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av, bv, acc[ky * 3 + kx], 0, 0, 0);
                }
        }
    }
    float* red = reinterpret_cast<float*>(smem);                   // 4 x 1024 floats over the two tiles' space
    const int ntiles_out = 9 * nci * nco;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * k;        // C/D layout of the 32x32 MFMA: col = lane & 31, row from the register index
            red[wave * 1024 + row * 32 + i] = acc[t][e];
        }
        __syncthreads();
        float* out = partial + (((size_t)blockIdx.y * ntiles_out + (t * nci + cib) * nco + cob) * 1024);
        for (int e = tid; e < 1024; e += 256) out[e] = (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]);
    }
    if (do_b) {
        __syncthreads();
        double* bred = reinterpret_cast<double*>(smem);            // [8][32] doubles
        bred[(tid >> 5) * 32 + (tid & 31)] = bsum;
        __syncthreads();
        if (tid < 32) {
            double t2 = 0.0;
            for (int j = 0; j < 8; ++j) t2 += bred[j * 32 + tid];
            bpart[((size_t)blockIdx.y * nco + cob) * 32 + tid] = t2;
        }
    }
}

// one thread per element of a quarter (blockIdx.y) of one 32x32 tile: the splits' partial tiles in split order, times `scale` in fp32; dw is HWIO [tap][Cin][Cout]
__global__ void wgrad_bf16_finish_kernel(const float* partial, int ntiles, int nsplit, int Cin, int Cout, int nci, int nco, float scale, float* dw, const double* bpart, float* db) {
    const int tile = blockIdx.x;
    int t = tile;
    const int cob = t % nco; t /= nco;
    const int cib = t % nci;
    const int tap = t / nci;
    {
        const int e = blockIdx.y * 256 + threadIdx.x;
        const int ci = cib * 32 + e / 32, co = cob * 32 + (e & 31);
        if (ci < Cin && co < Cout) {
            float s = 0.f;
#pragma unroll 16
            for (int sp = 0; sp < nsplit; ++sp) s += partial[((size_t)sp * ntiles + tile) * 1024 + e];
            dw[((size_t)tap * Cin + ci) * Cout + co] = mul_sep(scale, s);
        }
    }
    if (bpart && db && tap == 0 && cib == 0 && blockIdx.y == 0 && threadIdx.x < 32 && cob * 32 + (int)threadIdx.x < Cout) {
        double t2 = 0.0;
#pragma unroll 16
        for (int sp = 0; sp < nsplit; ++sp) t2 += bpart[((size_t)sp * nco + cob) * 32 + threadIdx.x];
        db[cob * 32 + threadIdx.x] = (float)((double)scale * t2);
    }
}

// ---- element-wise.  bf16 values travel as their 16 bits: a select or a permutation cannot round
constexpr int ELT_MAX_BLOCKS = 65535;
unsigned grid_n(int64_t n) { int64_t g = (n + 255) / 256; return (unsigned)(g < 1 ? 1 : (g > ELT_MAX_BLOCKS ? ELT_MAX_BLOCKS : g)); }

__device__ __forceinline__ float bf16_bits_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

__global__ void relu_bwd_bf16_kernel(const uint16_t* dy, const uint16_t* y, uint16_t* out, int64_t n) {
    // y > 0 read off the bits (sign clear, not zero, not NaN): the smallest positive bf16 is a subnormal, and no float mode may decide whether it counts
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint16_t v = y[i], mag = v & 0x7fffu;
        out[i] = (!(v & 0x8000u) && mag != 0 && mag <= 0x7f80u) ? dy[i] : (uint16_t)0;
    }
}

// inverse of tf.nn.depth_to_space (DCR): x [B, H*r, W*r, C] -> y [B, H, W, (i*r + j)*C + c]
__global__ void space_to_depth_bf16_kernel(const uint16_t* x, int B, int H, int W, int C, int r, uint16_t* y) {
    const int64_t n = (int64_t)B * H * W * r * r * C;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int cc = (int)(idx % (r * r * C));
        int64_t t = idx / (r * r * C);
        const int w = (int)(t % W); t /= W;
        const int h = (int)(t % H);
        const int64_t b = t / H;
        const int sub = cc / C, c = cc - sub * C, i = sub / r, j = sub - i * r;
        y[idx] = x[(((b * H * r) + (int64_t)h * r + i) * ((int64_t)W * r) + (int64_t)w * r + j) * C + c];
    }
}

// ---- loss.  y = clip(pre, 0, 1) in fp32; dpre = bf16(c * (y - t)) where 0 <= pre <= 1, else 0, c = fp32(2 / n), each fp32 operation rounded on its own (NumPy's
// evaluation of np.float32(2 / n) * (y - t)), then one round to nearest even; loss = mean (y - t)^2: every difference and square exact in fp64, a thread adds its
// elements in index order, the workgroup's 256 sums go through a fixed LDS tree, the workgroups' partial sums are added by one thread in block order.
constexpr int MSE_MAX_BLOCKS = 1024;

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

__global__ void __launch_bounds__(256) mse_clip_grad_bf16_kernel(const uint16_t* __restrict__ pre, const float* __restrict__ t, int64_t n, float c, uint16_t* __restrict__ dpre,
                                                                 float* __restrict__ y, double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        // 0 <= pre <= 1 read off the bits (-0 is inside; the neighbours of 0 are subnormals, and no float mode may decide on which side they fall)
        const uint16_t pb = pre[i], mag = pb & 0x7fffu;
        const bool neg = (pb & 0x8000u) != 0, inside = neg ? mag == 0 : mag <= 0x3f80u;
        const float ti = t[i];
        const float yi = inside ? bf16_bits_to_f32(pb) : ((neg || mag > 0x7f80u) ? 0.f : 1.f);
        const double d = (double)yi - (double)ti;
        s = add_sep(s, mul_sep(d, d));
        dpre[i] = inside ? f32_to_bf16_rne(mul_sep(c, sub_sep(yi, ti))) : (uint16_t)0;
        if (y) y[i] = yi;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = add_sep(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ void mse_finish_kernel(const double* partial, int nblk, double n, float* loss) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s = add_sep(s, partial[b]);
        loss[0] = (float)(s / n);
    }
}

}  // namespace

int wgrad_bf16_launch(sr_ctx* ctx, const bf16_t* x, int64_t x_cs, const bf16_t* dy, int64_t dy_cs, int B, int H, int W, int Cin, int Cout, float scale, float* dw, float* db,
                      hipStream_t st) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: empty tensor");
    if (x_cs < Cin || dy_cs < Cout) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: a channel stride is smaller than its channel count");
    const int nci = (Cin + 31) / 32, nco = (Cout + 31) / 32;
    if ((int64_t)nci * nco > 0x7fffffff / 9) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: too many channels");
    const int ntiles = 9 * nci * nco;
    const int tilesX = (W + WB_TW - 1) / WB_TW, tilesY = (H + WB_TH - 1) / WB_TH;
    if ((int64_t)B * tilesY * tilesX > 0x7fffffff) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: too many tiles");
    const int ntile = B * tilesY * tilesX;
    // pixel splits: enough workgroups for ~1.5 per CU, each a whole number of tiles
    int nsplit = (3 * ctx->cu_count() / 2 + nci * nco - 1) / (nci * nco);
    if (nsplit > ntile) nsplit = ntile;
    if (nsplit > WB_MAX_SPLIT) nsplit = WB_MAX_SPLIT;
    if (nsplit < 1) nsplit = 1;
    const int tiles_per_wg = (ntile + nsplit - 1) / nsplit;
    nsplit = (ntile + tiles_per_wg - 1) / tiles_per_wg;
    const size_t tile_bytes = (size_t)nsplit * ntiles * 1024 * sizeof(float);
    float* partial = static_cast<float*>(ctx->scratch(tile_bytes + (size_t)nsplit * nco * 32 * sizeof(double)));
    if (!partial) return SR_ERR_OOM;
    double* bpart = db ? reinterpret_cast<double*>(reinterpret_cast<char*>(partial) + tile_bytes) : nullptr;
    hipLaunchKernelGGL(wgrad3_bf16_kernel, dim3(nci * nco, nsplit), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(x), x_cs, reinterpret_cast<const uint16_t*>(dy), dy_cs, B, H, W,
                       Cin, Cout, nci, nco, tiles_per_wg, tilesX, tilesY, partial, bpart);
    hipLaunchKernelGGL(wgrad_bf16_finish_kernel, dim3(ntiles, 4), dim3(256), 0, st, partial, ntiles, nsplit, Cin, Cout, nci, nco, scale, dw, bpart, db);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int relu_bwd_bf16_launch(sr_ctx* ctx, const bf16_t* dy, const bf16_t* y, bf16_t* out, int64_t n, hipStream_t st) {
    if (n <= 0) return ctx->fail(SR_ERR_INVALID, "relu_bwd_bf16: empty tensor");
    hipLaunchKernelGGL(relu_bwd_bf16_kernel, dim3(grid_n(n)), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(dy), reinterpret_cast<const uint16_t*>(y),
                       reinterpret_cast<uint16_t*>(out), n);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int space_to_depth_bf16_launch(sr_ctx* ctx, const bf16_t* x, int B, int H, int W, int C, int r, bf16_t* y, hipStream_t st) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || r < 1) return ctx->fail(SR_ERR_INVALID, "space_to_depth_bf16: bad shape");
    const int64_t n = (int64_t)B * H * W * r * r * C;
    hipLaunchKernelGGL(space_to_depth_bf16_kernel, dim3(grid_n(n)), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(x), B, H, W, C, r, reinterpret_cast<uint16_t*>(y));
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int mse_clip_grad_bf16_launch(sr_ctx* ctx, const bf16_t* pre, const float* t, int64_t n, float* loss, bf16_t* dpre, float* y, hipStream_t st) {
    if (n <= 0) return ctx->fail(SR_ERR_INVALID, "mse_clip_grad_bf16: empty tensor");
    const int64_t want = (n + 255) / 256;
    const int nblk = (int)(want > MSE_MAX_BLOCKS ? MSE_MAX_BLOCKS : want);
    double* partial = static_cast<double*>(ctx->scratch(sizeof(double) * MSE_MAX_BLOCKS));
    if (!partial) return SR_ERR_OOM;
    hipLaunchKernelGGL(mse_clip_grad_bf16_kernel, dim3(nblk), dim3(256), 0, st, reinterpret_cast<const uint16_t*>(pre), t, n, (float)(2.0 / (double)n),
                       reinterpret_cast<uint16_t*>(dpre), y, partial);
    hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(64), 0, st, partial, nblk, (double)n, loss);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
