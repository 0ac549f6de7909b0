// wgrad_bf16.hip -- the bf16-storage pieces of a mixed-precision training step (EDSR_model.py:127-176 trained with bf16 activations and activation
// gradients, fp32 master weights / gradients / optimiser; include/sr355.h, DESIGN.md "Mixed-precision training"):
//   * wgrad3_bf16_group_kernel: dW[ky,kx,ci,co] = scale * sum over pixels of X[b, y+ky-1, x+kx-1, ci] * dY[b,y,x,co] of a 3x3 SAME conv on bf16 X and dY, fp32 out, on
//     v_mfma_f32_32x32x16_bf16.  The reduction axis is the pixel axis and both tensors are channel-contiguous, so both MFMA operands (8 consecutive pixels of one
//     channel per lane) are transposes of what memory holds: the tiles are staged PIXEL-major, as they lie in memory, and read with ds_read_b64_tr_b16.
//     One launch serves up to SR_WGRAD_GROUP_MAX layers that share [B,H,W] (sr_conv2d_wgrad_group_bf16: the five layers of a dense block read prefixes of one buffer).
//   * relu_bwd / space_to_depth on bf16 (selects and permutations: bit-exact), the same select and an axpby on channel ranges, and the fused clip + MSE loss + loss gradient.
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

// A group of layers in one launch: blockIdx.x enumerates the (cin block, cout block) pairs of all jobs in job order, job j owning pairs [pair0, next job's pair0); the table
// travels by value in the kernel arguments (no upload, no sync).  Every job shares [B,H,W], hence the tile walk and the trip counts below: workgroup-uniform whatever the job.
struct WgJob {
    const uint16_t* x;  int64_t x_cs;     // first channel of the view, channels per pixel of its buffer
    const uint16_t* dy; int64_t dy_cs;
    float* dw; float* db;                 // HWIO [9][Cin][Cout], [Cout] or null
    int Cin, Cout, nci, nco;
    int pair0, bco0;                      // first pair; first 32-cout block among the group's bias partials
    float scale;
};
struct WgTable { WgJob j[SR_WGRAD_GROUP_MAX]; int n, npairs, nbco; };

__device__ __forceinline__ int wg_job_of(const WgTable& t, int pair) {
    int j = 0;
#pragma unroll
    for (int q = 1; q < SR_WGRAD_GROUP_MAX; ++q) j += (q < t.n && pair >= t.j[q].pair0) ? 1 : 0;
    return j;
}

__global__ void __launch_bounds__(256) wgrad3_bf16_group_kernel(const WgTable tab, int B, int H, int W, int tiles_per_wg, int tilesX, int tilesY, float* partial, double* bpart) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[WB_XT_BYTES + WB_DT_BYTES];
    uint16_t* xt = reinterpret_cast<uint16_t*>(smem);                     // [WB_PH * WB_PW pixels][32 channels]
    uint16_t* dt = reinterpret_cast<uint16_t*>(smem + WB_XT_BYTES);       // [WB_NPIX pixels][32 channels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 31, k = lane >> 5;
    const WgJob& jb = tab.j[wg_job_of(tab, blockIdx.x)];
    const uint16_t* x = jb.x; const uint16_t* dy = jb.dy;
    const int64_t x_cs = jb.x_cs, dy_cs = jb.dy_cs;
    const int Cin = jb.Cin, Cout = jb.Cout, nco = jb.nco;
    const int lp = blockIdx.x - jb.pair0;                                 // the pair within its job
    const int cob = lp % nco, cib = lp / nco;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int ntile = B * tilesY * tilesX;
    const int t0 = blockIdx.y * tiles_per_wg, t1 = min(ntile, t0 + tiles_per_wg);
    const bool vec_x = (Cin & 7) == 0 && (x_cs & 7) == 0 && ((uintptr_t)x & 15) == 0, vec_y = (Cout & 7) == 0 && (dy_cs & 7) == 0 && ((uintptr_t)dy & 15) == 0;
    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    const bool do_b = jb.db != nullptr && cib == 0;
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
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = (e & 3) + 8 * (e >> 2) + 4 * k;        // C/D layout of the 32x32 MFMA: col = lane & 31, row from the register index
            red[wave * 1024 + row * 32 + i] = acc[t][e];
        }
        __syncthreads();
        float* out = partial + (((size_t)blockIdx.y * tab.npairs + blockIdx.x) * 9 + t) * 1024;
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
            bpart[((size_t)blockIdx.y * tab.nbco + jb.bco0 + cob) * 32 + tid] = t2;
        }
    }
}

// one thread per element of a quarter (blockIdx.y) of one 32x32 tile (blockIdx.x = pair * 9 + tap): the splits' partial tiles in split order, times the job's `scale` in
// fp32; dw is the job's HWIO [tap][Cin][Cout]
__global__ void wgrad_bf16_finish_kernel(const WgTable tab, const float* partial, int nsplit, const double* bpart) {
    const int pair = blockIdx.x / 9, tap = blockIdx.x - pair * 9;
    const WgJob& jb = tab.j[wg_job_of(tab, pair)];
    const int Cin = jb.Cin, Cout = jb.Cout, nco = jb.nco;
    const int lp = pair - jb.pair0;
    const int cob = lp % nco, cib = lp / nco;
    const float scale = jb.scale;
    {
        const int e = blockIdx.y * 256 + threadIdx.x;
        const int ci = cib * 32 + e / 32, co = cob * 32 + (e & 31);
        if (ci < Cin && co < Cout) {
            float s = 0.f;
#pragma unroll 16
            for (int sp = 0; sp < nsplit; ++sp) s += partial[(((size_t)sp * tab.npairs + pair) * 9 + tap) * 1024 + e];
            jb.dw[((size_t)tap * Cin + ci) * Cout + co] = mul_sep(scale, s);
        }
    }
    if (jb.db && tap == 0 && cib == 0 && blockIdx.y == 0 && threadIdx.x < 32 && cob * 32 + (int)threadIdx.x < Cout) {
        double t2 = 0.0;
#pragma unroll 16
        for (int sp = 0; sp < nsplit; ++sp) t2 += bpart[((size_t)sp * tab.nbco + jb.bco0 + cob) * 32 + threadIdx.x];
        jb.db[cob * 32 + threadIdx.x] = (float)((double)scale * t2);
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

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// the same select, and alpha * a + beta * b (fp32 arithmetic on the widened values, one rounding to nearest even), over C channels of every pixel of bf16 buffers: a / b /
// out point at their view's first channel, *_cs are the buffers' channels per pixel (a dense block's dz_k read off G and F where they lie; an RRDB's dX1 + dR)
template <bool RELU>
__global__ void eltwise_views_bf16_kernel(const uint16_t* a, int64_t a_cs, const uint16_t* b, int64_t b_cs, float alpha, float beta, uint16_t* out, int64_t o_cs, int64_t npix, int C) {
    const int64_t n = npix * C;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < n; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pix = idx / C;
        const int c = (int)(idx - pix * C);
        const uint16_t av = a[pix * a_cs + c];
        if (RELU) {
            const uint16_t v = b[pix * b_cs + c], mag = v & 0x7fffu;
            out[pix * o_cs + c] = (!(v & 0x8000u) && mag != 0 && mag <= 0x7f80u) ? av : (uint16_t)0;
        } else {
            float r = alpha * bf16_bits_to_f32(av);
            if (b) r += beta * bf16_bits_to_f32(b[pix * b_cs + c]);
            out[pix * o_cs + c] = f32_to_bf16_rne(r);
        }
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

int wgrad_group_bf16_launch(sr_ctx* ctx, const sr_wgrad_job* jobs, int n, int B, int H, int W, hipStream_t st) {
    if (n < 1 || n > SR_WGRAD_GROUP_MAX || !jobs) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: a group has 1 to 8 jobs");
    if (B <= 0 || H <= 0 || W <= 0) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: empty tensor");
    WgTable tab = {};
    int64_t npairs = 0;
    int nbco = 0;
    bool any_b = false;
    for (int q = 0; q < n; ++q) {
        const sr_wgrad_job& s = jobs[q];
        WgJob& d = tab.j[q];
        if (!s.x.p || !s.dy.p || !s.dw) return ctx->fail(SR_ERR_INVALID, "null tensor");
        if (s.Cin <= 0 || s.Cout <= 0) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: empty tensor");
        if (s.x.coff < 0 || s.dy.coff < 0 || s.x.cs - s.x.coff < s.Cin || s.dy.cs - s.dy.coff < s.Cout)
            return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: a channel stride is smaller than its channel count");
        d.x = static_cast<const uint16_t*>(s.x.p) + s.x.coff; d.x_cs = s.x.cs;
        d.dy = static_cast<const uint16_t*>(s.dy.p) + s.dy.coff; d.dy_cs = s.dy.cs;
        d.dw = s.dw; d.db = s.db; d.scale = s.scale;
        d.Cin = s.Cin; d.Cout = s.Cout; d.nci = (s.Cin + 31) / 32; d.nco = (s.Cout + 31) / 32;
        d.pair0 = (int)npairs; d.bco0 = nbco;
        npairs += (int64_t)d.nci * d.nco;
        if (npairs > 0x7fffffff / 9) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: too many channels");
        nbco += d.nco;
        any_b = any_b || s.db;
    }
    tab.n = n; tab.npairs = (int)npairs; tab.nbco = nbco;
    const int tilesX = (W + WB_TW - 1) / WB_TW, tilesY = (H + WB_TH - 1) / WB_TH;
    if ((int64_t)B * tilesY * tilesX > 0x7fffffff) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: too many tiles");
    const int ntile = B * tilesY * tilesX;
    // pixel splits: enough workgroups for ~1.5 per CU over all the group's pairs, each a whole number of tiles
    int nsplit = (3 * ctx->cu_count() / 2 + tab.npairs - 1) / tab.npairs;
    if (nsplit > ntile) nsplit = ntile;
    if (nsplit > WB_MAX_SPLIT) nsplit = WB_MAX_SPLIT;
    if (nsplit < 1) nsplit = 1;
    const int tiles_per_wg = (ntile + nsplit - 1) / nsplit;
    nsplit = (ntile + tiles_per_wg - 1) / tiles_per_wg;
    const size_t tile_bytes = (size_t)nsplit * tab.npairs * 9 * 1024 * sizeof(float);
    float* partial = static_cast<float*>(ctx->scratch(tile_bytes + (size_t)nsplit * nbco * 32 * sizeof(double)));
    if (!partial) return SR_ERR_OOM;
    double* bpart = any_b ? reinterpret_cast<double*>(reinterpret_cast<char*>(partial) + tile_bytes) : nullptr;
    hipLaunchKernelGGL(wgrad3_bf16_group_kernel, dim3(tab.npairs, nsplit), dim3(256), 0, st, tab, B, H, W, tiles_per_wg, tilesX, tilesY, partial, bpart);
    hipLaunchKernelGGL(wgrad_bf16_finish_kernel, dim3(tab.npairs * 9, 4), dim3(256), 0, st, tab, partial, nsplit, bpart);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

// one layer: the group of one job (the same tiles, splits and orders of summation)
int wgrad_bf16_launch(sr_ctx* ctx, const bf16_t* x, int64_t x_cs, const bf16_t* dy, int64_t dy_cs, int B, int H, int W, int Cin, int Cout, float scale, float* dw, float* db,
                      hipStream_t st) {
    if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return ctx->fail(SR_ERR_INVALID, "wgrad_bf16: empty tensor");
    sr_wgrad_job jb = {};
    jb.x = sr_view{x, x_cs, 0}; jb.dy = sr_view{dy, dy_cs, 0};
    jb.Cin = Cin; jb.Cout = Cout; jb.scale = scale; jb.dw = dw; jb.db = db;
    return wgrad_group_bf16_launch(ctx, &jb, 1, B, H, W, st);
}

int eltwise_views_bf16_launch(sr_ctx* ctx, int op, const bf16_t* a, int64_t a_cs, const bf16_t* b, int64_t b_cs, float alpha, float beta, bf16_t* out, int64_t o_cs, int64_t npix,
                              int C, hipStream_t st) {
    if (npix <= 0 || C <= 0) return ctx->fail(SR_ERR_INVALID, "eltwise_views_bf16: empty tensor");
    if (op != SR_ELT_AXPBY && op != SR_ELT_RELU_BWD) return ctx->fail(SR_ERR_INVALID, "eltwise_views_bf16: AXPBY and RELU_BWD only");
    if (op == SR_ELT_RELU_BWD && !b) return ctx->fail(SR_ERR_INVALID, "eltwise_views_bf16: RELU_BWD needs the activation as b");
    const uint16_t* ap = reinterpret_cast<const uint16_t*>(a); const uint16_t* bp = reinterpret_cast<const uint16_t*>(b);
    uint16_t* op_ = reinterpret_cast<uint16_t*>(out);
    if (op == SR_ELT_RELU_BWD) hipLaunchKernelGGL(eltwise_views_bf16_kernel<true>, dim3(grid_n(npix * C)), dim3(256), 0, st, ap, a_cs, bp, b_cs, alpha, beta, op_, o_cs, npix, C);
    else hipLaunchKernelGGL(eltwise_views_bf16_kernel<false>, dim3(grid_n(npix * C)), dim3(256), 0, st, ap, a_cs, bp, b_cs, alpha, beta, op_, o_cs, npix, C);
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
