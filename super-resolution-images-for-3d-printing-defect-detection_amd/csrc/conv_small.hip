// conv_small.hip -- 3x3 SAME stride-1 bf16 conv over MANY SMALL images with hundreds of channels (VGG19 blocks 4-5 on training patches: 6 x 6 and 3 x 3
// pixels, 512 channels; the kernel takes up to 144 pixels, the trainer's rule gan_train.small_conv_wins keeps it where it measured fastest; ESRGAN_model.py:379-408, 514-524).  gfx950 only.  DESIGN.md 3.29.
//
// Formulation.  An implicit GEMM D^T[cout][pixel] += W^T[cout][k] * X^T[k][pixel] on v_mfma_f32_16x16x32_bf16 whose pixel axis runs over the pixels of ALL images
// together (M = B * H * W): a workgroup owns 64 consecutive pixels x 32 couts, and the 64 pixels may lie in any number of images.  K = 9 taps x Cin runs in steps of one
// tap x 32 channels, s = tap * (Cin / 32) + chunk.  The workgroup's four waves split the STEPS, wave w taking [w S / 4, (w + 1) S / 4): each wave holds the whole
// 64 x 32 tile (8 accumulators of 16 x 16) for its quarter of K, so that no operand is fetched twice inside the workgroup, and the four partial tiles meet in LDS
// and are added in the fixed order ((w0 + w1) + w2) + w3 by the epilogue.  The split depends on Cin alone: an image's bits depend neither on B nor on where the
// image stands in the batch.  Nothing waits on another workgroup; there are no atomics and no second launch.
//
// Operands.  A (weights): packed once by conv_small_pack_kernel into fragment order [cout / 16][step][lane][8], so that a lane's fragment is one 16-byte load.
// B (pixels): lane l of a 16-pixel block reads channels 32 c + 8 (l >> 4) .. + 8 of the tap's pixel of column l & 15 straight from NHWC, one 16-byte load.  A tap
// that falls outside ITS OWN image (or a column beyond M) is a zero fragment that is never loaded: no other image's pixel is read, and nothing is multiplied by a
// zero weight.  Loads run SMALL_DEPTH steps ahead of the MFMAs in registers.
//
// Epilogue, all fp32: sum of the four partials + bias, ReLU or nothing, ONE round to nearest even, then the optional select on the rounded bits: +0 where
// mask <= 0 (the predicate of sr_relu_bwd_bf16).
//
// Grid: one workgroup per tile, ceil(M / 64) x Cout / 32, no cap and no tile loop; the launcher refuses M >= 2^31 - 64 and Cout / 32 > 65535.
#include "common.h"

namespace {

constexpr int SMALL_TM = 64;                        // pixels per workgroup
constexpr int SMALL_TN = 32;                        // couts per workgroup
constexpr int SMALL_WAVES = 4;                      // K-split inside the workgroup
constexpr int SMALL_ROW = SMALL_TN + 4;             // floats per pixel of a partial tile in LDS (16-byte aligned rows, 4 floats of skew)
constexpr int SMALL_LDS = SMALL_WAVES * SMALL_TM * SMALL_ROW * 4;
constexpr int SMALL_DEPTH = 4;                      // steps whose operands are in flight
constexpr int SMALL_MAX_HW = 144;                   // include/sr355.h

__device__ __forceinline__ uint16_t small_bf16_rne(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// One thread per lane fragment (8 consecutive cins of one cout of one step): dst [Cout / 16][S][64][8] bf16.  rot = 0: src HWIO [3,3,Cin,Cout].  rot = 1: src is the
// forward kernel [3,3,Cout,Cin] of the layer whose input gradient is wanted; the packed kernel is its 180-degree rotation with the channel axes swapped.
__global__ void __launch_bounds__(256) conv_small_pack_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, int Cin, int Cout, int rot, int64_t nfrag) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= nfrag) return;
    const int nch = Cin / 32, S = 9 * nch;
    const int lane = (int)(f & 63);
    const int64_t r = f >> 6;
    const int s = (int)(r % S), cb = (int)(r / S);
    const int tap = s / nch, c = s - tap * nch;
    const int co = cb * 16 + (lane & 15), ci0 = c * 32 + 8 * (lane >> 4);
    uint16_t v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = ci0 + j;
        const float w = rot ? src[((int64_t)(8 - tap) * Cout + co) * Cin + ci] : src[((int64_t)tap * Cin + ci) * Cout + co];
        v[j] = small_bf16_rne(w);
    }
    uint4 o;
    o.x = v[0] | ((uint32_t)v[1] << 16); o.y = v[2] | ((uint32_t)v[3] << 16); o.z = v[4] | ((uint32_t)v[5] << 16); o.w = v[6] | ((uint32_t)v[7] << 16);
    reinterpret_cast<uint4*>(dst)[f] = o;
}

struct SmallParams {
    const uint16_t* x; const uint16_t* w; const float* bias; const uint16_t* mask; uint16_t* y;
    int M, H, W, Cin, Cout, nch, act;
};

struct SmallFrags { bf16x8 a[2]; bf16x8 b[4]; };

__global__ void __launch_bounds__(256) conv_small_kernel(SmallParams p) {
    extern __shared__ float small_part[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m0 = blockIdx.x * SMALL_TM, cb0 = blockIdx.y * 2;
    const int S = 9 * p.nch;
    const int s_lo = wave * S / SMALL_WAVES, s_hi = (wave + 1) * S / SMALL_WAVES;

    // the lane's pixel in each 16-pixel block: its element offset in x (plus the lane's 8-channel slice) and the taps that stay inside its image
    int64_t pbase[4];
    uint32_t pvalid[4];
    const int hw = p.H * p.W;
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) {
        const int m = m0 + pb * 16 + (lane & 15);
        uint32_t vm = 0;
        if (m < p.M) {
            const int r = m % hw, py = r / p.W, px = r - py * p.W;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = py + t / 3 - 1, xx = px + t % 3 - 1;
                if (yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) vm |= 1u << t;
            }
        }
        pvalid[pb] = vm;
        pbase[pb] = (int64_t)m * p.Cin + 8 * (lane >> 4);
    }
    const bf16x8* __restrict__ wf = reinterpret_cast<const bf16x8*>(p.w) + lane;
    const int64_t wrow0 = (int64_t)cb0 * S * 64, wrow1 = (int64_t)(cb0 + 1) * S * 64;
    const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    // the load cursor: step ls = ltap * nch + lc
    int ls = s_lo, ltap = s_lo / p.nch, lc = s_lo - ltap * p.nch;
    auto load = [&](SmallFrags& f) {
        if (ls < s_hi) {
            f.a[0] = wf[wrow0 + (int64_t)ls * 64];
            f.a[1] = wf[wrow1 + (int64_t)ls * 64];
            const int64_t doff = (int64_t)((ltap / 3 - 1) * p.W + (ltap % 3 - 1)) * p.Cin + lc * 32;
#pragma unroll
            for (int pb = 0; pb < 4; ++pb) {
                f.b[pb] = zero;
                if ((pvalid[pb] >> ltap) & 1u) f.b[pb] = *reinterpret_cast<const bf16x8*>(p.x + pbase[pb] + doff);
            }
        } else {
            f.a[0] = zero; f.a[1] = zero;
#pragma unroll
            for (int pb = 0; pb < 4; ++pb) f.b[pb] = zero;
        }
        ++ls;
        if (++lc == p.nch) { lc = 0; ++ltap; }
    };

    f32x4 acc[4][2];
#pragma unroll
    for (int pb = 0; pb < 4; ++pb) { acc[pb][0] = f32x4{0.f, 0.f, 0.f, 0.f}; acc[pb][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    SmallFrags fr[SMALL_DEPTH];
#pragma unroll
    for (int d = 0; d < SMALL_DEPTH; ++d) load(fr[d]);
    for (int s = s_lo; s < s_hi; s += SMALL_DEPTH) {
#pragma unroll
        for (int d = 0; d < SMALL_DEPTH; ++d) {                   // a step beyond s_hi carries zero fragments: it adds +0
#pragma unroll
            for (int pb = 0; pb < 4; ++pb) {
                acc[pb][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[d].a[0], fr[d].b[pb], acc[pb][0], 0, 0, 0);
                acc[pb][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fr[d].a[1], fr[d].b[pb], acc[pb][1], 0, 0, 0);
            }
            load(fr[d]);
        }
    }

    // D: column (lane & 15) = pixel, rows 4 (lane >> 4) + i = cout
#pragma unroll
    for (int pb = 0; pb < 4; ++pb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
            *reinterpret_cast<f32x4*>(&small_part[(wave * SMALL_TM + pb * 16 + (lane & 15)) * SMALL_ROW + cb * 16 + 4 * (lane >> 4)]) = acc[pb][cb];
    __syncthreads();

    const int pix = tid >> 2, q = tid & 3;
    const int m = m0 + pix;
    if (m >= p.M) return;
    const int co = blockIdx.y * SMALL_TN + q * 8;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        f32x4 t = *reinterpret_cast<const f32x4*>(&small_part[pix * SMALL_ROW + q * 8 + 4 * h]);
#pragma unroll
        for (int w = 1; w < SMALL_WAVES; ++w) t += *reinterpret_cast<const f32x4*>(&small_part[(w * SMALL_TM + pix) * SMALL_ROW + q * 8 + 4 * h]);
        v[4 * h] = t[0]; v[4 * h + 1] = t[1]; v[4 * h + 2] = t[2]; v[4 * h + 3] = t[3];
    }
    const int64_t o = (int64_t)m * p.Cout + co;
    uint4 mk = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
    if (p.mask) mk = *reinterpret_cast<const uint4*>(p.mask + o);
    const uint32_t mw[4] = {mk.x, mk.y, mk.z, mk.w};
    uint32_t ow[4];
    const float slope = p.act == SR_ACT_RELU ? 0.f : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float r = v[j] + (p.bias ? p.bias[co + j] : 0.f);
        r = fmaxf(r, r * slope);                                            // conv_rows_epi.h's activation, so that the two kernels agree on the sign of a ReLU'd zero
        uint32_t bits = small_bf16_rne(r);
        const uint32_t mb = (mw[j >> 1] >> (16 * (j & 1))) & 0xffffu, mag = mb & 0x7fffu;
        if ((mb & 0x8000u) || mag == 0 || mag > 0x7f80u) bits = 0;           // mask > 0 read off the bits, as sr_relu_bwd_bf16 reads it
        if (j & 1) ow[j >> 1] |= bits << 16; else ow[j >> 1] = bits;
    }
    *reinterpret_cast<uint4*>(p.y + o) = uint4{ow[0], ow[1], ow[2], ow[3]};
}

int small_check_channels(sr_ctx* ctx, int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0 || Cin % 32 != 0 || Cout % 32 != 0)
        return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: Cin and Cout must be positive multiples of 32, got " + std::to_string(Cin) + " and " + std::to_string(Cout));
    if (Cout / SMALL_TN > 65535) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: at most 65535 * 32 output channels");
    return SR_OK;
}

int small_pack_launch(sr_ctx* ctx, const float* d_w, int Cin, int Cout, int rot, void* packed, hipStream_t st) {
    const int64_t nfrag = (int64_t)9 * Cin * Cout / 8;
    const int64_t blocks = (nfrag + 255) / 256;
    if (blocks >= (1ll << 31)) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: kernel too large to pack in one launch");
    int rec = -1;
    if (ctx->prof) rec = ctx->prof_open("conv_small_pack<bf16>", 0.0, (double)nfrag * 8 * 6.0, st);
    hipLaunchKernelGGL(conv_small_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_w, static_cast<uint16_t*>(packed), Cin, Cout, rot ? 1 : 0, nfrag);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // namespace

int64_t sr_conv3x3_small_pack_bytes(int Cin, int Cout) {
    if (Cin <= 0 || Cout <= 0 || Cin % 32 != 0 || Cout % 32 != 0) return 0;
    return (int64_t)9 * Cin * Cout * 2;
}

int sr_conv3x3_small_pack_bf16(sr_ctx* ctx, const float* d_w, int Cin, int Cout, int rot, void* packed, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!d_w || !packed) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (int rc = small_check_channels(ctx, Cin, Cout)) return rc;
    if (((uintptr_t)packed % 16) != 0) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: the packed kernel must be 16-byte aligned");
    return small_pack_launch(ctx, d_w, Cin, Cout, rot, packed, static_cast<hipStream_t>(stream));
}

int sr_conv3x3_small_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int Cin, const float* d_w, const void* packed, const float* d_bias, int Cout, int rot, int act,
                          const void* mask, void* y, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!x || !y || (!d_w && !packed)) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (B <= 0 || H <= 0 || W <= 0) return ctx->fail(SR_ERR_INVALID, "bad tensor shape");
    if (int rc = small_check_channels(ctx, Cin, Cout)) return rc;
    if ((int64_t)H * W > SMALL_MAX_HW)
        return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: images of at most " + std::to_string(SMALL_MAX_HW) + " pixels, got " + std::to_string(H) + " x " + std::to_string(W));
    if (act != SR_ACT_LINEAR && act != SR_ACT_RELU) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: the activation is linear or ReLU");
    const int64_t M = (int64_t)B * H * W;
    if (M >= (1ll << 31) - SMALL_TM) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: too many pixels for one launch");
    for (const void* q : {x, (const void*)y, mask, packed})
        if (q && ((uintptr_t)q % 16) != 0) return ctx->fail(SR_ERR_INVALID, "conv3x3_small_bf16: tensors must be 16-byte aligned");
    const void* wp = packed;
    if (!wp) {                                                   // no handle: round the fp32 kernel now, into the context's arena (stream-ordered reuse)
        void* a = ctx->arena(ctx->small_w, (size_t)sr_conv3x3_small_pack_bytes(Cin, Cout), st);
        if (!a) return SR_ERR_OOM;
        if (int rc = small_pack_launch(ctx, d_w, Cin, Cout, rot, a, st)) return rc;
        wp = a;
    }
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&conv_small_kernel), SMALL_LDS)) return rc;
    SmallParams p;
    p.x = static_cast<const uint16_t*>(x); p.w = static_cast<const uint16_t*>(wp); p.bias = d_bias; p.mask = static_cast<const uint16_t*>(mask);
    p.y = static_cast<uint16_t*>(y);
    p.M = (int)M; p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.nch = Cin / 32; p.act = act;
    const dim3 grid((unsigned)((M + SMALL_TM - 1) / SMALL_TM), (unsigned)(Cout / SMALL_TN));
    int rec = -1;
    if (ctx->prof) rec = ctx->prof_open("conv_small<bf16,k3,64x32,ks4>", 2.0 * M * 9.0 * Cin * Cout, 2.0 * (M * ((double)Cin + Cout) + 9.0 * Cin * Cout), st);
    hipLaunchKernelGGL(conv_small_kernel, grid, dim3(256), SMALL_LDS, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

// =================================================================================================
// The perceptual branch's other kernels (include/sr355.h).  bf16 values travel as their 16 bits: a select cannot round.  Every kernel here runs one
// thread per element (or per 8 channels) on an exact grid -- no cap, no grid-stride loop; a launcher refuses a tensor that needs 2^31 workgroups or more.
// =================================================================================================
namespace {

__device__ __forceinline__ float small_bits_f32(uint32_t v) { return __uint_as_float(v << 16); }
// > 0 read off the bits: sign clear, not zero, not NaN (sr_relu_bwd_bf16's predicate)
__device__ __forceinline__ bool small_positive(uint32_t v) { const uint32_t mag = v & 0x7fffu; return !(v & 0x8000u) && mag != 0 && mag <= 0x7f80u; }

// [fake | hr] fp32 RGB in [-1, 1] -> bf16 [2 npix, 6]: v = (x + 1) * 127.5 - mean in BGR order, vgg_preproc_kernel's expression; hi = bf16(v) in channels 0-2,
// lo = bf16(v - hi) in 3-5 (v - hi is exact in fp32: hi is v's own rounding)
__global__ void __launch_bounds__(256) vgg_preprocess_bf16_kernel(const float* __restrict__ fake, const float* __restrict__ hr, int64_t npix, uint16_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * npix * 3) return;
    const int c = (int)(i % 3);
    const int64_t p = i / 3;
    const float* src = p < npix ? fake : hr;
    const int64_t q = p < npix ? p : p - npix;
    const float mean = c == 0 ? 103.939f : (c == 1 ? 116.779f : 123.68f);
    const float v = (src[q * 3 + (2 - c)] + 1.f) * 127.5f - mean;
    const uint16_t hi = small_bf16_rne(v);
    out[p * 6 + c] = hi;
    out[p * 6 + 3 + c] = small_bf16_rne(v - small_bits_f32(hi));      // (a difference of two stored values: nothing here can fuse)
}

// the bf16 gradient of v [npix, 3] -> the fp32 gradient of the RGB input in [-1, 1]: channels flipped back, times 127.5
__global__ void __launch_bounds__(256) vgg_preprocess_bwd_kernel(const uint16_t* __restrict__ dv, int64_t n, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % 3);
    out[i] = 127.5f * small_bits_f32(dv[i - c + (2 - c)]);
}

// The 2x2 window of output pixel (oy, ox), 8 channels: the winner is the first of v00, v01, v10, v11 that equals the maximum (maxpool2_bwd_kernel's order and tie rule).
struct PoolWin { uint4 v[4]; };
__device__ __forceinline__ uint32_t lane16(const uint4& q, int j) { const uint32_t w = j < 2 ? q.x : (j < 4 ? q.y : (j < 6 ? q.z : q.w)); return (w >> (16 * (j & 1))) & 0xffffu; }
__device__ __forceinline__ int pool_arg(const PoolWin& w, int j) {
    const float v00 = small_bits_f32(lane16(w.v[0], j)), v01 = small_bits_f32(lane16(w.v[1], j)), v10 = small_bits_f32(lane16(w.v[2], j)), v11 = small_bits_f32(lane16(w.v[3], j));
    const float m = fmaxf(fmaxf(v00, v01), fmaxf(v10, v11));
    return v00 == m ? 0 : (v01 == m ? 1 : (v10 == m ? 2 : 3));
}
__device__ __forceinline__ uint32_t pool_pick(const PoolWin& w, int a, int j) {      // (a chain of selects: an index into w.v would put the window in scratch)
    return a == 0 ? lane16(w.v[0], j) : (a == 1 ? lane16(w.v[1], j) : (a == 2 ? lane16(w.v[2], j) : lane16(w.v[3], j)));
}
__device__ __forceinline__ PoolWin pool_load(const uint16_t* __restrict__ x, int64_t b, int oy, int ox, int c, int H, int W, int C) {
    const uint16_t* base = x + ((b * H + 2 * oy) * W + 2 * ox) * C + c;
    PoolWin w;
    w.v[0] = *reinterpret_cast<const uint4*>(base); w.v[1] = *reinterpret_cast<const uint4*>(base + C);
    w.v[2] = *reinterpret_cast<const uint4*>(base + (int64_t)W * C); w.v[3] = *reinterpret_cast<const uint4*>(base + (int64_t)W * C + C);
    return w;
}
__device__ __forceinline__ uint4 pack8(const uint32_t* o) { return uint4{o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16)}; }

__global__ void __launch_bounds__(256) maxpool2_bf16_kernel(const uint16_t* __restrict__ x, int B, int H, int W, int C, uint16_t* __restrict__ y) {
    const int oH = H / 2, oW = W / 2, Cv = C / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * oH * oW * Cv) return;
    const int c = (int)(i % Cv) * 8;
    int64_t t = i / Cv;
    const int ox = (int)(t % oW); t /= oW;
    const int oy = (int)(t % oH);
    const int64_t b = t / oH;
    const PoolWin w = pool_load(x, b, oy, ox, c, H, W, C);
    uint32_t o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = pool_pick(w, pool_arg(w, j), j);
    *reinterpret_cast<uint4*>(y + ((b * oH + oy) * oW + ox) * C + c) = pack8(o);
}

// dx = dy of the window where the element is the window's winner AND x > 0 (the ReLU of the conv in front of the pool), else +0; a row / column the pool dropped: +0
__global__ void __launch_bounds__(256) maxpool2_bwd_bf16_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ dy, int B, int H, int W, int C, uint16_t* __restrict__ dx) {
    const int oH = H / 2, oW = W / 2, Cv = C / 8;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * H * W * Cv) return;
    const int c = (int)(i % Cv) * 8;
    int64_t t = i / Cv;
    const int xq = (int)(t % W); t /= W;
    const int yq = (int)(t % H);
    const int64_t b = t / H;
    const int oy = yq >> 1, ox = xq >> 1, me = (yq & 1) * 2 + (xq & 1);
    uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (oy < oH && ox < oW) {
        const PoolWin w = pool_load(x, b, oy, ox, c, H, W, C);
        const uint4 g = *reinterpret_cast<const uint4*>(dy + ((b * oH + oy) * oW + ox) * C + c);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (pool_arg(w, j) == me && small_positive(pool_pick(w, me, j))) o[j] = lane16(g, j);
    }
    *reinterpret_cast<uint4*>(dx + ((b * H + yq) * W + xq) * C + c) = pack8(o);
}

// feats = [ff | fr], n elements each: the fp64 partial sums of (ff - fr)^2 (block-strided, a fixed tree) and dff = bf16(c * (ff - fr)) where ff > 0, else +0
constexpr int MSE_GRAD_MAX_BLOCKS = 1024;
__global__ void __launch_bounds__(256) mse_grad_bf16_kernel(const uint16_t* __restrict__ feats, int64_t n, float c, uint16_t* __restrict__ dff, double* __restrict__ partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint32_t fb = feats[i];
        const float ff = small_bits_f32(fb), fr = small_bits_f32(feats[n + i]);
        const double d = (double)ff - (double)fr;              // exact
        s += d * d;                                            // (fp64, held to fp32's rounding of the mean: fused or not is far below it)
        dff[i] = small_positive(fb) ? small_bf16_rne(c * (ff - fr)) : (uint16_t)0;      // a difference, then a product: two roundings, no sum for a product to fuse into
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
__global__ void mse_grad_finish_kernel(const double* __restrict__ partial, int nblk, double n, float* __restrict__ loss) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < nblk; ++b) s += partial[b];
        loss[0] = (float)(s / n);
    }
}

int exact_grid(sr_ctx* ctx, int64_t threads, const char* what, unsigned* blocks) {
    const int64_t g = (threads + 255) / 256;
    if (threads <= 0) return ctx->fail(SR_ERR_INVALID, std::string(what) + ": empty tensor");
    if (g >= (1ll << 31)) return ctx->fail(SR_ERR_INVALID, std::string(what) + ": too many elements for one launch");
    *blocks = (unsigned)g;
    return SR_OK;
}
bool aligned16(std::initializer_list<const void*> ps) { for (const void* q : ps) if (((uintptr_t)q % 16) != 0) return false; return true; }

}  // namespace

int sr_vgg_preprocess_bf16(sr_ctx* ctx, const float* fake, const float* hr, int B, int H, int W, void* out, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!fake || !hr || !out) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (B <= 0 || H <= 0 || W <= 0) return ctx->fail(SR_ERR_INVALID, "vgg_preprocess_bf16: bad shape");
    const int64_t npix = (int64_t)B * H * W;
    unsigned blocks;
    if (int rc = exact_grid(ctx, 2 * npix * 3, "vgg_preprocess_bf16", &blocks)) return rc;
    hipLaunchKernelGGL(vgg_preprocess_bf16_kernel, dim3(blocks), dim3(256), 0, st, fake, hr, npix, static_cast<uint16_t*>(out));
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_vgg_preprocess_bwd(sr_ctx* ctx, const void* dv, int64_t npix, float* dfake, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!dv || !dfake) return ctx->fail(SR_ERR_INVALID, "null tensor");
    unsigned blocks;
    if (int rc = exact_grid(ctx, npix > 0 ? npix * 3 : 0, "vgg_preprocess_bwd", &blocks)) return rc;
    hipLaunchKernelGGL(vgg_preprocess_bwd_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(dv), npix * 3, dfake);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_maxpool2_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int C, void* y, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (B <= 0 || H < 2 || W < 2 || C <= 0 || C % 8 != 0) return ctx->fail(SR_ERR_INVALID, "maxpool2_bf16: images of at least 2 x 2 pixels, channels a multiple of 8");
    if (!x || !y) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (!aligned16({x, y})) return ctx->fail(SR_ERR_INVALID, "maxpool2_bf16: tensors must be 16-byte aligned");
    unsigned blocks;
    if (int rc = exact_grid(ctx, (int64_t)B * (H / 2) * (W / 2) * (C / 8), "maxpool2_bf16", &blocks)) return rc;
    hipLaunchKernelGGL(maxpool2_bf16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x), B, H, W, C, static_cast<uint16_t*>(y));
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_maxpool2_bwd_bf16(sr_ctx* ctx, const void* x, const void* dy, int B, int H, int W, int C, void* dx, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (B <= 0 || H < 2 || W < 2 || C <= 0 || C % 8 != 0) return ctx->fail(SR_ERR_INVALID, "maxpool2_bwd_bf16: images of at least 2 x 2 pixels, channels a multiple of 8");
    if (!x || !dy || !dx) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (!aligned16({x, dy, (const void*)dx})) return ctx->fail(SR_ERR_INVALID, "maxpool2_bwd_bf16: tensors must be 16-byte aligned");
    unsigned blocks;
    if (int rc = exact_grid(ctx, (int64_t)B * H * W * (C / 8), "maxpool2_bwd_bf16", &blocks)) return rc;
    hipLaunchKernelGGL(maxpool2_bwd_bf16_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t*>(x), static_cast<const uint16_t*>(dy),
                       B, H, W, C, static_cast<uint16_t*>(dx));
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_mse_grad_bf16(sr_ctx* ctx, const void* feats, int64_t n, float* perc1, void* dff, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!feats || !perc1 || !dff) return ctx->fail(SR_ERR_INVALID, "null tensor");
    if (n <= 0) return ctx->fail(SR_ERR_INVALID, "mse_grad_bf16: empty tensor");
    const int64_t want = (n + 255) / 256;
    const int nblk = (int)(want > MSE_GRAD_MAX_BLOCKS ? MSE_GRAD_MAX_BLOCKS : want);
    double* partial = static_cast<double*>(ctx->scratch(sizeof(double) * MSE_GRAD_MAX_BLOCKS));
    if (!partial) return SR_ERR_OOM;
    hipLaunchKernelGGL(mse_grad_bf16_kernel, dim3(nblk), dim3(256), 0, st, static_cast<const uint16_t*>(feats), n, (float)(2.0 / (double)n), static_cast<uint16_t*>(dff), partial);
    hipLaunchKernelGGL(mse_grad_finish_kernel, dim3(1), dim3(64), 0, st, partial, nblk, (double)n, perc1);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
