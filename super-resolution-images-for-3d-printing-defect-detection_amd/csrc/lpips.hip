// lpips.hip -- LPIPS (AlexNet, version 0.1, spatial = False, eval mode) of B image pairs: the dataset EDA's first metric (reference data/EDA.ipynb,
// ImageDatasetAnalyzer.lpips_score) and a perceptual score for SR output that is already on the device.  The contract is stated in include/sr355.h.
//
// One chunk of pairs goes through the trunk as ONE batch of 2 nb images (the a images, then the b images):
//   lpips_input_kernel    uint8 BGR (through the [3][256] fp32 table) or fp32 RGB in [-1, 1] -> the scaled image, shifted by 2 pixels into a zero canvas
//                         and space-to-depth(4)'d: [2 nb, oh + 2, ow + 2, 48], channel (dy 4 + dx) 3 + c.  AlexNet's conv1 (11x11, stride 4, pad 2) is
//                         exactly a 3x3 conv over these 48 channels with the kernel zero-extended to 12x12 and regrouped the same way; output o of the
//                         stride-4 conv is the SAME conv's output at block (o + 1): the interior [1 : 1 + oh, 1 : 1 + ow]
//   conv_launch           conv1 .. conv5 on the fp32 MFMA routes of conv.hip (3x3 / 5x5 wide kernels, bias + ReLU fused, split-K never allowed), with
//                         weights packed once by sr_lpips_set_weights
//   lpips_window_kernel   max-pool 3x3 / stride 2 of a sub-window of an NHWC map (conv1's interior is pooled in place, no copy); with K = S = 1 the same
//                         kernel copies a window (the optional raw taps)
//   lpips_dist_kernel     a tap's two feature maps -> LP_SLICES partial sums per pair of  sum_c l_c (na_c - nb_c)^2,  n = f / (sqrt(sum_c f^2) + 1e-10):
//                         sixteen lanes own a pixel, a lane C / 16 channels; the channel norms of both maps, the weighted squared difference and the
//                         channel sum are formed in registers -- the normalised maps never reach memory
//   lpips_finish_kernel   adds a pair's partial sums in slice order, divides by the map's pixels (the spatial mean) and adds the five terms
// Every sum runs in a fixed order that depends on the map's size only (no atomics): a pair's terms and score are the same bits on every run, for any
// B, at any position in the batch and in whichever chunk it lands.
#include <algorithm>
#include <math.h>

#include "common.h"
#include "fp_sep.h"

namespace {

constexpr int LP_TAPS = 5;
constexpr int LP_C[LP_TAPS] = {64, 192, 384, 256, 256};       // channels of the five taps
constexpr int LP_CIN[LP_TAPS] = {3, 64, 192, 384, 256};
constexpr int LP_K[LP_TAPS] = {11, 5, 3, 3, 3};
constexpr int LP_LIN_TOTAL = 64 + 192 + 384 + 256 + 256;
constexpr int LP_SLICES = 32;                                  // partial sums per (pair, tap)
constexpr int LP_CHUNK_PAIRS = SR_LPIPS_CHUNK_PAIRS;           // pairs per internal chunk, at most
constexpr int64_t LP_WORK_BOUND = SR_LPIPS_WORK_BYTES;         // ... and as many as keep the chunk's maps below this (never fewer than one pair)
// the scaling layer, per R, G, B
__host__ __device__ inline float lp_shift(int c) { return c == 0 ? -.030f : (c == 1 ? -.088f : -.188f); }
__host__ __device__ inline float lp_scale(int c) { return c == 0 ? .458f : (c == 1 ? .448f : .450f); }

struct LpGeom {
    int h[LP_TAPS], w[LP_TAPS];   // the five taps
    int bh, bw;                   // conv1's block image: (oh + 2) x (ow + 2) blocks of 4 x 4 pixels
};

bool lp_geom(int H, int W, LpGeom* g) {
    if (H < 31 || W < 31 || H > 4096 || W > 4096 || (int64_t)H * W > ((int64_t)1 << 22)) return false;
    auto dims = [](int n, int* o) {
        const int c1 = (n - 7) / 4 + 1, p1 = (c1 - 3) / 2 + 1, p2 = (p1 - 3) / 2 + 1;
        o[0] = c1; o[1] = p1; o[2] = o[3] = o[4] = p2;
    };
    dims(H, g->h); dims(W, g->w);
    g->bh = g->h[0] + 2; g->bw = g->w[0] + 2;
    return true;
}

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

// floats of one IMAGE's maps: X0, F1 (block-image sized), P1, F2, P2, F3, F4, F5
struct LpSizes { int64_t x0, f1, p1, f2, p2, f3, f4, f5; int64_t per_image() const { return x0 + f1 + p1 + f2 + p2 + f3 + f4 + f5; } };
LpSizes lp_sizes(const LpGeom& g) {
    const int64_t blk = (int64_t)g.bh * g.bw, m1 = (int64_t)g.h[1] * g.w[1], m2 = (int64_t)g.h[2] * g.w[2];
    return {blk * 48, blk * 64, m1 * 64, m1 * 192, m2 * 192, m2 * 384, m2 * 256, m2 * 256};
}
int lp_chunk_pairs(const LpGeom& g) {
    const int64_t pair_bytes = 2 * 4 * lp_sizes(g).per_image();
    return (int)std::max<int64_t>(1, std::min<int64_t>(LP_CHUNK_PAIRS, LP_WORK_BOUND / pair_bytes));
}

void lp_input_table(float* tab) {
    for (int c = 0; c < 3; ++c)
        for (int v = 0; v < 256; ++v) {
            const double x = 2.0 * ((double)v / 255.0) - 1.0;   // the notebook's to_tensor, in fp64 (2 x is exact: contraction changes nothing)
            const float d = (float)x - lp_shift(c);             // the scaling layer, in fp32, each step rounded
            tab[c * 256 + v] = d / lp_scale(c);
        }
}

// ---------------------------------------------------------------------------------------------------------------------------------------
template <bool U8>
__global__ void __launch_bounds__(256) lpips_input_kernel(const void* __restrict__ a, const void* __restrict__ b, int64_t pair0, int nb, int H, int W, int bh, int bw,
                                                          const float* __restrict__ tab, float* __restrict__ out, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one thread per 4 of the 48 channels of a block
    if (idx >= total) return;
    const int k = (int)(idx % 12);
    int64_t t = idx / 12;
    const int bx = (int)(t % bw); t /= bw;
    const int by = (int)(t % bh);
    const int n = (int)(t / bh);
    const int64_t img = ((n < nb ? pair0 + n : pair0 + n - nb) * H) * (int64_t)W * 3;
    const void* src = n < nb ? a : b;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int ch = 4 * k + e, dy = ch / 12, dx = (ch / 3) & 3, c = ch % 3;
        const int y = by * 4 + dy - 2, x = bx * 4 + dx - 2;
        float s = 0.f;   // the zeros pad the SCALED image
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int64_t o = img + ((int64_t)y * W + x) * 3;
            if (U8) s = tab[c * 256 + static_cast<const uint8_t*>(src)[o + (2 - c)]];        // BGR -> R, G, B
            else s = __fdiv_rn(sub_sep(static_cast<const float*>(src)[o + c], lp_shift(c)), lp_scale(c));
        }
        v[e] = s;
    }
    *reinterpret_cast<f32x4*>(out + idx * 4) = v;
}

// y[n, oy, ox, :] = max over the K x K window at (y0 + oy S, x0 + ox S) of image n of x, an NHWC map of Ws pixels per row.  The host has checked that
// every window lies inside the map.
template <int K, int S>
__global__ void __launch_bounds__(256) lpips_window_kernel(const float* __restrict__ x, int64_t x_img, int Ws, int y0, int x0, int C, int oh, int ow,
                                                           float* __restrict__ y, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;   // one thread per 4 channels of an output pixel
    if (idx >= total) return;
    const int c4 = C >> 2;
    const int c = (int)(idx % c4) * 4;
    int64_t t = idx / c4;
    const int ox = (int)(t % ow); t /= ow;
    const int oy = (int)(t % oh);
    const int64_t n = t / oh;
    const float* p = x + n * x_img + ((int64_t)(y0 + oy * S) * Ws + (x0 + ox * S)) * C + c;
    f32x4 m = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int ky = 0; ky < K; ++ky)
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            if (ky == 0 && kx == 0) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(p + ((int64_t)ky * Ws + kx) * C);
#pragma unroll
            for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
        }
    *reinterpret_cast<f32x4*>(y + idx * 4) = m;
}

__device__ __forceinline__ float group_sum(float v) {   // butterfly over the 16 lanes of a pixel: each of them ends with the same bits
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// f: 2 nb maps of 64 CPL channels (a's, then b's), img floats apart, Ws pixels per row; the tap is their window of w pixels per row, hw pixels in all, at
// (y0, x0) -- conv1's interior is read where it lies.  grid (LP_SLICES, nb); slice s of pair p owns pixels [s per, (s + 1) per), per = ceil(hw / LP_SLICES).
// Sixteen lanes own a pixel, a lane CPL groups of four channels (16-byte loads, a pixel's 256 bytes per group contiguous); a workgroup takes sixteen
// pixels per step, pixel p0 + 16 step + 4 wave + (lane / 16).  part[p][s] = the slice's sum over pixels of sum_c l_c (na_c - nb_c)^2: every lane group adds
// its pixels in step order, the sixteen group sums meet in LDS and are added as a fixed tree.
template <int CPL>
__global__ void __launch_bounds__(256) lpips_dist_kernel(const float* __restrict__ f, int64_t img, int Ws, int y0, int x0, int w, int nb, int hw, const float* __restrict__ lin,
                                                         float* __restrict__ part) {
    constexpr int C = 64 * CPL;
    __shared__ float sm[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l16 = lane & 15, grp = lane >> 4;
    const int s = blockIdx.x, p = blockIdx.y;
    const int per = (hw + LP_SLICES - 1) / LP_SLICES;
    const int p0 = s * per, p1 = min(hw, p0 + per);
    const float* fa = f + (int64_t)p * img;
    const float* fb = f + ((int64_t)nb + p) * img;
    f32x4 l[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) l[j] = *reinterpret_cast<const f32x4*>(lin + (j * 16 + l16) * 4);
    float acc = 0.f;
    for (int q = p0 + wave * 4 + grp; q - (wave * 4 + grp) < p1; q += 16) {   // the trip count is the workgroup's: every lane reaches every shuffle
        const bool live = q < p1;
        const int px = live ? q : p1 - 1;
        const int py = px / w;
        const int64_t o = ((int64_t)(y0 + py) * Ws + (x0 + px - py * w)) * C + l16 * 4;
        f32x4 va[CPL], vb[CPL];
        float sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            va[j] = *reinterpret_cast<const f32x4*>(fa + o + j * 64);
            vb[j] = *reinterpret_cast<const f32x4*>(fb + o + j * 64);
        }
#pragma unroll
        for (int j = 0; j < CPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sa += va[j][e] * va[j][e];
                sb += vb[j][e] * vb[j][e];
            }
        const float da = sqrtf(group_sum(sa)) + 1e-10f, db = sqrtf(group_sum(sb)) + 1e-10f;   // all-zero channels: 0 / 1e-10 = 0, never NaN
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float df = __fdiv_rn(va[j][e], da) - __fdiv_rn(vb[j][e], db);
                d += l[j][e] * (df * df);
            }
        d = group_sum(d);
        acc += live ? d : 0.f;
    }
    if (l16 == 0) sm[wave * 4 + grp] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = (sm[4 * k] + sm[4 * k + 1]) + (sm[4 * k + 2] + sm[4 * k + 3]);
        part[(int64_t)p * LP_SLICES + s] = (t[0] + t[1]) + (t[2] + t[3]);
    }
}

struct LpHw { int hw[LP_TAPS]; };

// part: [LP_TAPS][nb][LP_SLICES].  One thread per pair.
__global__ void lpips_finish_kernel(const float* __restrict__ part, int nb, LpHw g, float* __restrict__ score, float* __restrict__ terms) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nb) return;
    float total = 0.f;
    for (int l = 0; l < LP_TAPS; ++l) {
        const float* q = part + ((int64_t)l * nb + p) * LP_SLICES;
        float t = 0.f;
        for (int s = 0; s < LP_SLICES; ++s) t += q[s];
        t = __fdiv_rn(t, (float)g.hw[l]);
        if (terms) terms[(int64_t)p * LP_TAPS + l] = t;
        total += t;
    }
    score[p] = total;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

struct LpipsState {
    ConvWeights cw[LP_TAPS];
    float* lin = nullptr;   // [LP_LIN_TOTAL], the taps' lin weights one after the other
    float* tab = nullptr;   // [3][256] the uint8 input table
};

static void lpips_unload(sr_ctx* ctx) {
    LpipsState* s = ctx->lpips;
    if (!s) return;
    (void)hipDeviceSynchronize();   // a launch in flight may still read the weights
    for (int l = 0; l < LP_TAPS; ++l) conv_free_weights(ctx, &s->cw[l]);
    ctx->dfree(s->lin);
    ctx->dfree(s->tab);
    if (ctx->lpips_work.p) { ctx->dfree(ctx->lpips_work.p); ctx->lpips_work = sr_ctx::Arena{}; }
    delete s;
    ctx->lpips = nullptr;
}

void lpips_release(sr_ctx* ctx) { lpips_unload(ctx); }

extern "C" {

int sr_lpips_shapes(int H, int W, int (*hw)[2]) {
    LpGeom g;
    if (!hw || !lp_geom(H, W, &g)) return SR_ERR_INVALID;
    for (int l = 0; l < LP_TAPS; ++l) { hw[l][0] = g.h[l]; hw[l][1] = g.w[l]; }
    return SR_OK;
}

int sr_lpips_input_table(float* table_3x256) {
    if (!table_3x256) return SR_ERR_INVALID;
    lp_input_table(table_3x256);
    return SR_OK;
}

int sr_lpips_set_weights(sr_ctx* ctx, const float* const* conv_w, const float* const* conv_b, const float* const* lin_w) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    int given = 0;
    for (int l = 0; l < LP_TAPS; ++l) given += (conv_w && conv_w[l] ? 1 : 0) + (conv_b && conv_b[l] ? 1 : 0) + (lin_w && lin_w[l] ? 1 : 0);
    if (given == 0) { lpips_unload(ctx); return SR_OK; }
    if (given != 3 * LP_TAPS) return ctx->fail(SR_ERR_INVALID, "lpips_set_weights: all fifteen arrays (five conv kernels, five biases, five lin weights) or none");
    lpips_unload(ctx);
    LpipsState* s = new LpipsState();
    ctx->lpips = s;
    int rc = SR_OK;
    {   // conv1: the 11x11x3 kernel zero-extended to 12x12 and regrouped to [3, 3, 48, 64], channel (dy 4 + dx) 3 + c of block (by, bx) = pixel (4 by + dy, 4 bx + dx)
        std::vector<float> w3((size_t)9 * 48 * 64, 0.f);
        for (int ky = 0; ky < 11; ++ky)
            for (int kx = 0; kx < 11; ++kx)
                for (int c = 0; c < 3; ++c) {
                    const size_t dst = ((size_t)((ky / 4) * 3 + kx / 4) * 48 + ((ky % 4) * 4 + kx % 4) * 3 + c) * 64;
                    memcpy(&w3[dst], conv_w[0] + ((size_t)(ky * 11 + kx) * 3 + c) * 64, sizeof(float) * 64);
                }
        rc = conv_pack_weights(ctx, w3.data(), conv_b[0], 3, 48, 64, SR_DTYPE_F32, &s->cw[0]);
    }
    for (int l = 1; l < LP_TAPS && rc == SR_OK; ++l) rc = conv_pack_weights(ctx, conv_w[l], conv_b[l], LP_K[l], LP_CIN[l], LP_C[l], SR_DTYPE_F32, &s->cw[l]);
    if (rc == SR_OK) {
        float tab[768];
        lp_input_table(tab);
        s->lin = static_cast<float*>(ctx->dalloc(sizeof(float) * LP_LIN_TOTAL));
        s->tab = static_cast<float*>(ctx->dalloc(sizeof tab));
        if (!s->lin || !s->tab) rc = SR_ERR_OOM;
        int off = 0;
        for (int l = 0; l < LP_TAPS && rc == SR_OK; ++l) {
            if (hipMemcpy(s->lin + off, lin_w[l], sizeof(float) * LP_C[l], hipMemcpyHostToDevice) != hipSuccess) rc = ctx->fail(SR_ERR_HIP, "lpips_set_weights: upload failed");
            off += LP_C[l];
        }
        if (rc == SR_OK && hipMemcpy(s->tab, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) rc = ctx->fail(SR_ERR_HIP, "lpips_set_weights: upload failed");
    }
    if (rc != SR_OK) {
        const std::string msg = ctx->err;
        lpips_unload(ctx);
        ctx->err = msg;
    }
    return rc;
}

int sr_lpips(sr_ctx* ctx, const void* a, const void* b, int dtype, int B, int H, int W, float* score_B, float* terms_Bx5, float* const* taps, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!a || !b || !score_B) return ctx->fail(SR_ERR_INVALID, "lpips: null tensor");
    if (dtype != SR_DTYPE_U8 && dtype != SR_DTYPE_F32) return ctx->fail(SR_ERR_INVALID, "lpips: images are uint8 BGR or float32 RGB in [-1, 1]");
    LpGeom g;
    if (B < 1 || B > (1 << 20) || !lp_geom(H, W, &g))
        return ctx->fail(SR_ERR_INVALID, "lpips: 1 <= B <= 2^20, 31 <= H, W <= 4096 and H * W <= 2^22 (got B " + std::to_string(B) + ", " + std::to_string(H) + " x " +
                                             std::to_string(W) + ")");
    if (dtype == SR_DTYPE_F32 && (((uintptr_t)a | (uintptr_t)b) & 3)) return ctx->fail(SR_ERR_INVALID, "lpips: float images must be 4-byte aligned");
    for (int l = 0; taps && l < LP_TAPS; ++l)
        if (taps[l] && ((uintptr_t)taps[l] & 15)) return ctx->fail(SR_ERR_INVALID, "lpips: tap buffers must be 16-byte aligned");
    const LpipsState* s = ctx->lpips;
    if (!s) return ctx->fail(SR_ERR_STATE, "lpips: the weights are not set (sr_lpips_set_weights)");
    hipStream_t st = static_cast<hipStream_t>(stream);

    const LpSizes z = lp_sizes(g);
    const int nbmax = std::min(B, lp_chunk_pairs(g));
    const int64_t nimg = 2 * (int64_t)nbmax;
    const int64_t fl[8] = {z.x0, z.f1, z.p1, z.f2, z.p2, z.f3, z.f4, z.f5};
    size_t off[9], total = 0;
    for (int i = 0; i < 8; ++i) { off[i] = total; total += al256(sizeof(float) * (size_t)(fl[i] * nimg)); }
    off[8] = total;
    total += al256(sizeof(float) * (size_t)LP_TAPS * nbmax * LP_SLICES);
    if (total > ctx->lpips_work.cap) {   // exact, not sr_ctx::arena's growth with slack: the bound the header states is the allocation's
        if (ctx->lpips_work.p) { SR_HIP(ctx, hipStreamSynchronize(st)); ctx->dfree(ctx->lpips_work.p); ctx->lpips_work = sr_ctx::Arena{}; }
        ctx->lpips_work.p = ctx->dalloc(total);
        if (!ctx->lpips_work.p) return SR_ERR_OOM;
        ctx->lpips_work.cap = total;
    }
    char* wk = static_cast<char*>(ctx->lpips_work.p);
    float* buf[8];
    for (int i = 0; i < 8; ++i) buf[i] = reinterpret_cast<float*>(wk + off[i]);
    float* X0 = buf[0]; float* F1 = buf[1]; float* P1 = buf[2]; float* F2 = buf[3]; float* P2 = buf[4];
    float* part = reinterpret_cast<float*>(wk + off[8]);
    // the buffer tap l lives in (tap 1 inside conv1's bordered output)
    float* const tapbuf[LP_TAPS] = {F1, F2, buf[5], buf[6], buf[7]};

    ConvEpilogue ep;
    ep.act = SR_ACT_RELU;       // allow_splitk stays 0: another summation order would make the bits depend on the batch
    LpHw hws;
    for (int l = 0; l < LP_TAPS; ++l) hws.hw[l] = g.h[l] * g.w[l];

    for (int pair0 = 0; pair0 < B; pair0 += nbmax) {
        const int nb = std::min(nbmax, B - pair0), N = 2 * nb;
        {
            const int64_t n = (int64_t)N * g.bh * g.bw * 12;
            if (dtype == SR_DTYPE_U8)
                hipLaunchKernelGGL(lpips_input_kernel<true>, dim3(blocks_of(n)), dim3(256), 0, st, a, b, (int64_t)pair0, nb, H, W, g.bh, g.bw, s->tab, X0, n);
            else
                hipLaunchKernelGGL(lpips_input_kernel<false>, dim3(blocks_of(n)), dim3(256), 0, st, a, b, (int64_t)pair0, nb, H, W, g.bh, g.bw, s->tab, X0, n);
        }
        // conv1 on the block image; tap 1 is the interior [1 : 1 + h0, 1 : 1 + w0] of F1
        if (int rc = conv_launch(ctx, s->cw[0], TensorView{X0, 48, 0}, N, g.bh, g.bw, F1, 64, 0, ep, st)) return rc;
        {
            const int64_t n = (int64_t)N * g.h[1] * g.w[1] * (64 / 4);
            hipLaunchKernelGGL((lpips_window_kernel<3, 2>), dim3(blocks_of(n)), dim3(256), 0, st, F1, (int64_t)g.bh * g.bw * 64, g.bw, 1, 1, 64, g.h[1], g.w[1], P1, n);
        }
        if (int rc = conv_launch(ctx, s->cw[1], TensorView{P1, 64, 0}, N, g.h[1], g.w[1], F2, 192, 0, ep, st)) return rc;
        {
            const int64_t n = (int64_t)N * g.h[2] * g.w[2] * (192 / 4);
            hipLaunchKernelGGL((lpips_window_kernel<3, 2>), dim3(blocks_of(n)), dim3(256), 0, st, F2, (int64_t)g.h[1] * g.w[1] * 192, g.w[1], 0, 0, 192, g.h[2], g.w[2], P2, n);
        }
        if (int rc = conv_launch(ctx, s->cw[2], TensorView{P2, 192, 0}, N, g.h[2], g.w[2], buf[5], 384, 0, ep, st)) return rc;
        if (int rc = conv_launch(ctx, s->cw[3], TensorView{buf[5], 384, 0}, N, g.h[2], g.w[2], buf[6], 256, 0, ep, st)) return rc;
        if (int rc = conv_launch(ctx, s->cw[4], TensorView{buf[6], 256, 0}, N, g.h[2], g.w[2], buf[7], 256, 0, ep, st)) return rc;

        int loff = 0;
        for (int l = 0; l < LP_TAPS; ++l) {
            const int C = LP_C[l], hw = hws.hw[l];
            const float* f = tapbuf[l];
            // conv1's tap is the interior of its block-image-sized output; the others are dense
            const int64_t img = l == 0 ? (int64_t)g.bh * g.bw * 64 : (int64_t)hw * C;
            const int Ws = l == 0 ? g.bw : g.w[l], org = l == 0 ? 1 : 0;
            if (taps && taps[l]) {   // [2, B, h, w, C]: a's maps of this chunk, then b's
                const int64_t n = (int64_t)nb * hw * (C / 4);
                for (int half = 0; half < 2; ++half)
                    hipLaunchKernelGGL((lpips_window_kernel<1, 1>), dim3(blocks_of(n)), dim3(256), 0, st, f + (int64_t)half * nb * img, img, Ws, org, org, C, g.h[l], g.w[l],
                                       taps[l] + ((int64_t)half * B + pair0) * hw * C, n);
            }
            float* pl = part + (int64_t)l * nb * LP_SLICES;
            const dim3 grid(LP_SLICES, (unsigned)nb);
            switch (C / 64) {
                case 1: hipLaunchKernelGGL(lpips_dist_kernel<1>, grid, dim3(256), 0, st, f, img, Ws, org, org, g.w[l], nb, hw, s->lin + loff, pl); break;
                case 3: hipLaunchKernelGGL(lpips_dist_kernel<3>, grid, dim3(256), 0, st, f, img, Ws, org, org, g.w[l], nb, hw, s->lin + loff, pl); break;
                case 4: hipLaunchKernelGGL(lpips_dist_kernel<4>, grid, dim3(256), 0, st, f, img, Ws, org, org, g.w[l], nb, hw, s->lin + loff, pl); break;
                default: hipLaunchKernelGGL(lpips_dist_kernel<6>, grid, dim3(256), 0, st, f, img, Ws, org, org, g.w[l], nb, hw, s->lin + loff, pl); break;
            }
            loff += C;
        }
        hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0, st, part, nb, hws, score_B + pair0,
                           terms_Bx5 ? terms_Bx5 + (int64_t)pair0 * LP_TAPS : nullptr);
        SR_HIP(ctx, hipGetLastError());
    }
    return SR_OK;
}

}  // extern "C"
