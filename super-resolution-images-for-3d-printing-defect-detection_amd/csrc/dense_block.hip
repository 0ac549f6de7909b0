// dense_block.hip -- a whole ESRGAN dense block at 8 growth channels as ONE kernel whose concat tensor lives in LDS.
//
// At G = 8 the concat tensor of a dense block has 64 + 4 * 8 = 96 channels: a 24 x 24 patch with its one-pixel zero border is
// 26 * 26 * 96 bf16 = 127 KiB, less than the 160 KiB of a CU.  One workgroup therefore loads the 64 input channels of an image, runs
// conv1 .. conv5 out of LDS with a barrier between the convs, and stores the 64 output channels: 128 B in and 128 B out per pixel
// (plus the RRDB skip of every third block) where the layer-by-layer path moves about 1.2 KB.  No ring, no row stream, no seam.
//
// LDS image: 12 planes of NP16 16-byte slots; plane 4 c + s holds channels 32 c + 8 s .. + 7 of every pixel of the padded image,
// pixel (y, x) in slot (y + 1)(W + 2) + x + 1.  NP16 = (H + 2)(W + 2) rounded up to 16, so a plane is a whole number of 256-byte bank
// rows: the B operand of v_mfma_f32_16x16x32_bf16 (lane = pixel + 16 * k-slice) is one ds_read_b128 whose 16-lane groups take eight
// pixels of one k-slice and eight of its neighbour (MI355X LDS: {0-3, 12-15, 20-27}, ..) -- consecutive pixels of a plane are
// consecutive slots, and the neighbour plane lies a multiple of 256 bytes away, so a tile inside one image row is conflict-free (a
// tile that wraps to the next row skips the two border slots and is 2-way on two banks).  The whole image is cleared at the start
// of every image: border, growth channels and pad; a workgroup's second image never sees its first.
//
// Tiles are 16 consecutive interior pixels in row-major order (a 24 x 24 patch: 36 tiles).  12 waves:
//   growth conv k: wave w owns tiles w, w + 12, ..: every weight fragment it loads (A operand: 8 couts padded to 16, K tail padded with
//                  zeros to whole 32-channel chunks) feeds all of its tiles.  bias, ReLU, ONE rounding to bf16, into plane 8 + (k - 1):
//                  the rounding points of the layer-by-layer path.  Channels [64, 96) start as zeros and are filled conv by conv, so a
//                  padded K tail multiplies zero weights with zeros or with finished values, never with stale memory.
//   conv5:         a unit is two of the four 16-cout blocks x six tiles; epilogue alpha * (conv + b) + beta1 * skip1 + beta2 * skip2 in
//                  the operation order of conv_rows_epi.h, rounded once.  The block's own input (a skip of every block) is read from LDS.
// Weights stream from L2 straight to registers (207 fragments of 1 KiB per block).
#include "common.h"

namespace {

constexpr int DB_THREADS = 768, DB_WAVES = DB_THREADS / 64;
constexpr int DB_G = 8, DB_CC = 64 + 4 * DB_G, DB_PLANES = DB_CC / 8;
constexpr int DB_TPW = 4;                        // growth convs: tiles a wave holds accumulators for at a time
constexpr int DB_T5 = 6;                         // conv5: tiles per unit
constexpr int DB_FRAG5 = 9 * (2 + 3 + 3 + 3);    // first fragment of conv5
constexpr int DB_FRAGS = DB_FRAG5 + 9 * 3 * 4;
constexpr int DB_BIAS = 4 * 16 + 64;

__host__ __device__ constexpr int db_nchunks(int k) { return k == 1 ? 2 : 3; }                       // 32-channel chunks conv k (1 .. 5) reads
__host__ __device__ constexpr int db_frag0(int k) { return k == 1 ? 0 : 9 * (2 + 3 * (k - 2)); }     // its first fragment

struct BlockParams {
    const bf16_t* in; bf16_t* grow; bf16_t* out; const bf16_t* so;
    const char* w; const float* bias;
    int B, H, W, np;
    float alpha, beta1, beta2;
    int x_skip;          // which skip (1 / 2) is the block's own input, read from LDS; the other one, if any, is `so`
    int store_growth;
};

typedef bf16x8 slot_t;

// The value, opaque to the optimiser: what is derived from it (a conv's tile slots and store offsets) is computed where it is used, per image, instead
// of being carried through all five convs in registers the MFMA loops need
__device__ __forceinline__ int fresh(int v) { asm volatile("" : "+v"(v)); return v; }

__device__ __forceinline__ int db_slot(int i, int W) { const int y = i / W; return (y + 1) * (W + 2) + (i - y * W) + 1; }

// NC chunks x 9 taps over the NT tiles at slots P[]: acc[j] += W . x.  The tap loop stays rolled and fetches the next tap's fragments while this tap's
// MFMAs run (unrolled, the compiler fetches the whole conv ahead and spills).
template <int NC, int NT>
__device__ __forceinline__ void growth_mma(const slot_t* lds, const slot_t* wf, int np, int Wp, const int (&P)[DB_TPW], int q, f32x4 (&acc)[DB_TPW]) {
    slot_t cur[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cur[c] = wf[c * 64];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = (tap * 11) >> 5, off = (dy - 1) * Wp + (tap - 3 * dy - 1);
        const int tn = min(tap + 1, 8);
        slot_t nxt[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) nxt[c] = wf[(tn * NC + c) * 64];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const slot_t x = lds[(c * 4 + q) * np + P[j] + off];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur[c], x, acc[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < NC; ++c) cur[c] = nxt[c];
    }
}

template <int NC>
__device__ __forceinline__ void growth_conv(const BlockParams& p, slot_t* lds, int k, int64_t img, int wave, int px, int q) {
    const int H = p.H, W = p.W, HW = H * W, Wp = W + 2, np = p.np;
    const int ntiles = (HW + 15) >> 4;
    const slot_t* wf = reinterpret_cast<const slot_t*>(p.w) + (size_t)db_frag0(k) * 64 + (px + 16 * q);
    const f32x4 biasv = *reinterpret_cast<const f32x4*>(p.bias + (k - 1) * 16 + 4 * (q & 1));
    for (int t0 = wave; t0 < ntiles; t0 += DB_WAVES * DB_TPW) {
        int P[DB_TPW], pix[DB_TPW];
        f32x4 acc[DB_TPW];
#pragma unroll
        for (int j = 0; j < DB_TPW; ++j) {
            pix[j] = (t0 + DB_WAVES * j) * 16 + px;
            P[j] = db_slot(min(pix[j], HW - 1), W);
            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int nt = min(DB_TPW, (ntiles - t0 + DB_WAVES - 1) / DB_WAVES);          // wave-uniform
        // (tiles beyond the image repeat its last pixel and are not stored: two instances cover every count -- one per count costs registers at the merge)
        if (nt <= 3) growth_mma<NC, 3>(lds, wf, np, Wp, P, q, acc);
        else growth_mma<NC, 4>(lds, wf, np, Wp, P, q, acc);
        // lanes q = 0, 1 hold couts 4 q .. 4 q + 3; q = 2, 3 the padding
#pragma unroll
        for (int j = 0; j < DB_TPW; ++j) {
            if (j < nt && q < 2 && pix[j] < HW) {
                f32x4 v = acc[j] + biasv;
                const bf16x4 o = {(bf16_t)fmaxf(v[0], 0.f), (bf16_t)fmaxf(v[1], 0.f), (bf16_t)fmaxf(v[2], 0.f), (bf16_t)fmaxf(v[3], 0.f)};
                reinterpret_cast<bf16x4*>(lds)[((8 + (k - 1)) * np + P[j]) * 2 + q] = o;
                if (p.store_growth) {
                    const int y = pix[j] / W, x = pix[j] - y * W;
                    *reinterpret_cast<bf16x4*>(p.grow + ((img * H + y) * 3 + 2) * (int64_t)(W * 32) + x * 32 + 8 * (k - 1) + 4 * q) = o;
                }
            }
        }
    }
}

// conv5's two cout blocks of a unit over its NT tiles: 27 (tap, chunk) steps of 2 NT MFMAs, each fetching the next step's two fragments first
template <int NT>
__device__ __forceinline__ void conv5_mma(const slot_t* lds, const slot_t* wf, int np, int Wp, const int (&P)[DB_T5], int q, f32x4 (&acc)[DB_T5][2]) {
    slot_t cur0 = wf[0], cur1 = wf[64];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = (tap * 11) >> 5, off = (dy - 1) * Wp + (tap - 3 * dy - 1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int sn = min(tap * 3 + c + 1, 26);
            const slot_t nxt0 = wf[(sn * 4) * 64], nxt1 = wf[(sn * 4 + 1) * 64];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const slot_t x = lds[(c * 4 + q) * np + P[j] + off];
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur0, x, acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur1, x, acc[j][1], 0, 0, 0);
            }
            cur0 = nxt0; cur1 = nxt1;
            __builtin_amdgcn_sched_barrier(0);   // one step's pixel fragments in flight, not the tap's
        }
    }
}

__device__ __forceinline__ void conv5(const BlockParams& p, const slot_t* lds, int64_t img, int wave, int px, int q) {
    const int H = p.H, W = p.W, HW = H * W, Wp = W + 2, np = p.np;
    const int ntiles = (HW + 15) >> 4, ngroups = (ntiles + DB_T5 - 1) / DB_T5;
    const float alpha = p.alpha, beta1 = p.beta1, beta2 = p.beta2;
    const bool has_so = p.so != nullptr, x_first = p.x_skip == 1;
    for (int u = wave; u < 2 * ngroups; u += DB_WAVES) {
        const int cp = u & 1, tg = u >> 1;
        const slot_t* wf = reinterpret_cast<const slot_t*>(p.w) + ((size_t)DB_FRAG5 + 2 * cp) * 64 + (px + 16 * q);
        int P[DB_T5], pix[DB_T5];
        f32x4 acc[DB_T5][2];
#pragma unroll
        for (int j = 0; j < DB_T5; ++j) {
            pix[j] = (tg * DB_T5 + j) * 16 + px;
            P[j] = db_slot(min(pix[j], HW - 1), W);
            acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int nt = min(DB_T5, ntiles - tg * DB_T5);                             // wave-uniform
        if (nt <= 3) conv5_mma<3>(lds, wf, np, Wp, P, q, acc);
        else conv5_mma<6>(lds, wf, np, Wp, P, q, acc);
        f32x4 biasv[2];
#pragma unroll
        for (int n = 0; n < 2; ++n) biasv[n] = *reinterpret_cast<const f32x4*>(p.bias + 64 + (2 * cp + n) * 16 + 4 * q);
        // couts 32 cp + 16 n + 4 q .. + 3: chunk cp of the output; in the LDS image plane 4 cp + 2 n + (q >> 1), half q & 1
#pragma unroll
        for (int j = 0; j < DB_T5; ++j) {
            if (j < nt && pix[j] < HW) {
                const int y = pix[j] / W, x = pix[j] - y * W;
                const int64_t e = ((img * H + y) * 3 + cp) * (int64_t)(W * 32) + x * 32 + 4 * q;
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const bf16x4 xs = reinterpret_cast<const bf16x4*>(lds)[((4 * cp + 2 * n + (q >> 1)) * np + P[j]) * 2 + (q & 1)];
                    bf16x4 os = xs;
                    if (has_so) os = *reinterpret_cast<const bf16x4*>(p.so + e + 16 * n);
                    const bf16x4 k1 = x_first ? xs : os, k2 = x_first ? os : xs;
                    f32x4 v = acc[j][n] + biasv[n];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        v[i] = v[i] * alpha;
                        v[i] += beta1 * (float)k1[i];
                        if (has_so) v[i] += beta2 * (float)k2[i];
                    }
                    const bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                    *reinterpret_cast<bf16x4*>(p.out + e + 16 * n) = o;
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // finish a tile before starting the next: keeps the register peak at one tile of temporaries
        }
    }
}

__global__ void __launch_bounds__(DB_THREADS) dense_block_lds_kernel(BlockParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    slot_t* lds = reinterpret_cast<slot_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, px = lane & 15, q = lane >> 4;
    const int H = p.H, W = p.W, Wp = W + 2, np = p.np;
    const int row_slots = W * 4, nunits = H * 2 * row_slots;          // 16-byte slices of channels [0, 64) of one image
    const slot_t zero = {};
    for (int64_t img = blockIdx.x; img < p.B; img += gridDim.x) {
        __syncthreads();                                              // the previous image's conv5 has read its skips
        for (int s = tid; s < DB_PLANES * np; s += DB_THREADS) lds[s] = zero;
        __syncthreads();
        // channels [0, 64) of the image, 16 bytes of one pixel at a time
        const slot_t* gin = reinterpret_cast<const slot_t*>(p.in) + img * H * 3 * row_slots;
#pragma unroll 4
        for (int u = tid; u < nunits; u += DB_THREADS) {
            const int rc = u / row_slots, within = u - rc * row_slots;
            const int y = rc >> 1, c = rc & 1;
            lds[(c * 4 + (within & 3)) * np + (y + 1) * Wp + (within >> 2) + 1] = gin[(y * 3 + c) * row_slots + within];
        }
        __syncthreads();
        growth_conv<2>(p, lds, 1, img, wave, fresh(px), fresh(q));
        __syncthreads();
        growth_conv<3>(p, lds, 2, img, wave, fresh(px), fresh(q));
        __syncthreads();
        growth_conv<3>(p, lds, 3, img, wave, fresh(px), fresh(q));
        __syncthreads();
        growth_conv<3>(p, lds, 4, img, wave, fresh(px), fresh(q));
        __syncthreads();
        conv5(p, lds, img, wave, fresh(px), fresh(q));
    }
}

int64_t lds_bytes(int G, int H, int W) {
    if (G != DB_G || H < 1 || W < 1) return -1;
    const int64_t npix = ((int64_t)H + 2) * ((int64_t)W + 2);
    const int64_t bytes = (npix + 15) / 16 * 16 * DB_PLANES * 16;
    if (bytes > sr_ctx::MAX_LDS_BYTES) return -1;
    return bytes;
}

}  // namespace

extern "C" int64_t sr_dense_block_lds_bytes(int growth_channels, int H, int W) { return lds_bytes(growth_channels, H, W); }

// k[i], b[i]: HWIO kernel [3][3][64 + 8 i][8] (i < 4) / [3][3][96][64] (i = 4) and bias of conv i + 1.  Fragment (tap, chunk c, cout block n) of a conv
// is the rows layout of conv_pack.h: lane l, element j = cin 32 c + 8 (l >> 4) + j, cout 16 n + (l & 15); zero beyond the conv's own cins / couts.
int block_pack_weights(sr_ctx* ctx, const float* const k[5], const float* const b[5], BlockWeights* out) {
    std::vector<uint16_t> packed((size_t)DB_FRAGS * 64 * 8, 0);
    std::vector<float> bias(DB_BIAS, 0.f);
    for (int i = 0; i < 5; ++i) {
        const int cin = 64 + DB_G * i, cout = i < 4 ? DB_G : 64, nc = db_nchunks(i + 1), nb = i < 4 ? 1 : 4;
        for (int tap = 0; tap < 9; ++tap)
            for (int c = 0; c < nc; ++c)
                for (int n = 0; n < nb; ++n) {
                    uint16_t* f = packed.data() + ((size_t)db_frag0(i + 1) + (tap * nc + c) * nb + n) * 64 * 8;
                    for (int l = 0; l < 64; ++l)
                        for (int j = 0; j < 8; ++j) {
                            const int ci = 32 * c + 8 * (l >> 4) + j, co = 16 * n + (l & 15);
                            if (ci < cin && co < cout) f[l * 8 + j] = f32_to_bf16_host(k[i][((size_t)tap * cin + ci) * cout + co]);
                        }
                }
        for (int co = 0; co < cout; ++co) bias[(i < 4 ? 16 * i : 64) + co] = b[i][co];
    }
    out->bytes = packed.size() * sizeof(uint16_t);
    return weights_upload(ctx, packed.data(), out->bytes, bias.data(), DB_BIAS, DB_BIAS, &out->w, &out->bias);
}

int block_launch(sr_ctx* ctx, const BlockWeights& w, TensorView in, int B, int H, int W, TensorView out, TensorView skip_o, float alpha, float beta1,
                 float beta2, int x_skip, int store_growth, hipStream_t st) {
    const int64_t lds = lds_bytes(DB_G, H, W);
    if (!w.w || lds <= 0 || B <= 0) return ctx->fail(SR_ERR_INVALID, "LDS-resident dense block: the image does not fit (sr_dense_block_lds_bytes)");
    for (const TensorView* v : {&in, &out, &skip_o})
        if ((v->p || v != &skip_o) && (!v->p || !v->blk || v->coff != 0 || v->cs != DB_CC))
            return ctx->fail(SR_ERR_INVALID, "LDS-resident dense block: needs row-blocked 96-channel concat buffers");
    if (in.p == out.p || (x_skip != 1 && x_skip != 2) || (!skip_o.p && x_skip != 1)) return ctx->fail(SR_ERR_INVALID, "LDS-resident dense block: bad skips or in-place output");
    BlockParams p;
    p.in = static_cast<const bf16_t*>(in.p); p.grow = static_cast<bf16_t*>(const_cast<void*>(in.p));
    p.out = static_cast<bf16_t*>(const_cast<void*>(out.p)); p.so = static_cast<const bf16_t*>(skip_o.p);
    p.w = static_cast<const char*>(w.w); p.bias = w.bias;
    p.B = B; p.H = H; p.W = W; p.np = (int)(lds / (DB_PLANES * 16));
    p.alpha = alpha; p.beta1 = beta1; p.beta2 = beta2; p.x_skip = x_skip; p.store_growth = store_growth;
    int grid = std::min(B, ctx->cu_count());
    if (ctx->chain_max_wgs > 0) grid = std::min(grid, ctx->chain_max_wgs);
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_lds_kernel), (int)lds)) return rc;
    int rec = -1;
    if (ctx->prof) {
        const double px = (double)B * H * W;
        double macs = 96.0 * 64.0;
        for (int i = 0; i < 4; ++i) macs += (64.0 + DB_G * i) * DB_G;
        rec = ctx->prof_open("dense_block_lds<bf16,g8>", 2.0 * px * 9.0 * macs, px * 2.0 * (64.0 + 64.0 + (skip_o.p ? 64.0 : 0.0) + (store_growth ? 32.0 : 0.0)), st);
    }
    hipLaunchKernelGGL(dense_block_lds_kernel, dim3(grid), dim3(DB_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
