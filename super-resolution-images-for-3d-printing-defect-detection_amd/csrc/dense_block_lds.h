// dense_block_lds.h -- the G = 8 dense block, stated once for its kernels: the LDS-resident forward kernel (a template over how the image lies in global memory:
// dense_block.hip launches it on sr_forward's row-blocked buffers, dense_block_train.hip on a training tape's NHWC buffers), the row-ring kernel
// (dense_block_stream.hip) and the backward kernel (dense_block_train.hip).  Here: the fragment and bias layouts for the host and the device packer, the two
// epilogues, the tap offset, the resident kernel's body and the launchers' shared preamble.
//
// At G = 8 the concat tensor of a dense block has 64 + 4 * 8 = 96 channels: a 24 x 24 patch with its one-pixel zero border is 26 * 26 * 96 bf16 = 127 KiB, less than
// the 160 KiB of a CU.  One workgroup therefore loads the 64 input channels of an image, runs conv1 .. conv5 out of LDS with a barrier between the convs, and stores
// the 64 output channels: 128 B in and 128 B out per pixel (plus the RRDB skip of every third block) where the layer-by-layer path moves about 1.2 KB.
//
// LDS image: 12 planes of NP16 16-byte slots; plane 4 c + s holds channels 32 c + 8 s .. + 7 of every pixel of the padded image, pixel (y, x) in slot
// (y + 1)(W + 2) + x + 1.  NP16 = (H + 2)(W + 2) rounded up to 16, so a plane is a whole number of 256-byte bank rows: the B operand of v_mfma_f32_16x16x32_bf16
// (lane = pixel + 16 * k-slice) is one ds_read_b128 whose 16-lane groups take eight pixels of one k-slice and eight of its neighbour (MI355X LDS: {0-3, 12-15,
// 20-27}, ..) -- consecutive pixels of a plane are consecutive slots, and the neighbour plane lies a multiple of 256 bytes away, so a tile inside one image row is
// conflict-free (a tile that wraps to the next row skips the two border slots and is 2-way on two banks).  The whole image is cleared at the start of every image:
// border, growth channels and pad; a workgroup's second image never sees its first.
//
// Tiles are 16 consecutive interior pixels in row-major order (a 24 x 24 patch: 36 tiles).  12 waves:
//   growth conv k: wave w owns tiles w, w + 12, ..: every weight fragment it loads (A operand: 8 couts padded to 16, K tail padded with zeros to whole 32-channel
//                  chunks) feeds all of its tiles.  db_growth_epilogue into plane 8 + (k - 1).  Channels [64, 96) start as zeros and are filled conv by conv, so a
//                  padded K tail multiplies zero weights with zeros or with finished values, never with stale memory.
//   conv5:         a unit is two of the four 16-cout blocks x six tiles; db_conv5_epilogue.  The block's own input (a skip of every block) is read from LDS.
// Weights stream from L2 straight to registers (207 fragments of 1 KiB per block).
//
// Forward fragments (DB_FRAGS of 1 KiB = 64 lanes x 8 bf16): conv k (1 .. 5) starts at db_frag0(k) and holds (tap, chunk c < db_nchunks(k), cout block n < db_nblk(k))
// at (tap * nc + c) * nb + n; lane l, element j = cin 32 c + 8 (l >> 4) + j, cout 16 n + (l & 15) of kernel tap `tap` (the rows layout of conv_pack.h); zero beyond
// the conv's own cins and couts: db_frag_decode / db_frag_src.  Bias table (DB_BIAS floats): conv k < 5 at 16 (k - 1), conv5 at 64; zero padded: db_bias_conv / db_bias_src.
//
// Backward (input-gradient) fragments (DBT_BFRAGS of 1 KiB, dbt_bfrag_src): the conv that carries a gradient of conv k's output back to its input is a 3x3 conv with
// the taps rotated by 180 degrees and cin / cout swapped: tap t of it is kernel tap 8 - t.
//   conv5 (K = its 64 couts, two 32-channel chunks; 96 input channels = six 16-row output blocks): (tap, chunk c, block n) at dbt_bfrag0(5) + (tap * 2 + c) * 6 + n; lane l,
//         element j = kernel[8 - tap][cin 16 n + (l & 15)][cout 32 c + 8 (l >> 4) + j].
//   conv k < 5 (K = its 8 couts in ONE chunk whose K rows 8 .. 31 are zero; dbt_nblocks(k) = ceil(cin_k / 16) output blocks): (tap, block n) at dbt_bfrag0(k) + tap * nb + n;
//         lane l < 16, element j = kernel[8 - tap][cin 16 n + l][cout j], zero where the cin is beyond the conv's own; lanes 16 .. 63 zero.
#pragma once
#include "common.h"

namespace {

constexpr int DB_THREADS = 768, DB_WAVES = DB_THREADS / 64;
constexpr int DB_G = 8, DB_C0 = 64, DB_CC = DB_C0 + 4 * DB_G, DB_PLANES = DB_CC / 8;
constexpr int DB_TPW = 4;                        // growth convs: tiles a wave holds accumulators for at a time
constexpr int DB_T5 = 6;                         // conv5: tiles per unit
constexpr int DB_FRAG5 = 9 * (2 + 3 + 3 + 3);    // first fragment of conv5
constexpr int DB_FRAGS = DB_FRAG5 + 9 * 3 * 4;
constexpr int DB_BIAS = 4 * 16 + 64;

__host__ __device__ constexpr int db_nchunks(int k) { return k == 1 ? 2 : 3; }                       // 32-channel chunks conv k (1 .. 5) reads
__host__ __device__ constexpr int db_frag0(int k) { return k == 1 ? 0 : 9 * (2 + 3 * (k - 2)); }     // its first fragment
__host__ __device__ constexpr int db_cin(int k) { return DB_C0 + DB_G * (k - 1); }
__host__ __device__ constexpr int db_cout(int k) { return k < 5 ? DB_G : DB_C0; }
__host__ __device__ constexpr int db_nblk(int k) { return k < 5 ? 1 : 4; }                             // its 16-cout blocks
__host__ __device__ constexpr int db_frag_conv(int f) { return f >= DB_FRAG5 ? 5 : f < db_frag0(2) ? 1 : 2 + (f - db_frag0(2)) / 27; }
struct DbFrag { int k, tap, c, n; };             // forward fragment f: conv, kernel tap, 32-channel chunk, cout block
__host__ __device__ inline DbFrag db_frag_decode(int f) {
    const int k = db_frag_conv(f), r = f - db_frag0(k), nb = db_nblk(k), nc = db_nchunks(k);
    return DbFrag{k, r / (nb * nc), r / nb % nc, r % nb};
}
// where lane l, element j of a forward fragment comes from in its conv's HWIO kernel [3][3][db_cin][db_cout]; -1: a zero
__host__ __device__ inline int db_frag_src(const DbFrag& fr, int l, int j) {
    const int ci = 32 * fr.c + 8 * (l >> 4) + j, co = 16 * fr.n + (l & 15);
    return ci < db_cin(fr.k) && co < db_cout(fr.k) ? (fr.tap * db_cin(fr.k) + ci) * db_cout(fr.k) + co : -1;
}
// entry i of the bias table: the conv (0: a zero) and the index in that conv's bias
__host__ __device__ constexpr int db_bias_conv(int i) { return i >= 64 ? 5 : (i & 15) < DB_G ? (i >> 4) + 1 : 0; }
__host__ __device__ constexpr int db_bias_src(int i) { return i >= 64 ? i - 64 : i & 15; }

// the input-gradient fragments
__host__ __device__ constexpr int dbt_nblocks(int k) { return (db_cin(k) + 15) / 16; }               // 16-row output blocks of conv k's input-gradient conv: 4, 5, 5, 6, 6
__host__ __device__ constexpr int dbt_bfrag0(int k) { return k == 5 ? 0 : 9 * 2 * 6 + 9 * (k == 1 ? 0 : k == 2 ? 4 : k == 3 ? 9 : 14); }
constexpr int DBT_BFRAGS = 9 * 2 * 6 + 9 * (4 + 5 + 5 + 6);
__host__ __device__ constexpr int dbt_bfrag_conv(int g) { return g < dbt_bfrag0(1) ? 5 : g < dbt_bfrag0(2) ? 1 : g < dbt_bfrag0(3) ? 2 : g < dbt_bfrag0(4) ? 3 : 4; }
// where lane l, element j of backward fragment g comes from in the HWIO kernel of conv dbt_bfrag_conv(g); -1: a zero
__host__ __device__ inline int dbt_bfrag_src(int g, int l, int j) {
    const int k = dbt_bfrag_conv(g), r = g - dbt_bfrag0(k);
    if (k == 5) {
        const int n = r % 6, c = r / 6 & 1, tap = r / 12;
        return ((8 - tap) * DB_CC + 16 * n + (l & 15)) * DB_C0 + 32 * c + 8 * (l >> 4) + j;
    }
    const int nb = dbt_nblocks(k), n = r % nb, tap = r / nb, ci = 16 * n + l;
    return l < 16 && ci < db_cin(k) ? ((8 - tap) * db_cin(k) + ci) * DB_G + j : -1;
}
// the images that the backward kernel takes: conv5's input gradient of channels [0, 64) is held in registers by 12 waves of one unit (2 blocks x 6 tiles) each
constexpr int DBT_MAX_TILES = DB_WAVES / 2 * DB_T5;
// ... stated as a bound on the padded image: (H + 2)(W + 2) <= N gives H W <= (sqrt(N) - 2)^2, here 24 x 24 pixels = 36 tiles
constexpr int DBT_MAX_NPIX = 676;
static_assert((26 - 2) * (26 - 2) == DBT_MAX_TILES * 16 && 26 * 26 == DBT_MAX_NPIX, "every image the backward kernel accepts has at most DBT_MAX_TILES tiles");

struct BlockParams {
    const bf16_t* in; bf16_t* grow; bf16_t* out; const bf16_t* so;
    const char* w; const float* bias;
    int B, H, W, np;
    float alpha, beta1, beta2;
    int x_skip;          // which skip (1 / 2) is the block's own input, read from LDS; the other one, if any, is `so`
    int store_growth;
    static constexpr bool NHWC = false;      // row-blocked buffers [B][H][3][W][32] (sr_forward's)
};
// the same on NHWC buffers [B][H][W][cs] (a training tape's); the growth slices are always stored
struct BlockParamsNHWC : BlockParams {
    int in_cs, out_cs, so_cs;                // channels per pixel of the buffers behind in / grow, out and so
    static constexpr bool NHWC = true;
};

typedef bf16x8 slot_t;

// The value, opaque to the optimiser: what is derived from it (a conv's tile slots and store offsets) is computed where it is used, per image, instead
// of being carried through all five convs in registers the MFMA loops need
__device__ __forceinline__ int fresh(int v) { asm volatile("" : "+v"(v)); return v; }

__device__ __forceinline__ int db_slot(int i, int W) { const int y = i / W; return (y + 1) * (W + 2) + (i - y * W) + 1; }
// Kernel tap `tap` of a 3x3 conv reads the slot off = (dy - 1) * Wp + (dx - 1) from the output pixel's, dy = (tap * 11) >> 5 = tap / 3, in an image of Wp slots
// per row.  The four tap loops (here and in dense_block_train.hip) write that out: as a function of any form it changed their kernels' register allocation
// (the resident kernel's VGPRs, the backward kernel's SGPR spills).

// The two epilogues, in fp32 on a lane's four couts, each rounded ONCE to bf16: the rounding points of the layer-by-layer path.
// growth conv: ReLU(acc + b)
__device__ __forceinline__ bf16x4 db_growth_epilogue(f32x4 acc, f32x4 biasv) {
    const f32x4 v = acc + biasv;
    return bf16x4{(bf16_t)fmaxf(v[0], 0.f), (bf16_t)fmaxf(v[1], 0.f), (bf16_t)fmaxf(v[2], 0.f), (bf16_t)fmaxf(v[3], 0.f)};
}
// conv5: alpha * (acc + b) + beta1 * skip1 + beta2 * skip2 in the operation order of conv_rows_epi.h.  xs: the block's own input, skip 1 if x_first, else 2;
// os: the other skip (used only with has_so)
__device__ __forceinline__ bf16x4 db_conv5_epilogue(f32x4 acc, f32x4 biasv, bf16x4 xs, bf16x4 os, bool has_so, bool x_first, float alpha, float beta1, float beta2) {
    const bf16x4 k1 = x_first ? xs : os, k2 = x_first ? os : xs;
    f32x4 v = acc + biasv;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = v[i] * alpha;
        v[i] += beta1 * (float)k1[i];
        if (has_so) v[i] += beta2 * (float)k2[i];
    }
    return bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
}

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

template <int NC, typename PT>
__device__ __forceinline__ void growth_conv(const PT& p, slot_t* lds, int k, int64_t img, int wave, int px, int q) {
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
                const bf16x4 o = db_growth_epilogue(acc[j], biasv);
                reinterpret_cast<bf16x4*>(lds)[((8 + (k - 1)) * np + P[j]) * 2 + q] = o;
                if (PT::NHWC || p.store_growth) {
                    if constexpr (PT::NHWC) {
                        *reinterpret_cast<bf16x4*>(p.grow + img * HW * p.in_cs + (pix[j] * p.in_cs + DB_C0 + 8 * (k - 1) + 4 * q)) = o;      // (an image is far below 2^31 elements)
                    } else {
                        const int y = pix[j] / W, x = pix[j] - y * W;
                        *reinterpret_cast<bf16x4*>(p.grow + ((img * H + y) * 3 + 2) * (int64_t)(W * 32) + x * 32 + 8 * (k - 1) + 4 * q) = o;
                    }
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

template <typename PT>
__device__ __forceinline__ void conv5(const PT& p, const slot_t* lds, int64_t img, int wave, int px, int q) {
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
                int64_t e, es;      // first element of the lane's four couts (n = 0) in out and in so
                if constexpr (PT::NHWC) {
                    e = img * HW * p.out_cs + (pix[j] * p.out_cs + 32 * cp + 4 * q);
                    es = img * HW * p.so_cs + (pix[j] * p.so_cs + 32 * cp + 4 * q);
                } else {
                    const int y = pix[j] / W, x = pix[j] - y * W;
                    e = es = ((img * H + y) * 3 + cp) * (int64_t)(W * 32) + x * 32 + 4 * q;
                }
#pragma unroll
                for (int n = 0; n < 2; ++n) {
                    const bf16x4 xs = reinterpret_cast<const bf16x4*>(lds)[((4 * cp + 2 * n + (q >> 1)) * np + P[j]) * 2 + (q & 1)];
                    bf16x4 os = xs;
                    if (has_so) os = *reinterpret_cast<const bf16x4*>(p.so + es + 16 * n);
                    *reinterpret_cast<bf16x4*>(p.out + e + 16 * n) = db_conv5_epilogue(acc[j][n], biasv[n], xs, os, has_so, x_first, alpha, beta1, beta2);
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // finish a tile before starting the next: keeps the register peak at one tile of temporaries
        }
    }
}

template <typename PT>
__global__ void __launch_bounds__(DB_THREADS) dense_block_lds_kernel(PT p) {
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
        if constexpr (PT::NHWC) {
            const int64_t pix_slots = p.in_cs / 8;
            const slot_t* gin = reinterpret_cast<const slot_t*>(p.in) + img * H * W * pix_slots;
#pragma unroll 4
            for (int u = tid; u < nunits; u += DB_THREADS) lds[(u & 7) * np + db_slot(u >> 3, W)] = gin[(u >> 3) * pix_slots + (u & 7)];
        } else {
            const slot_t* gin = reinterpret_cast<const slot_t*>(p.in) + img * H * 3 * row_slots;
#pragma unroll 4
            for (int u = tid; u < nunits; u += DB_THREADS) {
                const int rc = u / row_slots, within = u - rc * row_slots;
                const int y = rc >> 1, c = rc & 1;
                lds[(c * 4 + (within & 3)) * np + (y + 1) * Wp + (within >> 2) + 1] = gin[(y * 3 + c) * row_slots + within];
            }
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

// ---- the launchers' shared preamble
int64_t db_lds_bytes(int G, int H, int W) {
    if (G != DB_G || H < 1 || W < 1) return -1;
    const int64_t npix = ((int64_t)H + 2) * ((int64_t)W + 2);
    const int64_t bytes = (npix + 15) / 16 * 16 * DB_PLANES * 16;
    if (bytes > sr_ctx::MAX_LDS_BYTES) return -1;
    return bytes;
}

double db_block_macs() {                          // per pixel and tap
    double macs = 0.0;
    for (int k = 1; k <= 5; ++k) macs += (double)db_cin(k) * db_cout(k);
    return macs;
}

// a persistent grid over `items` work items: one workgroup per CU at the most
int db_grid(sr_ctx* ctx, int items) {
    int grid = std::min(items, ctx->cu_count());
    if (ctx->chain_max_wgs > 0) grid = std::min(grid, ctx->chain_max_wgs);
    return grid;
}

// a profiler record of one block over B H W pixels that moves `channels` bf16 per pixel
int db_prof_open(sr_ctx* ctx, const char* name, int B, int H, int W, double channels, hipStream_t st) {
    if (!ctx->prof) return -1;
    const double px = (double)B * H * W;
    return ctx->prof_open(name, 2.0 * px * 9.0 * db_block_macs(), px * 2.0 * channels, st);
}

// the row-blocked launchers' (block_launch, block_stream_launch) views and skips; `who` opens the message
int db_check_blocked_views(sr_ctx* ctx, const char* who, const TensorView& in, const TensorView& out, const TensorView& skip_o, int x_skip) {
    for (const TensorView* v : {&in, &out, &skip_o})
        if ((v->p || v != &skip_o) && (!v->p || !v->blk || v->coff != 0 || v->cs != DB_CC))
            return ctx->fail(SR_ERR_INVALID, std::string(who) + ": needs row-blocked 96-channel concat buffers");
    if (in.p == out.p || (x_skip != 1 && x_skip != 2) || (!skip_o.p && x_skip != 1)) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": bad skips or in-place output");
    return SR_OK;
}

// in: the block's concat buffer (its growth slices are stored there); so: the other skip or null
void db_fill_params(BlockParams& p, const void* in, const void* out, const void* so, const void* w, const float* bias, int B, int H, int W, int np, float alpha, float beta1,
                    float beta2, int x_skip, int store_growth) {
    p.in = static_cast<const bf16_t*>(in); p.grow = static_cast<bf16_t*>(const_cast<void*>(in));
    p.out = static_cast<bf16_t*>(const_cast<void*>(out)); p.so = static_cast<const bf16_t*>(so);
    p.w = static_cast<const char*>(w); p.bias = bias;
    p.B = B; p.H = H; p.W = W; p.np = np;
    p.alpha = alpha; p.beta1 = beta1; p.beta2 = beta2; p.x_skip = x_skip; p.store_growth = store_growth;
}

}  // namespace
