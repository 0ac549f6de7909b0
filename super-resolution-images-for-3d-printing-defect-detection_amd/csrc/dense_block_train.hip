// dense_block_train.hip -- training a G = 8 dense block on the LDS-resident image of dense_block_lds.h: the device-side weight packer, the launcher of
// the forward kernel on a training tape's NHWC buffers, and the backward kernel.  Layouts, the forward body and the launchers' preamble: dense_block_lds.h.
//
// Backward, one workgroup of 12 waves per image, persistent over images.  The 12 planes of the LDS image hold G, the gradient of the concat tensor F; nothing else of
// size fits beside it, and nothing else is needed:
//   1. clear; dY's 64 channels with their zero border -> planes 0 .. 7
//   2. conv5's input gradient, channels [64, 96): bf16(a5 * acc) -> planes 8 .. 11, which dY does not occupy
//   3. conv5's input gradient, channels [0, 64): the forward conv5's shape -- a wave holds its ONE unit (2 output blocks x 6 tiles, 48 accumulator registers) across a
//      workgroup barrier; only then are the rounded values stored over dY
//   4. k = 4 .. 2: dz_k = G slice k where F slice k > 0 (a select on bits, in place on plane 8 + k - 1, stored to dz as well); barrier; the input-gradient conv from
//      that ONE plane into planes [0, cin_k / 8): a lane adds to, rounds and rewrites only elements it owns, and the input plane is never an output plane; barrier
//   5. k = 1: the select, the conv into registers; dX = bf16(acc + G[:64] + bx * dY), dY read again from global
// The growth convs' K is 8 of the MFMA's 32: the B-operand lanes of k-slices 1 .. 3 supply register zeros -- the neighbouring planes hold live G values, and a zero
// weight times an Inf would be a NaN.  Tiles beyond the image repeat its last pixel and store nothing (and add nothing to LDS).
#include "dense_block_lds.h"

namespace {

typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------------------------------------------------- the packer
struct PackPtrs { const float* k[5]; const float* b[5]; };      // one dense block: HWIO kernels [3][3][db_cin][db_cout] and biases, fp32, on the device

constexpr int PACK_ITEMS = (DB_FRAGS + DBT_BFRAGS) * 64 + DB_BIAS;     // per block: a (fragment, lane) each, then a bias entry each

// every item asks dense_block_lds.h's layout functions where its values come from (-1 / conv 0: a zero), as the host packer does for the forward half
__global__ void __launch_bounds__(256) dense_block_pack_kernel(const PackPtrs* tab, u16x8* fwd, float* bias, u16x8* bwd) {
    const int t = blockIdx.x * 256 + threadIdx.x, blk = blockIdx.y;
    if (t >= PACK_ITEMS) return;
    const PackPtrs& pp = tab[blk];
    if (t >= (DB_FRAGS + DBT_BFRAGS) * 64) {
        const int i = t - (DB_FRAGS + DBT_BFRAGS) * 64, c = db_bias_conv(i);
        bias[(size_t)blk * DB_BIAS + i] = c ? pp.b[c - 1][db_bias_src(i)] : 0.f;
        return;
    }
    const int f = t >> 6, l = t & 63, g = f - DB_FRAGS;
    const bool forward = f < DB_FRAGS;
    const DbFrag fr = db_frag_decode(forward ? f : 0);
    const float* kernel = pp.k[(forward ? fr.k : dbt_bfrag_conv(g)) - 1];
    u16x8 o = {};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int s = forward ? db_frag_src(fr, l, j) : dbt_bfrag_src(g, l, j);
        if (s >= 0) o[j] = f32_to_bf16_rne(kernel[s]);
    }
    if (forward) fwd[((size_t)blk * DB_FRAGS + f) * 64 + l] = o;
    else bwd[((size_t)blk * DBT_BFRAGS + g) * 64 + l] = o;
}

// ------------------------------------------------------------------------------------------------------------- backward
struct BwdParams {
    const bf16_t* dY; const bf16_t* F; bf16_t* dz; bf16_t* dX; bf16_t* stages;
    const char* w;
    int dy_cs, f_cs, dx_cs;
    int B, H, W, np;
    float a5, bx;
};

// Opaque to the optimiser, as dense_block_lds.h's fresh(): a stage derives its slots, addresses and masks from such copies, where it uses them, so that nothing of one
// stage is hoisted out of the image loop or carried through another stage's MFMA loop in registers (that is what spilled)
__device__ __forceinline__ int fresh_s(int v) { asm volatile("" : "+s"(v)); return v; }
struct Dims { int H, W, np; };
__device__ __forceinline__ Dims fresh_dims(const BwdParams& p) { return Dims{fresh_s(p.H), fresh_s(p.W), fresh_s(p.np)}; }

// conv5's input gradient: two of its six 16-channel output blocks over the NT tiles at slots P[]: 18 (tap, chunk) steps of 2 NT MFMAs, each fetching the next step's
// two fragments first.  wf: the lane's element of the unit's first fragment.
template <int NT>
__device__ __forceinline__ void dgrad5_mma(const slot_t* lds, const slot_t* wf, int np, int Wp, const int (&P)[DB_T5], int q, f32x4 (&acc)[DB_T5][2]) {
    slot_t cur0 = wf[0], cur1 = wf[64];
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = (tap * 11) >> 5, off = (dy - 1) * Wp + (tap - 3 * dy - 1);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int sn = min(tap * 2 + c + 1, 17);
            const slot_t nxt0 = wf[(sn * 6) * 64], nxt1 = wf[(sn * 6 + 1) * 64];
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const slot_t x = lds[(c * 4 + q) * np + P[j] + off];
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur0, x, acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cur1, x, acc[j][1], 0, 0, 0);
            }
            cur0 = nxt0; cur1 = nxt1;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// tiles t0 .. t0 + nt - 1 (nt <= NTMAX <= DB_T5) of block pair bp of conv5's input gradient into acc
__device__ __forceinline__ void dgrad5_unit(const BwdParams& p, const slot_t* lds, int bp, int t0, int nt, int px, int q, int (&P)[DB_T5], int (&pix)[DB_T5], f32x4 (&acc)[DB_T5][2]) {
    const Dims d = fresh_dims(p);
    const int HW = d.H * d.W;
    const slot_t* wf = reinterpret_cast<const slot_t*>(p.w) + ((size_t)dbt_bfrag0(5) + 2 * bp) * 64 + (px + 16 * q);
#pragma unroll
    for (int j = 0; j < DB_T5; ++j) {
        pix[j] = (t0 + j) * 16 + px;
        P[j] = db_slot(min(pix[j], HW - 1), d.W);
        acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (nt <= 3) dgrad5_mma<3>(lds, wf, d.np, d.W + 2, P, q, acc);
    else dgrad5_mma<6>(lds, wf, d.np, d.W + 2, P, q, acc);
}

// bf16(a5 * acc) of a unit's lanes into planes 4 bp + 2 n + (q >> 1), half q & 1: output channels 32 bp + 16 n + 4 q .. + 3
__device__ __forceinline__ void dgrad5_store(const BwdParams& p, slot_t* lds, int bp, int nt, int q, const int (&P)[DB_T5], const int (&pix)[DB_T5], const f32x4 (&acc)[DB_T5][2]) {
    const Dims d = fresh_dims(p);
    const int HW = d.H * d.W;
    const float a5 = p.a5;
#pragma unroll
    for (int j = 0; j < DB_T5; ++j) {
        if (j < nt && pix[j] < HW) {
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const f32x4 v = acc[j][n] * a5;
                const bf16x4 o = {(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                reinterpret_cast<bf16x4*>(lds)[((4 * bp + 2 * n + (q >> 1)) * d.np + P[j]) * 2 + (q & 1)] = o;
            }
        }
    }
}

constexpr int DBT_TPW = DBT_MAX_TILES / DB_WAVES;       // growth input-gradient convs: wave w owns tiles w, w + 12, w + 24

// dz_k = G slice k where F slice k > 0, else +0, in place on plane 8 + k - 1 and into dz; read off the bits (sign clear, not zero, not NaN)
__device__ __forceinline__ void relu_select(const BwdParams& p, slot_t* lds, int k, int64_t img, int tid) {
    const Dims d = fresh_dims(p);
    const int HW = d.H * d.W;
    u16x8* plane = reinterpret_cast<u16x8*>(lds) + (8 + k - 1) * d.np;
    for (int i = tid; i < HW; i += DB_THREADS) {
        const int s = db_slot(i, d.W);
        const u16x8 g = plane[s];
        const u16x8 f = *reinterpret_cast<const u16x8*>(p.F + (img * HW + i) * (int64_t)p.f_cs + DB_C0 + DB_G * (k - 1));
        u16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint16_t mag = f[j] & 0x7fffu;
            o[j] = ((f[j] & 0x8000u) == 0 && mag != 0 && mag <= 0x7f80u) ? g[j] : (uint16_t)0;
        }
        plane[s] = o;
        *reinterpret_cast<u16x8*>(p.dz + (img * HW + i) * (int64_t)(4 * DB_G) + DB_G * (k - 1)) = o;
    }
}

// the input-gradient conv of growth conv k from plane 8 + k - 1, output blocks N0 .. N0 + NN - 1 of its NB = dbt_nblocks(k), over the wave's tiles
template <int NB, int N0, int NN>
__device__ __forceinline__ void growth_dgrad_part(const BwdParams& p, slot_t* lds, int k, int64_t img, int wave, int px, int q) {
    const Dims d = fresh_dims(p);
    const int H = d.H, W = d.W, HW = H * W, Wp = W + 2, np = d.np;
    const int ntiles = (HW + 15) >> 4;
    if (wave >= ntiles) return;
    const int nt = (ntiles - wave + DB_WAVES - 1) / DB_WAVES;                       // wave-uniform, <= DBT_TPW
    const slot_t* wf = reinterpret_cast<const slot_t*>(p.w) + ((size_t)dbt_bfrag0(k) + N0) * 64 + (px + 16 * q);
    const slot_t* plane = lds + (8 + k - 1) * np;
    const slot_t zero = {};
    int P[DBT_TPW], pix[DBT_TPW];
    f32x4 acc[DBT_TPW][NN];
#pragma unroll
    for (int j = 0; j < DBT_TPW; ++j) {
        pix[j] = (wave + DB_WAVES * j) * 16 + px;
        P[j] = db_slot(min(pix[j], HW - 1), W);
#pragma unroll
        for (int n = 0; n < NN; ++n) acc[j][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
        const int dy = (tap * 11) >> 5, off = (dy - 1) * Wp + (tap - 3 * dy - 1);
        slot_t a[NN];
#pragma unroll
        for (int n = 0; n < NN; ++n) a[n] = wf[(tap * NB + n) * 64];
#pragma unroll
        for (int j = 0; j < DBT_TPW; ++j) {
            slot_t x = zero;                                                        // k-slices 1 .. 3: register zeros, never a neighbouring plane
            if (q == 0) x = plane[P[j] + off];
#pragma unroll
            for (int n = 0; n < NN; ++n) acc[j][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[n], x, acc[j][n], 0, 0, 0);
        }
    }
    // the lane holds output channels 16 n + 4 q .. + 3 of its pixel: plane 2 n + (q >> 1), half q & 1
    const int nplanes = db_cin(k) / 8;
    if (k > 1) {
#pragma unroll
        for (int j = 0; j < DBT_TPW; ++j) {
            if (j < nt && pix[j] < HW) {
#pragma unroll
                for (int n = 0; n < NN; ++n) {
                    const int pl = 2 * (N0 + n) + (q >> 1);
                    if (pl < nplanes) {
                        bf16x4* e = reinterpret_cast<bf16x4*>(lds) + (pl * np + P[j]) * 2 + (q & 1);
                        const bf16x4 g = *e;
                        const f32x4 v = acc[j][n] + f32x4{(float)g[0], (float)g[1], (float)g[2], (float)g[3]};
                        *e = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // finish a tile before starting the next
        }
    } else {
        const float bx = p.bx;
#pragma unroll
        for (int j = 0; j < DBT_TPW; ++j) {
            if (j < nt && pix[j] < HW) {
#pragma unroll
                for (int n = 0; n < NN; ++n) {
                    const int c0 = 16 * (N0 + n) + 4 * q;
                    const bf16x4 g = reinterpret_cast<const bf16x4*>(lds)[((2 * (N0 + n) + (q >> 1)) * np + P[j]) * 2 + (q & 1)];
                    const bf16x4 dy = *reinterpret_cast<const bf16x4*>(p.dY + (img * HW + pix[j]) * (int64_t)p.dy_cs + c0);
                    f32x4 v = acc[j][n] + f32x4{(float)g[0], (float)g[1], (float)g[2], (float)g[3]};
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] += bx * (float)dy[i];
                    *reinterpret_cast<bf16x4*>(p.dX + (img * HW + pix[j]) * (int64_t)p.dx_cs + c0) = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]};
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ... all NB blocks, three at a time: 36 accumulator registers beside conv5's 48 elsewhere in the kernel (all six at once, 72, and the kernel spilled)
template <int NB>
__device__ __forceinline__ void growth_dgrad(const BwdParams& p, slot_t* lds, int k, int64_t img, int wave, int px, int q) {
    constexpr int NA = NB < 3 ? NB : 3;
    growth_dgrad_part<NB, 0, NA>(p, lds, k, img, fresh_s(wave), fresh(px), fresh(q));
    if constexpr (NB > NA) growth_dgrad_part<NB, NA, NB - NA>(p, lds, k, img, fresh_s(wave), fresh(px), fresh(q));
}

// the whole G image of this workgroup's image -> stages[s][img]: [H][W][96]
__device__ __forceinline__ void dump_stage(const BwdParams& p, const slot_t* lds, int s, int64_t img, int tid) {
    const Dims d = fresh_dims(p);
    const int HW = d.H * d.W;
    slot_t* dst = reinterpret_cast<slot_t*>(p.stages) + (((int64_t)s * p.B + img) * HW) * DB_PLANES;
    for (int u = tid; u < HW * DB_PLANES; u += DB_THREADS) {
        const int i = u / DB_PLANES, pl = u - i * DB_PLANES;
        dst[u] = lds[pl * d.np + db_slot(i, d.W)];
    }
}

__global__ void __launch_bounds__(DB_THREADS) dense_block_bwd_kernel(BwdParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    slot_t* lds = reinterpret_cast<slot_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, px = lane & 15, q = lane >> 4;
    const int wave0 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool dump = p.stages != nullptr;
    for (int64_t img = blockIdx.x; img < p.B; img += gridDim.x) {
        __syncthreads();                                              // the previous image's last conv has read G
        {
            const Dims d = fresh_dims(p);
            const slot_t zero = {};
            for (int s = fresh(tid); s < DB_PLANES * d.np; s += DB_THREADS) lds[s] = zero;
            __syncthreads();
            const int64_t pix_slots = p.dy_cs / 8;
            const int HW = d.H * d.W;
            const slot_t* gin = reinterpret_cast<const slot_t*>(p.dY) + img * HW * pix_slots;
#pragma unroll 4
            for (int u = fresh(tid); u < HW * 8; u += DB_THREADS) lds[(u & 7) * d.np + db_slot(u >> 3, d.W)] = gin[(u >> 3) * pix_slots + (u & 7)];
        }
        __syncthreads();
        {
            const Dims d = fresh_dims(p);
            const int wave = fresh_s(wave0);
            const int ntiles = (d.H * d.W + 15) >> 4, ngroups = (ntiles + DB_T5 - 1) / DB_T5, ntrip = (ntiles + 2) / 3;      // <= DBT_MAX_TILES, 6 and 12 (the launcher checks)
            int P[DB_T5], pix[DB_T5];
            f32x4 acc[DB_T5][2];
            // channels [64, 96): units of three tiles, one per wave; into planes that nobody reads before the barrier below
            if (wave < ntrip) {
                const int nt = min(3, ntiles - 3 * wave);
                dgrad5_unit(p, lds, 2, 3 * wave, nt, fresh(px), fresh(q), P, pix, acc);
                dgrad5_store(p, lds, 2, nt, fresh(q), P, pix, acc);
            }
            // channels [0, 64): every unit's accumulators are complete before any of them replaces dY
            const bool has = wave < 2 * ngroups;
            const int bp = wave & 1, tg = wave >> 1, nt = min(DB_T5, ntiles - tg * DB_T5);
            if (has) dgrad5_unit(p, lds, bp, tg * DB_T5, nt, fresh(px), fresh(q), P, pix, acc);
            __syncthreads();
            if (has) dgrad5_store(p, lds, bp, nt, fresh(q), P, pix, acc);
        }
        __syncthreads();
        if (dump) { dump_stage(p, lds, 0, img, fresh(tid)); __syncthreads(); }
        relu_select(p, lds, 4, img, fresh(tid));
        __syncthreads();
        growth_dgrad<dbt_nblocks(4)>(p, lds, 4, img, fresh_s(wave0), fresh(px), fresh(q));
        __syncthreads();
        if (dump) { dump_stage(p, lds, 1, img, fresh(tid)); __syncthreads(); }
        relu_select(p, lds, 3, img, fresh(tid));
        __syncthreads();
        growth_dgrad<dbt_nblocks(3)>(p, lds, 3, img, fresh_s(wave0), fresh(px), fresh(q));
        __syncthreads();
        if (dump) { dump_stage(p, lds, 2, img, fresh(tid)); __syncthreads(); }
        relu_select(p, lds, 2, img, fresh(tid));
        __syncthreads();
        growth_dgrad<dbt_nblocks(2)>(p, lds, 2, img, fresh_s(wave0), fresh(px), fresh(q));
        __syncthreads();
        if (dump) { dump_stage(p, lds, 3, img, fresh(tid)); __syncthreads(); }
        relu_select(p, lds, 1, img, fresh(tid));
        __syncthreads();
        growth_dgrad<dbt_nblocks(1)>(p, lds, 1, img, fresh_s(wave0), fresh(px), fresh(q));
    }
}

bool view_ok(const sr_view* v, int C) {
    return v && v->p && v->cs > 0 && v->coff >= 0 && v->cs % 8 == 0 && v->coff % 8 == 0 && v->cs - v->coff >= C && ((uintptr_t)v->p % 16) == 0;
}
const bf16_t* view_ptr(const sr_view* v) { return static_cast<const bf16_t*>(v->p) + v->coff; }

}  // namespace

extern "C" {

int sr_dense_block_train_max_pixels(void) { return DBT_MAX_NPIX; }

void sr_dense_block_pack_sizes(int64_t* fwd_bytes, int64_t* bias_floats, int64_t* bwd_bytes) {
    if (fwd_bytes) *fwd_bytes = (int64_t)DB_FRAGS * 1024;
    if (bias_floats) *bias_floats = DB_BIAS;
    if (bwd_bytes) *bwd_bytes = (int64_t)DBT_BFRAGS * 1024;
}

int sr_dense_block_pack_dev(sr_ctx* ctx, const void* d_table, int nblocks, void* fwd, float* bias, void* bwd, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!d_table || !fwd || !bias || !bwd || nblocks <= 0 || nblocks > 65535) return ctx->fail(SR_ERR_INVALID, "dense block pack: null buffer or bad block count");
    if (((uintptr_t)fwd % 16) != 0 || ((uintptr_t)bwd % 16) != 0 || ((uintptr_t)d_table % 8) != 0) return ctx->fail(SR_ERR_INVALID, "dense block pack: buffers must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rec = -1;
    if (ctx->prof) rec = ctx->prof_open("dense_block_pack_dev<g8>", 0.0, (double)nblocks * ((DB_FRAGS + DBT_BFRAGS) * 1024.0 * 3.0), st);
    hipLaunchKernelGGL(dense_block_pack_kernel, dim3((PACK_ITEMS + 255) / 256, nblocks), dim3(256), 0, st, static_cast<const PackPtrs*>(d_table), static_cast<u16x8*>(fwd), bias,
                       static_cast<u16x8*>(bwd));
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_dense_block_fwd_bf16(sr_ctx* ctx, const void* fwd_w, const float* bias, void* F, int64_t f_cs, int B, int H, int W, const sr_view* out, const sr_view* skip2, float alpha,
                            float beta1, float beta2, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lds = db_lds_bytes(DB_G, H, W);
    if (lds <= 0 || B <= 0) return ctx->fail(SR_ERR_INVALID, "LDS-resident dense block: the image does not fit (sr_dense_block_lds_bytes)");
    if (!fwd_w || !bias || !F || f_cs < DB_CC || f_cs % 8 != 0 || ((uintptr_t)F % 16) != 0 || ((uintptr_t)fwd_w % 16) != 0 || ((uintptr_t)bias % 16) != 0)
        return ctx->fail(SR_ERR_INVALID, "dense block fwd: needs packed weights and a 16-byte aligned NHWC concat buffer of at least 96 channels, a multiple of 8");
    if (!view_ok(out, DB_C0) || (skip2 && skip2->p && !view_ok(skip2, DB_C0))) return ctx->fail(SR_ERR_INVALID, "dense block fwd: a view needs 64 channels, cs and coff multiples of 8");
    if (out->p == F) return ctx->fail(SR_ERR_INVALID, "dense block fwd: the output may not lie in the block's own concat buffer");
    BlockParamsNHWC p;
    db_fill_params(p, F, view_ptr(out), (skip2 && skip2->p) ? view_ptr(skip2) : nullptr, fwd_w, bias, B, H, W, (int)(lds / (DB_PLANES * 16)), alpha, beta1, beta2, 1, 1);
    p.in_cs = (int)f_cs; p.out_cs = (int)out->cs; p.so_cs = p.so ? (int)skip2->cs : 0;
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_lds_kernel<BlockParamsNHWC>), (int)lds)) return rc;
    const int rec = db_prof_open(ctx, "dense_block_fwd_lds<bf16,g8,nhwc>", B, H, W, 64.0 + 64.0 + 32.0 + (p.so ? 64.0 : 0.0), st);
    hipLaunchKernelGGL(dense_block_lds_kernel<BlockParamsNHWC>, dim3(db_grid(ctx, B)), dim3(DB_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_dense_block_bwd_bf16(sr_ctx* ctx, const void* bwd_w, const sr_view* dY, const void* F, int64_t f_cs, int B, int H, int W, float a5, float bx, void* dz, const sr_view* dX,
                            void* stages, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int64_t lds = db_lds_bytes(DB_G, H, W);
    if (lds <= 0 || B <= 0 || ((int64_t)H + 2) * ((int64_t)W + 2) > DBT_MAX_NPIX)
        return ctx->fail(SR_ERR_INVALID, "dense block bwd: the image does not fit (sr_dense_block_lds_bytes, sr_dense_block_train_max_pixels)");
    if (!bwd_w || !F || !dz || f_cs < DB_CC || f_cs % 8 != 0 || ((uintptr_t)F % 16) != 0 || ((uintptr_t)bwd_w % 16) != 0 || ((uintptr_t)dz % 16) != 0 ||
        (stages && ((uintptr_t)stages % 16) != 0))
        return ctx->fail(SR_ERR_INVALID, "dense block bwd: needs packed weights, a 16-byte aligned NHWC concat buffer of at least 96 channels and a [B,H,W,32] dz");
    if (!view_ok(dY, DB_C0) || !view_ok(dX, DB_C0)) return ctx->fail(SR_ERR_INVALID, "dense block bwd: a view needs 64 channels, cs and coff multiples of 8");
    BwdParams p;
    p.dY = view_ptr(dY); p.F = static_cast<const bf16_t*>(F); p.dz = static_cast<bf16_t*>(dz); p.dX = const_cast<bf16_t*>(view_ptr(dX));
    p.stages = static_cast<bf16_t*>(stages); p.w = static_cast<const char*>(bwd_w);
    p.dy_cs = (int)dY->cs; p.f_cs = (int)f_cs; p.dx_cs = (int)dX->cs;
    p.B = B; p.H = H; p.W = W; p.np = (int)(lds / (DB_PLANES * 16));
    p.a5 = a5; p.bx = bx;
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_bwd_kernel), (int)lds)) return rc;
    const int rec = db_prof_open(ctx, "dense_block_bwd_lds<bf16,g8>", B, H, W, 64.0 + 64.0 + 32.0 + 32.0 + 64.0, st);
    hipLaunchKernelGGL(dense_block_bwd_kernel, dim3(db_grid(ctx, B)), dim3(DB_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
