// dense_block_stream.hip -- a whole ESRGAN dense block at 8 growth channels as ONE kernel that streams image rows through a ring in LDS: the line-buffer
// variant of the resident kernel (dense_block_lds.h) for images too large to be LDS-resident (48 x 48 patches: ESRGAN.super_resolve_image's default patch_size_lr).
//
// LDS: 12 planes (plane p = channels 8 p .. 8 p + 7) of a ring of R image rows; a row is WP = 16 ceil(W / 16) + 2 sixteen-byte slots: a zero border slot, the W
// pixels, and zeros up to the end of the last 16-pixel tile and the right border; image row y lies in ring row y mod R.  A plane is R WP slots rounded up to 16, a
// whole number of 256-byte bank rows: the B operand of v_mfma_f32_16x16x32_bf16 is one conflict-free ds_read_b128 per lane, as in dense_block_lds.h.  Whole tiles
// per row make a tile's slot a constant distance from its neighbour's: one address register per (chunk, row) serves the 3 tiles x 3 horizontal taps of a wave.
// A wave computes tiles in threes: past the last tile of a row it reads on into the next ring row or plane (finite values, results dropped), past the last
// plane into DS_OVER spare slots.
//
// Work item = (image, band of output rows [y0, y1)).  Step r: input row r (channels [0, 64)) is in the ring, conv k produces row r - delay(k) from rows
// that EARLIER barriers finished.  A 3x3 conv at row y reads row y + 1 of its input, so with all five convs running at once (one barrier per step) conv k
// can only follow conv k - 1 at a distance of TWO rows: delay = 1, 3, 5, 7, 9, and with the row being prefetched the ring holds rows r - 10 .. r + 1: R = 12.
// That fits up to W = 64.  Wider images (up to W = 96) take the schedule of five phases per step, a barrier after each: conv k in phase k - 1 follows at ONE
// row, delay = 1 .. 5, rows r - 6 .. r + 1: R = 8.  Either way a conv reads only rows that a barrier has finished and the layers write disjoint (row, plane) pairs.
//
// 8 waves, each with ONE role for the whole kernel: wave k - 1 is growth conv k (k = 1 .. 4), wave 4 + n is cout block n of conv5.  A role's 18 / 27
// weight fragments (27 KiB) stay in its registers from the first work item to the last: the 207 KiB of a block's weights are read once per workgroup, not once
// per row.  Per row and 48 pixels: 54 + 3 * 81 MFMAs on the growth waves, 4 * 81 on the conv5 waves; waves w and w + 4 share a SIMD.
//
// Arithmetic is the resident kernel's: per output element one fp32 accumulator chain from zero, taps outer, 32-channel chunks inner, then the same function
// as there: db_growth_epilogue or db_conv5_epilogue (dense_block_lds.h).  The result therefore has the resident kernel's bits and depends neither on the band
// count nor on the schedule.
//
// Zeros: the ring is cleared at the start of every work item.  When a ring row is recycled for input row r + 1, its growth planes are cleared with it, and a row
// outside the image (or outside what the band needs) is cleared in all 12 planes: a growth conv's K tail multiplies zero weights with zeros or with finished
// values only, and rows y < 0, y >= H read as zero in all 96 channels.
#include <algorithm>
#include "dense_block_lds.h"

namespace {

constexpr int DS_THREADS = 512;
constexpr int DS_NT = 3;                        // tiles (16 pixels of one row) a wave holds accumulators for at a time
constexpr int DS_HALO = 5;                      // rows of input beyond a band on either side: one per conv
// Bands: each costs DS_HALO + delay(5) = 10 or 14 steps that store nothing.  Bands are only cut while every work item still gets a workgroup of its own, so a
// launch lasts (rows of a band + 14) steps and shorter bands only shorten it: measured on a 239 x 239 frame in chunks of 16 patches of 48 x 48,
// 3 / 6 / 12 / 16 bands per patch took 6.99 / 5.68 / 4.86 / 4.65 ms.  The floor of 3 rows (a 3x3 conv's reach) caps the recomputation at about 6 x the work.
constexpr int DS_MIN_BAND = 3;

// the two schedules: how far conv k runs behind the input row of its step, the phase of the step it runs in, and the ring that needs
__host__ __device__ constexpr int ds_delay(int phases, int k) { return phases == 1 ? 2 * k - 1 : k; }
__host__ __device__ constexpr int ds_phase(int phases, int k) { return phases == 1 ? 0 : k - 1; }
__host__ __device__ constexpr int ds_rows(int phases) { return ds_delay(phases, 5) + 3; }     // rows r - delay(5) - 1 .. r + 1
static_assert(ds_rows(1) == 12 && ds_rows(5) == 8, "the ring sizes the header comment states");

constexpr int DS_OVER = (DS_NT - 1) * 16;       // slots behind the last plane that a wave's tiles beyond the row may read
__host__ __device__ constexpr int64_t ds_row_slots(int64_t W) { return (W + 15) / 16 * 16 + 2; }
constexpr int64_t ds_plane_slots(int rows, int64_t W) { return (rows * ds_row_slots(W) + 15) / 16 * 16; }
constexpr int64_t ds_need(int rows, int64_t W) { return (ds_plane_slots(rows, W) * DB_PLANES + DS_OVER) * 16; }
// the widest image of the one-phase schedule, and of the kernel
constexpr int ds_widest(int rows) { int w = 0; while (ds_need(rows, w + 1) <= sr_ctx::MAX_LDS_BYTES) ++w; return w; }
constexpr int DS_W1 = ds_widest(ds_rows(1)), DS_WMAX = ds_widest(ds_rows(5));
static_assert(DS_W1 == 64 && DS_WMAX == 96 && ds_need(ds_rows(1), DS_W1) <= sr_ctx::MAX_LDS_BYTES && ds_need(ds_rows(1), DS_W1 + 1) > sr_ctx::MAX_LDS_BYTES &&
              ds_need(ds_rows(5), DS_WMAX) <= sr_ctx::MAX_LDS_BYTES && ds_need(ds_rows(5), DS_WMAX + 1) > sr_ctx::MAX_LDS_BYTES, "the widths the header comment states");
// a step's row prefetch: 8 W slots of input in two passes of the workgroup, 4 W slots of growth planes in one
static_assert(8 * DS_WMAX <= 2 * DS_THREADS && 4 * DS_WMAX <= DS_THREADS, "row prefetch covers the widest row");

int ds_phases(int64_t W) { return W < 1 || W > DS_WMAX ? 0 : W <= DS_W1 ? 1 : 5; }

// The launch's dynamic LDS.  The five-phase ring is smaller than the widest one-phase ring for every W; it asks for that much anyway, so that the size never
// falls as W grows (one workgroup per CU either way: 8 waves of up to 256 registers).
int64_t ds_lds_bytes(int G, int64_t W) {
    const int ph = ds_phases(W);
    if (G != DB_G || !ph) return -1;
    return ph == 1 ? ds_need(ds_rows(1), W) : std::max(ds_need(ds_rows(5), W), ds_need(ds_rows(1), DS_W1));
}

int ds_auto_bands(int64_t B, int H, int cus) {
    if (B >= cus) return 1;
    const int64_t want = cus / B;          // rounded down: no workgroup gets a second item
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, H / DS_MIN_BAND));
}
__host__ __device__ inline int ds_band_y0(int band, int nbands, int H) { return (int)((int64_t)band * H / nbands); }

// One row of one conv over DS_NT tiles: acc[j] += W . x, taps outer, chunks inner.  A group is the DS_NT pixel fragments of one (tap, chunk); the fragments of
// group g + DS_AHEAD are requested before the MFMAs of group g (left to itself, hipcc reads each fragment right in front of the MFMA that takes it, and every
// MFMA waits out an LDS read; a whole tap ahead spills).
constexpr int DS_AHEAD = 2;
template <int NC>
__device__ __forceinline__ void ds_row_mma(const slot_t* base, int np, const int (&rb)[3], const slot_t (&wr)[27], f32x4 (&acc)[DS_NT]) {
    slot_t x[DS_AHEAD + 1][DS_NT];
    auto request = [&](int g) {
        const int tap = g / NC, c = g - tap * NC, dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
        for (int j = 0; j < DS_NT; ++j) x[g % (DS_AHEAD + 1)][j] = base[c * 4 * np + rb[dy] + 16 * j + dx];
    };
#pragma unroll
    for (int g = 0; g < DS_AHEAD; ++g) request(g);
#pragma unroll
    for (int g = 0; g < 9 * NC; ++g) {
        if (g + DS_AHEAD < 9 * NC) request(g + DS_AHEAD);
        __builtin_amdgcn_sched_barrier(0);
        const int tap = g / NC, c = g - tap * NC;
#pragma unroll
        for (int j = 0; j < DS_NT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[tap * 3 + c], x[g % (DS_AHEAD + 1)][j], acc[j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

struct StreamParams : BlockParams {
    int nbands, items;       // work items = B * nbands, item = image * nbands + band
    int phases, R;
};

__global__ void __launch_bounds__(DS_THREADS) dense_block_stream_kernel(StreamParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    slot_t* lds = reinterpret_cast<slot_t*>(smem);
    const int tid = threadIdx.x, lane = tid & 63, px = lane & 15, q = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = p.H, W = p.W, Wp = (int)ds_row_slots(W), np = p.np, R = p.R, phases = p.phases;
    const int row_slots = W * 4, ntiles = (W + 15) >> 4;
    const slot_t zero = {};
    // the wave's role
    const int k = wave < 4 ? wave + 1 : 5, nb = wave < 4 ? 0 : wave - 4;
    const int nc = db_nchunks(k), delay = ds_delay(phases, k), my_phase = ds_phase(phases, k), last_delay = ds_delay(phases, 5);
    slot_t wr[27];
    {
        const slot_t* wf = reinterpret_cast<const slot_t*>(p.w) + ((size_t)db_frag0(k) + nb) * 64 + lane;
        const int fstride = (k < 5 ? 1 : 4) * 64;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int c = 0; c < 3; ++c) wr[tap * 3 + c] = c < nc ? wf[(tap * nc + c) * fstride] : zero;
    }
    const f32x4 biasv = k < 5 ? *reinterpret_cast<const f32x4*>(p.bias + (k - 1) * 16 + 4 * (q & 1)) : *reinterpret_cast<const f32x4*>(p.bias + 64 + nb * 16 + 4 * q);
    const float alpha = p.alpha, beta1 = p.beta1, beta2 = p.beta2;
    const bool has_so = p.so != nullptr, x_first = p.x_skip == 1;

    for (int it = blockIdx.x; it < p.items; it += gridDim.x) {
        const int64_t img = it / p.nbands;
        const int band = it - (int)img * p.nbands;
        const int y0 = ds_band_y0(band, p.nbands, H), y1 = ds_band_y0(band + 1, p.nbands, H);
        const int lo_in = max(0, y0 - DS_HALO), hi_in = min(H, y1 + DS_HALO);                       // input rows the band needs
        const int lo = k < 5 ? max(0, y0 - (5 - k)) : y0, hi = k < 5 ? min(H, y1 + (5 - k)) : y1;   // rows of this wave's conv the band needs
        // (the barrier that ended the previous item's last step: every read of the ring is done)
        for (int s = tid; s < DB_PLANES * np + DS_OVER; s += DS_THREADS) lds[s] = zero;
        __syncthreads();
        // step y0 - 6 only brings in the first row
        for (int r = y0 - DS_HALO - 1; r <= y1 - 1 + last_delay; ++r) {
            // row r + 1 on its way: no conv of this step reads the ring row it replaces
            const int rn = r + 1;
            slot_t pre[2] = {zero, zero};
            if (rn >= lo_in && rn < hi_in) {
                const slot_t* gin = reinterpret_cast<const slot_t*>(p.in) + (img * H + rn) * 3 * row_slots;     // chunks 0 and 1 of a row are adjacent
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int u = tid + DS_THREADS * i;
                    if (u < 2 * row_slots) pre[i] = gin[u];
                }
            }
            for (int ph = 0; ph < phases; ++ph) {
                const int y = r - delay;
                if (ph == my_phase && y >= lo && y < hi) {
                    const int rb0 = (y - 1 + 2 * R) % R * Wp, rb1 = (y + 2 * R) % R * Wp, rb2 = (y + 1 + 2 * R) % R * Wp;
                    for (int t0 = 0; t0 < ntiles; t0 += DS_NT) {
                        int xs[DS_NT];
                        f32x4 acc[DS_NT];
#pragma unroll
                        for (int j = 0; j < DS_NT; ++j) {
                            xs[j] = (t0 + j) * 16 + px;
                            acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
                        }
                        const int rb[3] = {rb0, rb1, rb2};
                        // conv5: first element of the lane's four couts in out and in so, per tile + 32 xs; the other skip is requested now and used after the MFMAs
                        const int64_t e0 = ((img * H + y) * 3 + (nb >> 1)) * (int64_t)(W * 32) + 16 * (nb & 1) + 4 * q;
                        bf16x4 sov[DS_NT] = {};
                        if (k == 5 && has_so) {
#pragma unroll
                            for (int j = 0; j < DS_NT; ++j)
                                if (xs[j] < W) sov[j] = *reinterpret_cast<const bf16x4*>(p.so + e0 + xs[j] * 32);
                        }
                        // (a partial tile reads the zeros behind the row, a tile beyond the row what follows it: neither is stored)
                        const slot_t* base = lds + q * np + t0 * 16 + px;
                        if (nc == 2) ds_row_mma<2>(base, np, rb, wr, acc);
                        else ds_row_mma<3>(base, np, rb, wr, acc);
                        if (k < 5) {
                            // lanes q = 0, 1 hold couts 4 q .. 4 q + 3; q = 2, 3 the padding
                            const bool to_mem = p.store_growth && y >= y0 && y < y1;      // every row is in one band
#pragma unroll
                            for (int j = 0; j < DS_NT; ++j) {
                                if (q < 2 && xs[j] < W) {
                                    const bf16x4 o = db_growth_epilogue(acc[j], biasv);
                                    reinterpret_cast<bf16x4*>(lds)[((8 + (k - 1)) * np + rb1 + xs[j] + 1) * 2 + q] = o;
                                    if (to_mem) *reinterpret_cast<bf16x4*>(p.grow + ((img * H + y) * 3 + 2) * (int64_t)(W * 32) + xs[j] * 32 + 8 * (k - 1) + 4 * q) = o;
                                }
                            }
                        } else {
                            // couts 16 nb + 4 q .. + 3: chunk nb >> 1 of the output; in the ring plane 2 nb + (q >> 1), half q & 1
#pragma unroll
                            for (int j = 0; j < DS_NT; ++j) {
                                if (xs[j] < W) {
                                    const int64_t e = e0 + xs[j] * 32;
                                    const bf16x4 xsk = reinterpret_cast<const bf16x4*>(lds)[((2 * nb + (q >> 1)) * np + rb1 + xs[j] + 1) * 2 + (q & 1)];
                                    *reinterpret_cast<bf16x4*>(p.out + e) = db_conv5_epilogue(acc[j], biasv, xsk, has_so ? sov[j] : xsk, has_so, x_first, alpha, beta1, beta2);
                                }
                            }
                        }
                    }
                }
                if (ph == phases - 1) {
                    // row r + 1 into its ring row: channels [0, 64) (zeros where the band does not need the row), and zeros in the growth planes
                    const int rbn = (rn + 2 * R) % R * Wp;
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int u = tid + DS_THREADS * i;
                        if (u < 2 * row_slots) {
                            const int c = u >= row_slots ? 1 : 0, within = u - c * row_slots;
                            lds[(c * 4 + (within & 3)) * np + rbn + (within >> 2) + 1] = pre[i];
                        }
                    }
                    if (tid < row_slots) {
                        const int g = tid / W;
                        lds[(8 + g) * np + rbn + (tid - g * W) + 1] = zero;
                    }
                }
                __syncthreads();
            }
        }
    }
}

}  // namespace

extern "C" int64_t sr_dense_block_stream_lds_bytes(int growth_channels, int W) { return ds_lds_bytes(growth_channels, W); }

extern "C" int sr_dense_block_stream_bands(int B, int H, int num_cus, int32_t* y0_out, int cap) {
    if (B < 1 || H < 1 || num_cus < 1) return -1;
    const int n = ds_auto_bands(B, H, num_cus);
    if (y0_out) {
        if (cap < n) return -1;
        for (int b = 0; b < n; ++b) y0_out[b] = ds_band_y0(b, n, H);
    }
    return n;
}

int block_stream_launch(sr_ctx* ctx, const BlockWeights& w, TensorView in, int B, int H, int W, TensorView out, TensorView skip_o, float alpha, float beta1,
                        float beta2, int x_skip, int store_growth, hipStream_t st) {
    const int64_t lds = ds_lds_bytes(DB_G, W);
    if (!w.w || lds <= 0 || B <= 0 || H <= 0) return ctx->fail(SR_ERR_INVALID, "streamed dense block: the row ring does not fit (sr_dense_block_stream_lds_bytes)");
    if (int rc = db_check_blocked_views(ctx, "streamed dense block", in, out, skip_o, x_skip)) return rc;
    const int nbands = ctx->block_stream_bands > 0 ? std::min(ctx->block_stream_bands, H) : ds_auto_bands(B, H, ctx->cu_count());
    if ((int64_t)B * nbands >= ((int64_t)1 << 31)) return ctx->fail(SR_ERR_INVALID, "streamed dense block: too many work items");
    StreamParams p;
    p.phases = ds_phases(W); p.R = ds_rows(p.phases);
    db_fill_params(p, in.p, out.p, skip_o.p, w.w, w.bias, B, H, W, (int)ds_plane_slots(p.R, W), alpha, beta1, beta2, x_skip, store_growth);
    p.nbands = nbands; p.items = B * nbands;
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_stream_kernel), (int)lds)) return rc;
    const int rec = db_prof_open(ctx, "dense_block_stream<bf16,g8>", B, H, W, 64.0 + 64.0 + (skip_o.p ? 64.0 : 0.0) + (store_growth ? 32.0 : 0.0), st);
    hipLaunchKernelGGL(dense_block_stream_kernel, dim3(db_grid(ctx, p.items)), dim3(DS_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
