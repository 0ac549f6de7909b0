// conv_pack.h -- the packed weight layouts of the conv kernels, each stated once: conv_plan chooses a conv's kernel family and the sizes of its
// packed image, conv_pack_decode says which (tap, cin, cout) sits at a packed index, pack_source fetches it from the caller's kernel.  Host packing
// (conv_pack_weights) and device packing (pack_weights_f32_kernel, pack_weights_f32_many_kernel) all go through these three, so a model's
// forward and the training tape multiply with the same image.
//
// A fragment is the 1 KiB A operand of one MFMA step: 64 lanes x E elements, E = 16 bytes of the compute dtype.  Lane l, element j of a fragment hold
//   few        no fragments: [tap][CinP][4 couts], fp32 (conv_fewcout_*_kernel)
//   thin       [ct][g][n]:           tap 2 g + (l >> 5),  cin j,                                cout 32 (ct NT + n) + (l & 31)
//   wide       [ct][ch][tap][kg][n]: tap,                 cin 2 E (ch KGPT + kg) + E (l >> 5) + j,  cout 32 (ct NT + n) + (l & 31)
//   rows, pw   [ct][ch][tap][n]:     tap,                 cin 4 E ch + E (l >> 4) + j,           cout 16 (ct NT + n) + (l & 15)      (bf16: 32 cins per chunk)
// and zero wherever tap, cin or cout lies beyond the kernel's own.
#pragma once
#include "common.h"

enum { PL_FEW = 0, PL_THIN = 1, PL_WIDE = 2, PL_ROWS = 3 };

// What the decoder needs.  All int: a PackJob table is compared bytewise (conv_prepack_dev), so no padding may hide in here.
struct PackPlan { int layout, esh, ntap, Cin, Cout, CinP, CoutP, NT, nchunks, KGPT, rot; };      // esh = log2 E
static_assert(sizeof(PackPlan) == 11 * sizeof(int), "PackPlan: no padding");
struct PackCoord { int tap, ci, co; };

// The one place that chooses family, NT, KGPT, CinP, CoutP, nchunks, element size and packed element count of a conv.  Fills the metadata of `out`
// (no allocation: w and bias stay null) and the decoder's plan.  rot = 1: the source is the kernel whose 180-degree-rotated, channel-swapped form is
// packed (pack_source).  rows_head = 1 (bf16 3x3 only): an RGB head goes to the row-sliding kernel on one zero-padded 32-channel chunk.
inline int conv_plan(sr_ctx* ctx, int dtype, int KS, int Cin, int Cout, int rows_head, int rot, ConvWeights* out, PackPlan* plan, int64_t* count) {
    if (dtype != SR_DTYPE_BF16 && dtype != SR_DTYPE_F32) return ctx->fail(SR_ERR_INVALID, "conv: dtype must be f32 or bf16");
    if (KS != 1 && KS != 3 && KS != 5 && KS != 9) return ctx->fail(SR_ERR_INVALID, "conv: kernel size must be 1,3,5 or 9");
    const int esz = dtype_size(dtype), E = 16 / esz, ntap = KS * KS;
    ConvWeights w;
    w.dtype = dtype; w.KS = KS; w.Cin = Cin; w.Cout = Cout;
    w.CoutP = round_up(Cout, 32);
    const int nb = w.CoutP / 32;
    w.NT = (nb % 2 == 0) ? 2 : (nb % 3 == 0 ? 3 : 1);
    if (KS == 5 && !(Cin <= E)) w.NT = 1;   // 25 taps of weights: keep the LDS stage small
    const bool as_rows = rows_head && dtype == SR_DTYPE_BF16 && KS == 3;
    // thin (RGB) inputs pair two taps in a k-group; a 1x1 has no second tap and takes the wide / 1x1 kernels on zero-padded channels instead
    w.thin = Cin <= E && !as_rows && KS != 1;
    if (w.thin) w.NT = 1;                    // thin: one 32-cout block per workgroup (112 + 48 registers, 3 waves/SIMD);
                                             // re-reading the 3-channel input per cout block is cheap, 1 wave/SIMD at NT=3 was not (9x9: 1.8x)
    // fp32, <= 4 couts, not thin: the VALU kernel (conv_fewcout_f32_kernel)
    w.few = (dtype == SR_DTYPE_F32 && Cout <= 4 && !w.thin && (KS == 3 || KS == 5)) ? 1 : 0;
    w.rows = (dtype == SR_DTYPE_BF16 && KS == 3 && !w.thin) ? 1 : 0;
    // bf16 1x1 with the whole weight matrix in 16 register fragments: the streaming kernel of conv_pw.hip (the rows layout)
    {   // (register budget of the instantiations in conv_pw.hip: 4 waves/SIMD without spills)
        const int nb16 = round_up(Cout, 16) / 16, nch = round_up(Cin, 32) / 32;
        w.pw = (dtype == SR_DTYPE_BF16 && KS == 1 && !w.thin && nch <= 4 &&
                (nb16 <= 2 || (nb16 == 3 && nch <= 3) || (nb16 == 4 && nch == 1))) ? 1 : 0;
    }
    if (!w.thin && KS == 9) return ctx->fail(SR_ERR_INVALID, "conv: 9x9 supported for <= one 16-byte channel slice only");
    int layout;
    int64_t n;                               // packed elements
    if (w.few) {
        layout = PL_FEW;
        w.CoutP = 4; w.NT = 1; w.KGPT = 0;
        w.CinP = round_up(Cin, 4);
        w.nchunks = w.CinP / 4;
        n = (int64_t)ntap * w.CinP * 4;
    } else if (w.rows || w.pw) {
        layout = PL_ROWS;
        w.CoutP = round_up(Cout, 16);
        const int nb16 = w.CoutP / 16;
        w.NT = w.pw ? nb16 : ((nb16 % 4 == 0) ? 4 : (nb16 % 2 == 0 ? 2 : 1));
        w.KGPT = 1;
        w.CinP = round_up(Cin, 32);
        w.nchunks = w.CinP / 32;
        n = (int64_t)nb16 * w.nchunks * ntap * 64 * E;
    } else if (w.thin) {
        layout = PL_THIN;
        w.CinP = E; w.KGPT = 0;
        w.nchunks = (ntap + 1) / 2;          // k-groups: two taps each
        n = (int64_t)nb * w.nchunks * 64 * E;
    } else {
        layout = PL_WIDE;
        w.KGPT = (KS == 1 && (round_up(Cin, 4 * E) * esz) % 128 == 0) ? 4 : 2;
        const int chunkE = w.KGPT * 2 * E;
        w.CinP = round_up(Cin, chunkE);
        w.nchunks = w.CinP / chunkE;
        n = (int64_t)nb * w.nchunks * ntap * w.KGPT * 64 * E;
    }
    w.bytes = (size_t)n * esz;
    *out = w;
    *plan = PackPlan{layout, E == 8 ? 3 : 2, ntap, Cin, Cout, w.CinP, w.CoutP, w.NT, w.nchunks, w.KGPT, rot};
    *count = n;
    return SR_OK;
}

// (tap, cin, cout) of lane 0, element 0 of fragment f
__host__ __device__ inline PackCoord pack_fragment_origin(int64_t f, const PackPlan& q) {
    const int nn = (int)(f % q.NT); f /= q.NT;
    if (q.layout == PL_THIN) {
        const int g = (int)(f % q.nchunks), ct = (int)(f / q.nchunks);
        return {2 * g, 0, (ct * q.NT + nn) * 32};
    }
    int kg = 0;
    if (q.layout == PL_WIDE) { kg = (int)(f % q.KGPT); f /= q.KGPT; }
    const int tap = (int)(f % q.ntap); f /= q.ntap;
    const int ch = (int)(f % q.nchunks), ct = (int)(f / q.nchunks);
    if (q.layout == PL_WIDE) return {tap, (ch * q.KGPT + kg) << (q.esh + 1), (ct * q.NT + nn) * 32};
    return {tap, ch << (q.esh + 2), (ct * q.NT + nn) * 16};
}

// ... and of element 0 of its lane l; the lane's elements j = 0 .. E - 1 are the E consecutive cins from there
__host__ __device__ inline PackCoord pack_fragment_lane(PackCoord o, int l, const PackPlan& q) {
    if (q.layout == PL_THIN) return {o.tap + (l >> 5), 0, o.co + (l & 31)};
    if (q.layout == PL_WIDE) return {o.tap, o.ci + ((l >> 5) << q.esh), o.co + (l & 31)};
    return {o.tap, o.ci + ((l >> 4) << q.esh), o.co + (l & 15)};
}

// The element order of every layout: packed index -> (tap, cin, cout)
__host__ __device__ inline PackCoord conv_pack_decode(int64_t idx, const PackPlan& q) {
    if (q.layout == PL_FEW) {
        const int64_t t = idx >> 2;
        return {(int)(t / q.CinP), (int)(t % q.CinP), (int)(idx & 3)};
    }
    PackCoord c = pack_fragment_lane(pack_fragment_origin(idx >> (q.esh + 6), q), (int)(idx >> q.esh) & 63, q);
    c.ci += (int)idx & ((1 << q.esh) - 1);
    return c;
}

// Where an element of the kernel's own sits in the source: HWIO [tap][Cin][Cout], or with rot [ntap - 1 - tap][Cout][Cin]; consecutive cins lie
// pack_source_stride apart
__host__ __device__ inline int64_t pack_source_index(PackCoord c, const PackPlan& q) {
    return q.rot ? ((int64_t)(q.ntap - 1 - c.tap) * q.Cout + c.co) * q.Cin + c.ci : ((int64_t)c.tap * q.Cin + c.ci) * q.Cout + c.co;
}
__host__ __device__ inline int pack_source_stride(const PackPlan& q) { return q.rot ? 1 : q.Cout; }

// The source value of a packed element; zero in the padding
__host__ __device__ inline float pack_source(const float* __restrict__ src, PackCoord c, const PackPlan& q) {
    return (c.tap < q.ntap && c.ci < q.Cin && c.co < q.Cout) ? src[pack_source_index(c, q)] : 0.f;
}
