// dense_plan.h -- the schedule of the fused dense-block kernels (dense_fused.hip), written down ONCE as plain constexpr C++17 without HIP.  The
// kernels take every piece list, stage list, buffer count and counted-wait immediate from here, chain_pack_weights packs in frag_at()'s order, and
// tests/dense_plan_dump.cpp prints the tables for the CPU model checks (tests/test_loader_schedule_cpu.py, test_operand_prefetch_schedule_cpu.py).
#pragma once

namespace dense_plan {

constexpr int ROWB = 3072;             // one LDS / HBM row of a chunk: 48 pixels x 64 B
constexpr int NSTG = 11;               // staged rows per chunk: stream rows [8s-2, 8s+9)
constexpr int STGB = NSTG * ROWB;
constexpr int WINR = 10;               // ring rows of layer 0's output: [8s-2, 8s+8)
constexpr int NCOMP = 8, NLOAD = 4;    // compute waves (one stream row each) + loader waves (LDS-DMA issue only), one loader per SIMD
constexpr int WDEPTH = 3, NWQ = 6;     // a compute wave requests the weight fragment of stage k + WDEPTH ahead of stage k's MFMAs; wq is indexed by stage modulo NWQ

// EXT: external 32-channel chunks both convs read; NB0 / NB1: 16-cout blocks of layer 0 / layer 1.
// MODE 0: both layers are growth convs (ReLU) whose outputs go to chunks EXT and EXT+1 of the source buffer.
// MODE 1: layer 0 is a growth conv kept on chip only, layer 1 is the block tail (NB1 = 4).
template <int NB0, int NB1, int MODE> struct ChainLds {
    static constexpr int WSLOT = (NB0 + NB1) * 3 * 1024;
    // Tail: two staging buffers (next chunk's rows fly during this chunk), three weight slots (the loaders' DMA runs two granules
    // ahead).  Growth pairs: their weights are register-resident in the loader waves (ds_write, one granule ahead: two slots), which
    // frees the room for a THIRD staging buffer -- rows are requested two chunks ahead, so a row piece has a whole chunk (~7 k
    // cycles) more than HBM's latency to land before anybody waits for it.
    static constexpr int NSB = MODE == 0 ? 3 : 2;
    static constexpr int NWS = MODE == 0 ? 2 : 3;
    static constexpr int BYTES = NSB * STGB + WINR * ROWB + NWS * WSLOT + (NB0 + NB1) * 16 * 4;
};

// What loader wave LW issues where and what it then waits with, as compile-time functions of the granule position in a step (chain2_kernel's
// loader section).  A step has NGR granules: (chunk, kx) for the EXT external chunks (positions [0, EXTG)), then layer 1's three kx on the ring.
template <int EXT, int NB0, int NB1, int MODE, int LW> struct LoaderPlan {
    using L = ChainLds<NB0, NB1, MODE>;
    static constexpr int NBT = NB0 + NB1, EXTG = 3 * EXT, NGR = 3 * (EXT + 1);
    static constexpr int RT_E = MODE == 1 ? 2 : 3;      // resident pieces per loader of an external granule's ceil(3 NBT / 4) = 5 (tail) / 3 (growth pair)
    static constexpr int RT_R = 2;                      // ... of a ring granule's ceil(3 NB1 / 4) = 3 / 2
    static constexpr int WL = L::NWS - 1;               // weights run WL granules ahead
    static constexpr int SL = L::NSB - 1;               // rows run SL chunks ahead
    // row(kx, r): the r-th row of a chunk requested in the chunk's granule kx, -1 past the end: {LW, LW + 4} | {8 + LW} (LW < 3) | {}
    static constexpr int row(int kx, int r) { return kx == 0 ? (r == 0 ? LW : r == 1 ? LW + 4 : -1) : kx == 1 && r == 0 && LW < 3 ? 8 + LW : -1; }
    static constexpr int nrows(int kx) { return (row(kx, 0) >= 0) + (row(kx, 1) >= 0); }
    // row pieces requested at granule position i of a step (any integer: the pattern repeats every step)
    static constexpr int nst_at(int i) {
        i = (i % NGR + NGR) % NGR;
        return i < EXTG ? 3 * nrows(i % 3) : 0;
    }
    // 1 KiB weight pieces of the granule at position iw: loader LW owns pieces LW, LW + 4, ...; its first RT_E (RT_R) are resident, the others DMA'd
    static constexpr int npieces(int iw) { return iw < EXTG ? NBT * 3 : NB1 * 3; }
    static constexpr bool resident(int iw, int k) { return k / NLOAD < (iw < EXTG ? RT_E : RT_R); }
    static constexpr int nwdma(int iw) {
        int n = 0;
        for (int k = LW; k < npieces(iw); k += NLOAD)
            if (!resident(iw, k)) ++n;
        return n;
    }
    // The vmcnt count behind the issues of granule position i.  Order of issue: weights of granule G+WL (position issue_w(i)), then this granule's
    // rows.  vmcnt retires in order.  The barrier that ends the iteration publishes the weights of granule G+1 (issued first in the PREVIOUS
    // iteration) and, after a chunk's third granule, all of the next chunk's rows (issued in its first two).  Tail: leave in flight this
    // iteration's pieces and -- except in a third granule -- the previous iteration's rows (younger than its weights).  Growth pairs (no weight
    // DMA, rows two chunks ahead): everything older than three iterations has landed.
    static constexpr int issue_w(int i) { return (i + WL) % NGR; }
    static constexpr int wait_rows(int i) {
        if (MODE == 0) return nst_at(i) + nst_at(i - 1) + nst_at(i - 2);
        const bool third = i < EXTG && i % 3 == 2;
        return nst_at(i) + (third ? 0 : nst_at(i - 1));
    }
    static constexpr int wait_n(int i) { return nwdma(issue_w(i)) + wait_rows(i); }
    static_assert(MODE == 1 || (RT_E * NLOAD >= NBT * 3 && RT_R * NLOAD >= NB1 * 3), "growth pairs: every weight piece is resident (no weight DMA in the counted waits)");
    static_assert(SL <= EXT, "rows run at most one step ahead");
};

// Which operands of a granule its predecessor has already requested (chain2_kernel's compute waves, "one continuous pipeline").  Weights: the first WDEPTH
// fragments, from the next weight slot.  Pixels: row 0 of the next granule -- only where that row is already published and is not rewritten during the
// following iteration:
//   kx -> kx + 1 inside an external chunk: the same staging buffer; ring kx 0 -> 1 -> 2: the same ring rows;
//   chunk c -> c + 1: growth pairs only (three staging buffers, rows published a chunk early); the tail's next chunk is published by the very barrier in between;
//   never into a step's first granule or into ring kx = 0 (behind the bias re-initialisation / the layer-0 epilogue that has just written the ring row).
// tests/test_operand_prefetch_schedule_cpu.py replays this against the loaders' schedule.
template <int EXT, int MODE, bool CARRY> struct CarryPlan {
    static constexpr int EXTG = 3 * EXT, NGR = 3 * (EXT + 1);
    // by granule position i of a step: external granule i = 3 * chunk + kx for i < EXTG, ring kx = i - EXTG behind them
    static constexpr bool pre_w(int i) { return CARRY && i > 0 && i < NGR && i != EXTG; }
    static constexpr bool pre_x(int i) { return pre_w(i) && (i > EXTG || i % 3 != 0 || MODE == 0); }
    // the pre-reads in flight across the barrier that opens position i (a weight fragment is one LDS read, a row three): the compute waves' counted lgkmcnt
    static constexpr int npre(int i) { return (pre_w(i) ? WDEPTH : 0) + (pre_x(i) ? 3 : 0); }
};
// MODE 1 (tail): carried.  MODE 0 (growth pairs): not carried -- their weight slot of granule G + 1 is written during granule G (two slots, one granule
// ahead); the first fragments would need a three-buffer ring of their own, and the skeleton shows nothing to gain at their granule sizes.
template <int MODE> constexpr bool kCarry = MODE == 1;

// Stage lists of a compute wave: one weight fragment x three column groups per stage, stage k uses the granule's weight fragment k.
// External granule (chunk, kx) on a staged chunk: staged row j holds stream row 8s-2+j; layer 0 (row 8s+w) reads j = w+1+ky, layer 1 (row 8s+w-1) reads
// j = w+ky.  Stage order: row d = 0..3: [layer 0, ky = d-1 (d >= 1)] [layer 1, ky = d (d <= 2)], every cout block n of a layer in turn; `first`: the
// row's first stage.
struct ExtStage { int d, layer, n, first; };
constexpr int ext_stages(int nb0, int nb1) { return 3 * (nb0 + nb1); }
constexpr ExtStage ext_stage(int nb0, int nb1, int k) {
    const int d = (k + nb0) / (nb0 + nb1), r = (k + nb0) % (nb0 + nb1);      // (as if row 0 had layer-0 stages too)
    return r < nb0 ? ExtStage{d, 0, r, r == 0} : ExtStage{d, 1, r - nb0, d == 0 && r == nb0};
}
// Ring granule kx (layer 1 on layer 0's output): ring rows ky = 0..2, every cout block in turn.
struct RingStage { int ky, n; };
constexpr int ring_stages(int nb1) { return 3 * nb1; }
constexpr RingStage ring_stage(int nb1, int k) { return RingStage{k / nb1, k % nb1}; }
static_assert(WDEPTH < NWQ, "a stage's wq entry must not be requested again while it is live");

// The packed weights (chain_pack_weights), fragment by fragment: granule after granule in the order of a step -- external (chunk, kx), then the ring's
// kx on conv 1's last chunk (= conv 0's output) -- and inside a granule in stage order: for an external granule, row by row of the four staged rows a
// wave walks, [1: ky 0][0: ky 0][1: ky 1][0: ky 1][1: ky 2][0: ky 2], every cout block of a conv in turn.  conv: 0 = layer 0's conv, 1 = layer 1's.
struct Frag { int conv, chunk, ky, kx, blk; };
constexpr int nfrags(int ext, int nb0, int nb1) { return 3 * ext * ext_stages(nb0, nb1) + 3 * ring_stages(nb1); }
constexpr Frag frag_at(int ext, int nb0, int nb1, int f) {
    const int per = ext_stages(nb0, nb1);
    if (f < 3 * ext * per) {
        const int g = f / per;
        const ExtStage st = ext_stage(nb0, nb1, f % per);
        return Frag{st.layer, g / 3, st.layer == 0 ? st.d - 1 : st.d, g % 3, st.n};
    }
    const int r = f - 3 * ext * per;
    const RingStage st = ring_stage(nb1, r % ring_stages(nb1));
    return Frag{1, ext, st.ky, r / ring_stages(nb1), st.n};
}

// ---- conv1_stream_kernel: unit k = (step k / 2, chunk k % 2) of a workgroup's rows goes to staging buffer k % C1_NSB
constexpr int C1_NSTG = 10;            // staged rows per chunk and step: stream rows [8s - 1, 8s + 9)
constexpr int C1_STGB = C1_NSTG * ROWB;
constexpr int C1_NSB = 4;
constexpr int C1_WBYTES = 2 * 9 * 2 * 1024;
constexpr int C1_LDS = C1_NSB * C1_STGB + C1_WBYTES + 32 * 4;
// Loader LW stages rows LW, LW + 4 and (LW < 2) 8 + LW of every unit: three 1 KiB pieces per row.  Per barrier k (the barrier that lets the compute waves
// start unit k): issue unit k + AHEAD (its buffer was released by the barrier before: unit k - 1 is done), then wait until unit k + 1 has landed = all
// but this loader's pieces of units k + 2 and k + 3.
template <int LW> struct Conv1LoaderPlan {
    static constexpr int NROWS = LW < 2 ? 3 : 2, NP = 3 * NROWS;
    static constexpr int row(int r) { return r == 0 ? LW : r == 1 ? LW + 4 : 8 + LW; }
    static constexpr int AHEAD = 3;
    static constexpr int WAIT = (AHEAD - 1) * NP;
    static_assert(AHEAD + 1 == C1_NSB, "unit k + AHEAD takes the buffer unit k - 1 has just left");
};

}  // namespace dense_plan
