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
#include "dense_block_lds.h"

// (layouts, constants and the kernel body: dense_block_lds.h -- the training kernels of dense_block_train.hip share them)

extern "C" int64_t sr_dense_block_lds_bytes(int growth_channels, int H, int W) { return db_lds_bytes(growth_channels, H, W); }

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
    const int64_t lds = db_lds_bytes(DB_G, H, W);
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
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_lds_kernel<BlockParams>), (int)lds)) return rc;
    int rec = -1;
    if (ctx->prof) {
        const double px = (double)B * H * W;
        double macs = 96.0 * 64.0;
        for (int i = 0; i < 4; ++i) macs += (64.0 + DB_G * i) * DB_G;
        rec = ctx->prof_open("dense_block_lds<bf16,g8>", 2.0 * px * 9.0 * macs, px * 2.0 * (64.0 + 64.0 + (skip_o.p ? 64.0 : 0.0) + (store_growth ? 32.0 : 0.0)), st);
    }
    hipLaunchKernelGGL(dense_block_lds_kernel<BlockParams>, dim3(grid), dim3(DB_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
