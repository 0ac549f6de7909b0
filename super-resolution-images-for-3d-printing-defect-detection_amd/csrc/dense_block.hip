// dense_block.hip -- the LDS-resident G = 8 dense block on sr_forward's row-blocked buffers: the host packer of a model's blocks and the launcher.  The layouts, the
// kernel body and the why of both: dense_block_lds.h.
#include "dense_block_lds.h"

extern "C" int64_t sr_dense_block_lds_bytes(int growth_channels, int H, int W) { return db_lds_bytes(growth_channels, H, W); }

// k[i], b[i]: HWIO kernel [3][3][64 + 8 i][8] (i < 4) / [3][3][96][64] (i = 4) and bias of conv i + 1, into the forward fragments and the bias table
int block_pack_weights(sr_ctx* ctx, const float* const k[5], const float* const b[5], BlockWeights* out) {
    std::vector<uint16_t> packed((size_t)DB_FRAGS * 64 * 8, 0);
    std::vector<float> bias(DB_BIAS, 0.f);
    for (int f = 0; f < DB_FRAGS; ++f) {
        const DbFrag fr = db_frag_decode(f);
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 8; ++j)
                if (const int s = db_frag_src(fr, l, j); s >= 0) packed[((size_t)f * 64 + l) * 8 + j] = f32_to_bf16_rne(k[fr.k - 1][s]);
    }
    for (int i = 0; i < DB_BIAS; ++i)
        if (const int c = db_bias_conv(i)) bias[i] = b[c - 1][db_bias_src(i)];
    out->bytes = packed.size() * sizeof(uint16_t);
    return weights_upload(ctx, packed.data(), out->bytes, bias.data(), DB_BIAS, DB_BIAS, &out->w, &out->bias);
}

int block_launch(sr_ctx* ctx, const BlockWeights& w, TensorView in, int B, int H, int W, TensorView out, TensorView skip_o, float alpha, float beta1,
                 float beta2, int x_skip, int store_growth, hipStream_t st) {
    const int64_t lds = db_lds_bytes(DB_G, H, W);
    if (!w.w || lds <= 0 || B <= 0) return ctx->fail(SR_ERR_INVALID, "LDS-resident dense block: the image does not fit (sr_dense_block_lds_bytes)");
    if (int rc = db_check_blocked_views(ctx, "LDS-resident dense block", in, out, skip_o, x_skip)) return rc;
    BlockParams p;
    db_fill_params(p, in.p, out.p, skip_o.p, w.w, w.bias, B, H, W, (int)(lds / (DB_PLANES * 16)), alpha, beta1, beta2, x_skip, store_growth);
    if (int rc = ctx->ensure_dyn_lds(reinterpret_cast<const void*>(&dense_block_lds_kernel<BlockParams>), (int)lds)) return rc;
    const int rec = db_prof_open(ctx, "dense_block_lds<bf16,g8>", B, H, W, 64.0 + 64.0 + (skip_o.p ? 64.0 : 0.0) + (store_growth ? 32.0 : 0.0), st);
    hipLaunchKernelGGL(dense_block_lds_kernel<BlockParams>, dim3(db_grid(ctx, B)), dim3(DB_THREADS), (size_t)lds, st, p);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
