/* sr355.h -- C ABI of libsr355.so: the MI355X (gfx950) super-resolution + defect-classifier hot path.
 *
 * The reference (bgmanuel99/Super-Resolution-Images-for-3D-Printing-Defect-Detection) has no
 * FFI/plugin interface; its boundary to the device is the Keras call `model.predict(...)` /
 * `generator(...)` / `tf.image.psnr|ssim` / `cv2.resize`.  Each entry point below names the
 * reference call site (file:line under /root/reference) it stands in for.  The Python host
 * (package sr355, mirroring the reference's SRModels/ classes) binds these with ctypes; see
 * INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *  - return 0 (SR_OK) on success, negative sr_status on error; text via sr_last_error(ctx).
 *  - nothing throws across the ABI.
 *  - image tensors are NHWC, dense, DEVICE pointers owned by the caller (e.g. torch tensors'
 *    data_ptr()); conv kernels handed to sr_model_set_weight are HOST float32 HWIO, Dense [in,out].
 *  - all work is enqueued on `stream` (a hipStream_t passed as void*, NULL = default stream) and
 *    is asynchronous; the caller synchronises.
 *  - one sr_ctx per GPU; a ctx (and its models) is not thread-safe; different ctxs are independent.
 */
#ifndef SR355_H
#define SR355_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sr_ctx sr_ctx;
typedef struct sr_model sr_model;

typedef enum sr_status {
    SR_OK = 0,
    SR_ERR_INVALID = -1,   /* bad argument / unsupported shape                 */
    SR_ERR_HIP = -2,       /* HIP runtime error (message holds hipGetErrorString) */
    SR_ERR_OOM = -3,       /* device allocation failed                          */
    SR_ERR_STATE = -4,     /* model not finalised / weight missing              */
    SR_ERR_NAME = -5,      /* unknown layer name                                */
    SR_ERR_CAPACITY = -6   /* caller's output buffer too small                  */
} sr_status;

enum { SR_DTYPE_F32 = 0, SR_DTYPE_BF16 = 1, SR_DTYPE_U8 = 2 };
enum { SR_MODEL_SRCNN = 0, SR_MODEL_EDSR = 1, SR_MODEL_ESRGAN_G = 2, SR_MODEL_VGG16 = 3,
       SR_MODEL_ESRGAN_D = 4,          /* discriminator, inference graph (ESRGAN_model.py:347-377): [B,H,W,3] in [-1,1] -> [B,1] probabilities */
       SR_MODEL_VGG19_FEATURES = 5 };  /* perceptual-loss extractor incl. preprocessing (ESRGAN_model.py:379-408): -> [B,H/16,W/16,512]     */
enum { SR_ACT_LINEAR = 0, SR_ACT_RELU = 1, SR_ACT_LRELU = 2, SR_ACT_TANH = 3 };
enum { SR_WEIGHT_KERNEL = 0, SR_WEIGHT_BIAS = 1 };
/* sr_eltwise ops: out = alpha*a + beta*b | dy where y > 0 | dy (0.2 dy where y <= 0) | dy where 0 <= x <= 1 | alpha*a*b | dy*(1 - y^2) |
 * clip(a, 0, 1) | alpha * sign(a - b) */
enum { SR_ELT_AXPBY = 0, SR_ELT_RELU_BWD = 1, SR_ELT_LRELU_BWD = 2, SR_ELT_CLIP01_BWD = 3, SR_ELT_MUL = 4, SR_ELT_TANH_BWD = 5, SR_ELT_CLIP01 = 6,
       SR_ELT_SIGN_DIFF = 7 };

/* Architecture hyper-parameters = the keyword arguments of the reference's setup_model():
 * SRCNN_model.py:23, EDSR_model.py:29, ESRGAN_model.py:108, VGG16_model.py:21. */
typedef struct sr_model_cfg {
    int32_t compute_dtype;    /* SR_DTYPE_F32 (reference precision) or SR_DTYPE_BF16 (fp32 accumulate) */
    int32_t scale_factor;     /* EDSR: 2,3,4; ESRGAN: 2,4,8; ignored otherwise                         */
    int32_t channels;         /* image channels (3)                                                    */
    int32_t num_blocks;       /* EDSR num_res_blocks / ESRGAN num_rrdb_blocks                          */
    int32_t num_filters;      /* EDSR num_filters (ESRGAN trunk is fixed at 64)                        */
    int32_t growth_channels;  /* ESRGAN growth_channels                                                */
    float   res_scaling;      /* EDSR res_scaling                                                      */
    int32_t num_classes;      /* VGG16 classifier head width                                           */
    int32_t use_attention;    /* ESRGAN: 1 = reference graph (two SelfAttention layers); 0 = tuning-only variant */
} sr_model_cfg;

/* ---- context ------------------------------------------------------------------------------ */
int  sr_init(int device_id, sr_ctx** out);
void sr_destroy(sr_ctx* ctx);
const char* sr_last_error(sr_ctx* ctx);
/* bytes of device memory the library currently holds / has held at most (weights + workspaces).
 * Feeds the reference's inference_metrics keys gpu_mean_current_mb / gpu_peak_mb
 * (SRCNN_model.py:201-242, tf.config.experimental.get_memory_info). */
int  sr_mem_info(sr_ctx* ctx, int64_t* current_bytes, int64_t* peak_bytes);
/* wall-clock of the last sr_forward on this ctx measured with HIP events on its stream (ms);
 * blocks until that forward has finished. */
int  sr_last_forward_ms(sr_ctx* ctx, float* ms);

/* Shader clock (MHz) the GPU holds under a dense bf16 MFMA load, measured in-kernel (s_memtime / s_memrealtime around an
 * MFMA loop, ~0.3 s of load first).  bench.py prices the MFMA roof at this clock beside the nominal peak -- the reference
 * has no counterpart (it never names its hardware).  Blocks until measured. */
int  sr_measure_clock(sr_ctx* ctx, float* mhz, void* stream);

/* Per-launch timing of the hot kernels with HIP events recorded on the launching stream (the
 * reference's analogue is its time.perf_counter() bracket around predict, SRCNN_model.py:208-212).
 * begin: start collecting; end: synchronise the device and write a JSON array
 * [{"kernel","launches","total_ms","flops","bytes"}...] (algorithmic FLOP / HBM bytes per kernel
 * template instance) into `json` (capacity `cap` bytes). */
/* Diagnostic only (never set in production): a device buffer of 16 uint64 per workgroup of the next 3x3 bf16 conv
 * launches; a separately compiled stamped variant of the kernel writes s_memtime stamps there (NULL switches back).
 * `capacity_bytes` is the size of that buffer: a launch whose grid would write beyond it is refused with SR_ERR_INVALID
 * instead of running (round 2's one memory fault was a probe handing a buffer sized for another kernel).
 * sr_debug_stamp_bytes_needed(0, workgroups) is the size a launch of `workgroups` workgroups needs. */
int  sr_debug_set_stamp_buffer(sr_ctx* ctx, void* device_u64_buffer, int64_t capacity_bytes);
/* Diagnostic only: a device buffer of 64 x 4 x 64 x 4 uint64 for the stamped variant of the fused dense-block kernels (s_memtime at four
 * points of each of the first 64 granules, waves 0, 5, 8, 11 of the first 64 workgroups; tools/probe_chain.py).  NULL switches back.
 * A non-NULL buffer smaller than sr_debug_stamp_bytes_needed(1, 0) is refused with SR_ERR_INVALID. */
int  sr_debug_set_chain_stamp_buffer(sr_ctx* ctx, void* device_u64_buffer, int64_t capacity_bytes);
/* Bytes of stamp buffer the stamped diagnostic kernels write: which = 0 -> the 3x3 conv (16 uint64 per workgroup of the launch),
 * which = 1 -> the fused dense-block kernels (fixed size; `workgroups` ignored).  Pure function, no context; -1 for anything else. */
int64_t sr_debug_stamp_bytes_needed(int which, int64_t workgroups);
/* Which dense-block conv pairs of the ESRGAN trunk run as one fused line-buffer kernel when the shape allows (bf16, 32 growth
 * channels, images 48 pixels wide, or 24 wide with two images per 48-pixel row when bits 0, 1 and 5 are all set): bit 0 = conv4+conv5, bit 1 = conv2+conv3; bit 2 = the generator's last conv (64 -> image channels,
 * ESRGAN_model.py:341) computed inside final_conv1's epilogue, so that final_conv1's 64-channel output is never stored; bit 3 = the three
 * 1x1 projections that open a SelfAttention layer (ESRGAN_model.py:48-56) computed in the epilogue of the conv producing its input; bit 4 = batches of small
 * images (the VGG16 classifier's block 5: 6 x 6 pixels for 96-pixel patches) packed side by side with zero separator rows / columns into one
 * tall image for the 3x3 kernel, whose 12 x 16 output tiles a single such image would fill to 19 %; bit 5 = conv1 of a dense block (64 -> 32 channels, the block's one
 * HBM-bound conv) on a streaming line-buffer kernel with its weights resident in LDS; bit 6 = a MaxPooling2D computed in the epilogue of the conv in front of it
 * (every VGG16 block ends conv -> pool: the full-resolution tensor is never stored); bit 7 = 3x3 convs from 64 input channels (the generator's
 * up-sampling convs, EDSR's body) on a persistent kernel that keeps a 64-cout tile's weights in LDS; bit 8 = SRCNN's 1x1 conv (conv2d_1, 96 -> 32, ReLU:
 * SRCNN_model.py:51) computed from the accumulators in the epilogue of the 9x9 head, whose 96-channel fp32 output is then never stored; default 511.
 * mask 0 = layer by layer (the A/B switch of the parity tests and of tools/ benchmarks).  max_workgroups > 0 caps the persistent grid (tests: several images per workgroup
 * at small batches); 0 = one workgroup per CU.
 * At 8 growth channels (bf16; the reference notebook's generator) bits 0, 1 and 5 together -- the bits that mean "the whole dense block on fused kernels" -- run every
 * dense block as ONE kernel whose 96-channel concat tensor lives in LDS (dense_block_lds<bf16,g8>), for every image sr_dense_block_lds_bytes accepts (24 x 24 patches
 * among them); without one of the three, or for a larger image, the block runs conv by conv as before.  max_workgroups caps that kernel's grid too. */
int  sr_debug_set_fused(sr_ctx* ctx, int mask, int max_workgroups);
/* Dynamic LDS bytes the LDS-resident dense-block kernel needs for one H x W image of a generator with `growth_channels` growth channels (the padded (H + 2) x (W + 2)
 * image of 96 bf16 channels, in whole 256-byte bank rows per 8-channel plane), or -1 where that kernel does not apply: growth_channels != 8, H or W < 1, or more than
 * the 160 KiB of a CU.  Every H, W with (H + 2)(W + 2) <= 676 fits.  Pure function, no context: sr_forward's router and the kernel's launcher both ask it. */
int64_t sr_dense_block_lds_bytes(int growth_channels, int H, int W);
/* The streamed dense-block kernel (dense_block_stream<bf16,g8>): the same block as ONE kernel for images too large to be LDS-resident, their rows streamed through a
 * ring in LDS (ESRGAN.super_resolve_image's default 48 x 48 patches).  Any height; the ring sets the width.
 * sr_dense_block_stream_lds_bytes: the dynamic LDS of the ring for images W pixels wide, or -1 where the kernel does not apply: growth_channels != 8, W < 1, or
 *   more than the 160 KiB of a CU at the smallest ring (8 rows).  Every W <= 96 fits; never falls as W grows.  Pure, no context: router, launcher and tests ask it.
 * sr_dense_block_stream_bands: a work item of the kernel is (image, band of consecutive output rows); halo rows are recomputed, nothing is exchanged.  Returns the
 *   band count for B images of H rows on num_cus CUs -- 1 when B >= num_cus, else as many bands as leave every (image, band) a CU of its own, none shorter than 3 rows -- and, with y0_out
 *   not NULL, writes each band's first row (band b ends where b + 1 starts, the last at H).  -1 for B, H or num_cus < 1, or when `cap` entries do not hold
 *   the bands (nothing is written).  Pure.  The result of a forward does not depend on the band count.
 * sr_model_set_dense_block_stream: when a forward of this model takes the kernel, under the conditions of the resident kernel (mask bits 0, 1 and 5).  mode 0, the
 *   default: never.  1: where the resident kernel does not fit and the ring does.  2: wherever the ring fits, also in place of the resident kernel (diagnostic).
 *   SR_ERR_INVALID for another mode, or for a model that is not ESRGAN_G / bf16 / 8 growth channels on row-blocked concat buffers.
 * sr_debug_set_block_stream_bands: test hook.  n = 0: automatic; n > 0: that many bands (at most H). */
int64_t sr_dense_block_stream_lds_bytes(int growth_channels, int W);
int  sr_dense_block_stream_bands(int B, int H, int num_cus, int32_t* y0_out, int cap);
int  sr_model_set_dense_block_stream(sr_model* m, int mode);
int  sr_debug_set_block_stream_bands(sr_ctx* ctx, int n);
/* The bits of sr_debug_set_fused's mask, as described above.  SR_FUSE_TWO_UP: the bits the two-up packing of 24-pixel-wide images needs. */
enum { SR_FUSE_DENSE_TAIL = 1, SR_FUSE_DENSE_MID = 2, SR_FUSE_RGB_TAIL = 4, SR_FUSE_ATTN_PROJ = 8, SR_FUSE_CELLS = 16, SR_FUSE_CONV1_STREAM = 32,
       SR_FUSE_POOL = 64, SR_FUSE_CONV_STREAM = 128, SR_FUSE_SRCNN_1X1 = 256, SR_FUSE_ALL = 511,
       SR_FUSE_TWO_UP = SR_FUSE_DENSE_TAIL | SR_FUSE_DENSE_MID | SR_FUSE_CONV1_STREAM };
/* Test hook: device allocations through this ctx fail (SR_ERR_OOM) once the bytes it holds would exceed `bytes`
 * (0 = no cap).  Lets the tests walk the out-of-memory path of sr_forward without filling a 288 GB card. */
int  sr_debug_set_alloc_cap(sr_ctx* ctx, int64_t bytes);
/* Test hook: the kernel variant every conv launch on this ctx runs, one name per line (e.g. "wide<f32,k3,kg2,nt2>/sk", "pw<bf16,nb3,nch2>",
 * "rows<bf16,nb4>/skip_lds").  Copies the names logged since the previous call into `text` (NUL-terminated; SR_ERR_CAPACITY, nothing cleared,
 * when `cap` bytes do not hold them; text NULL: discarded), clears the log, and logs the launches that follow iff `enable`.  Off by default. */
int  sr_debug_conv_routes(sr_ctx* ctx, int enable, char* text, int64_t cap);
int  sr_profile_begin(sr_ctx* ctx);
int  sr_profile_end(sr_ctx* ctx, char* json, int64_t cap);

/* ---- models: replaces Keras model build + predict ------------------------------------------ */
/* Keras graph construction: SRCNN_model.py:45-53, EDSR_model.py:96-125, ESRGAN_model.py:303-345,
 * VGG16_model.py:57-97. */
int  sr_model_create(sr_ctx* ctx, int kind, const sr_model_cfg* cfg, sr_model** out);
void sr_model_destroy(sr_model* m);
/* number of parameter tensors the graph expects, and the i-th one's Keras layer name, which
 * (kernel/bias) and shape (ndim <= 4).  Lets the host enumerate what load_model() would restore. */
int  sr_model_num_params(sr_model* m);
int  sr_model_param_info(sr_model* m, int index, const char** name, int* which, int64_t shape[4], int* ndim);
/* copy one parameter (host fp32; conv HWIO, dense [in,out], bias [out]) into the model.
 * Stands in for keras load_model / set_weights (SRCNN_model.py:35, ESRGAN_model.py:143-149). */
int  sr_model_set_weight(sr_model* m, const char* keras_layer_name, int which,
                         const float* host, const int64_t* shape, int ndim);
/* pack all weights into the device MFMA layouts; must precede sr_forward. */
int  sr_model_finalize(sr_model* m);
/* Free the model's activation workspaces (they are grow-only otherwise; weights stay).  sr_forward releases them by
 * itself when growing them fails with SR_ERR_OOM, so a retry with a smaller batch starts clean -- the analogue of
 * the reference's tf.keras.backend.clear_session() between runs (defect_detection_pipeline / notebooks). */
int  sr_model_release_workspace(sr_model* m);
/* Diagnostics for stage-by-stage parity traces (tests/): the graph as a flat op list -- name = Keras layer name of a
 * conv (ESRGAN_model.py:230-341), else the op kind; the op's output is [B, h, w, channels] with h = (H*mul)>>shift then
 * ceil-halved ceil_halvings times (stride-2 SAME convs), w likewise (channels 0: no tensor output) -- and a tap that copies op `op_index`'s output, as dense fp32 NHWC, into
 * `device_dst` during every later sr_forward (NULL removes the tap).  Never set in production runs. */
int  sr_model_num_ops(sr_model* m);
int  sr_model_op_info(sr_model* m, int index, const char** name, int* channels, int* mul, int* shift, int* ceil_halvings);
int  sr_model_set_tap(sr_model* m, int op_index, float* device_dst, int64_t capacity);
/* output shape for an input of [B,H,W,C]. */
int  sr_model_output_shape(sr_model* m, int B, int H, int W, int C, int64_t out_shape[4]);
/* model.predict / generator(x): SRCNN_model.py:210, EDSR_model.py:274, ESRGAN_model.py:941,
 * VGG16_model.py:244.  x,y DEVICE NHWC of `io_dtype` (f32 or bf16; VGG16 output is [B,num_classes]).
 * y_capacity in elements. */
int  sr_forward(sr_model* m, const void* x, int io_dtype, int B, int H, int W, int C,
                void* y, int64_t y_capacity, void* stream);

/* ---- single ops (also used by the kernel-level parity tests) -------------------------------- */
/* Keras Conv2D(padding="same", strides=1) + bias + activation, then
 * y = alpha*act(conv+b) + beta1*skip1 + beta2*skip2, optional clip[0,1], optional depth_to_space(r)
 * in TF "DCR" order (EDSR_model.py:61-90, ESRGAN_model.py:230-299).  x [B,H,W,Cin], w HOST HWIO,
 * skips [B,H,W,Cout] (same dtype as x), y [B,H*r,W*r,Cout/r^2].  dtype applies to x, skips and y. */
int  sr_conv2d(sr_ctx* ctx, const void* x, int dtype, int B, int H, int W, int Cin,
               const float* w_hwio, const float* bias, int KH, int KW, int Cout, int act,
               float alpha, const void* skip1, float beta1, const void* skip2, float beta2,
               int clip01, int d2s_r, void* y, void* stream);
/* SelfAttention.call (ESRGAN_model.py:48-70) on x [B,H,W,C]; weights HOST HWIO 1x1. */
int  sr_self_attention(sr_ctx* ctx, const void* x, int dtype, int B, int H, int W, int C,
                       const float* wf, const float* bf, const float* wg, const float* bg,
                       const float* wh, const float* bh, const float* wv, const float* bv,
                       void* y, void* stream);
/* cv2.resize(..., interpolation=cv2.INTER_CUBIC) (classic_algorithms.py:11-13, SRCNN_model.py:191,
 * loading_methods.py:147).  dtype f32: float path; u8: OpenCV fixed-point path. */
int  sr_bicubic(sr_ctx* ctx, const void* x, int dtype, int B, int H, int W, int C,
                int outH, int outW, void* y, void* stream);
/* cv2.resize(x, (outW, outH), interpolation=code) with OpenCV's codes INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2,
 * INTER_AREA = 3, INTER_LANCZOS4 = 4: classic_algorithms.py:7-21 (interpolate_bilinear / _bicubic / _area / _lanczos) and the
 * per-file codes of interpolation_map.pkl in load_dataset_as_patches(mode="srcnn") (loading_methods.py:131-148, which hands an
 * integer entry of the map to cv2.resize as it is).  f32: float path; u8: OpenCV's 11-bit fixed-point path; uint8 INTER_AREA
 * shrinking: integer cell sums for whole-number factors ((sum + 2) >> 2 for 2 x 2, a rounded float product otherwise), the
 * float taps rounded half to even for the others.  Any other code: SR_ERR_INVALID.
 * The float path (f32 LINEAR / AREA / LANCZOS4, and the uint8 fractional INTER_AREA shrink before its rint) is OpenCV's two passes in
 * float: per source row the horizontal taps in ascending source order, then the vertical taps, every product and every sum rounded
 * on its own (no fused multiply-add) -- bit for bit NumPy's `acc += x * w` in that order.  The tap coordinates are fp64, likewise
 * uncontracted: d * scale, (d + 0.5) * scale - 0.5 and (d + 1) - (s + 1) * inv_scale round the product first. */
int  sr_resize(sr_ctx* ctx, const void* x, int dtype, int B, int H, int W, int C,
               int outH, int outW, int interpolation, void* y, void* stream);
/* tf.image.psnr / tf.image.ssim(max_val) (metrics.py:3-7): a,b f32 [B,H,W,C] -> out f32 [B] (device). */
int  sr_psnr(sr_ctx* ctx, const void* a, const void* b, int B, int H, int W, int C, float max_val,
             float* out_B, void* stream);
int  sr_ssim(sr_ctx* ctx, const void* a, const void* b, int B, int H, int W, int C, float max_val,
             float* out_B, void* stream);
/* mean squared error over all elements -> out f32 [1] (Keras loss="mean_squared_error",
 * SRCNN_model.py:59). */
int  sr_mse(sr_ctx* ctx, const void* a, const void* b, int64_t n, float* out1, void* stream);
/* Pieces of the ESRGAN generator loss (ESRGAN_model.py:433-473; _train_step :511-523, evaluate :812-826): a, b f32 [B,H,W,C] device.
 * sr_l1: mean |a - b| over n elements (_pixel_loss).  sr_spectral_l1: mean | |F(a)| - |F(b)| | with tf.signal.fft2d's axes, the
 * INNERMOST two of NHWC = (W, C) (_spectral_loss; C must be 3).  Both write one float.  The adversarial term is a [B,1] vector
 * (host arithmetic), the perceptual term is sr_mse on two SR_MODEL_VGG19_FEATURES outputs. */
int  sr_l1(sr_ctx* ctx, const void* a, const void* b, int64_t n, float* out1, void* stream);
int  sr_spectral_l1(sr_ctx* ctx, const void* a, const void* b, int B, int H, int W, int C, float* out1, void* stream);
/* Backward-pass pieces of Keras model.fit (SRCNN_model.py:84-90, EDSR_model.py:164-170: loss = mean_squared_error, Adam) and of
 * ESRGAN._train_step (ESRGAN_model.py:475-533).  fp32 device tensors, NHWC dense.
 * sr_conv2d_wgrad: gradient of a Keras Conv2D(K x K, SAME, stride 1) kernel and bias: dw HWIO [K,K,Cin,Cout] = sum over pixels of
 *   x[b, y+ky-p, x+kx-p, ci] * dy[b,y,x,co];  db [Cout] = sum of dy (NULL to skip).  The input gradient needs no entry point of its
 *   own: it is sr_conv2d on dy with the kernel rotated by 180 degrees and its channel axes swapped.
 * sr_eltwise: the element-wise halves of the chain rule (SR_ELT_*), a / b / out of n floats (b may be NULL for AXPBY with beta 0).
 * sr_space_to_depth: the inverse of tf.nn.depth_to_space (DCR order): x [B,H*r,W*r,C] -> y [B,H,W,r*r*C] (its gradient). */
int  sr_conv2d_wgrad(sr_ctx* ctx, const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, int K,
                     float* dw_hwio, float* db, void* stream);
/* sr_conv2d_wgrad for 3x3 layers on maps of at most 8 x 8 pixels (H <= 8, W <= 8; block5 of a fine-tuned VGG16 on 128-pixel patches): the same
 * kernel scheme and summation structure, on staged tiles that hold 27 / (W + 1) images side by side (one shared zero column between neighbours)
 * instead of one image in an 8 x 24 tile.  Deterministic; not bit-identical to sr_conv2d_wgrad (the pixels meet in another order). */
int  sr_conv2d_wgrad_maps(sr_ctx* ctx, const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, float* dw_hwio, float* db,
                          void* stream);
/* sr_conv2d with DEVICE fp32 weights (the training loop keeps its parameters on the device between optimiser steps): d_w is a device
 * HWIO tensor [K,K,Cin,Cout]; with rot = 1 it is instead the forward kernel [K,K,Cout,Cin] of the layer whose INPUT gradient is wanted,
 * and the conv runs on its 180-degree-rotated, channel-swapped form (ESRGAN_model.py:505-533 via tf.GradientTape).  The kernel is packed
 * into MFMA fragment order by a device kernel; fully asynchronous on `stream`; scratch is reused call to call in stream order, so one
 * stream per context.  fp32 tensors only. */
int  sr_conv2d_dev(sr_ctx* ctx, const void* x, int B, int H, int W, int Cin, const float* d_w, const float* d_bias, int K, int Cout,
                   int rot, int act, float alpha, const void* skip1, float beta1, const void* skip2, float beta2, int clip01,
                   int d2s_r, void* y, void* stream);
/* The same three pieces of the training step on CHANNEL RANGES of NHWC fp32 buffers (ESRGAN_model.py:212-254: a dense block's concat tensor kept in one buffer,
 * every conv reading a prefix of it and writing its own slice; in the backward pass every input gradient accumulating in place into a prefix of the gradient
 * buffer through skip1 = y).  sr_view: p = the buffer, cs = its channels per pixel, coff = the view's first channel (cs, coff multiples of 4; the conv's Cin a
 * multiple of 16).  sr_eltwise_views: op over npix pixels x C channels. */
typedef struct { const void* p; int64_t cs; int32_t coff; } sr_view;
int  sr_conv2d_dev_views(sr_ctx* ctx, const sr_view* x, int B, int H, int W, int Cin, const float* d_w, const float* d_bias, int K, int Cout, int rot,
                         int act, float alpha, const sr_view* skip1, float beta1, const sr_view* y, void* stream);
int  sr_conv2d_wgrad_views(sr_ctx* ctx, const sr_view* x, const sr_view* dy, int B, int H, int W, int Cin, int Cout, int K,
                           float* dw_hwio, float* db, void* stream);
int  sr_eltwise_views(sr_ctx* ctx, int op, const sr_view* a, const sr_view* b, float alpha, float beta, const sr_view* out, int64_t npix, int C, void* stream);
/* Pack the weights of n conv uses by ONE launch, now, on `stream`, from the current contents of w / bias (a training step otherwise packs once per sr_conv2d_dev /
 * _views call: ~800 launches of ~5 us in the step of ESRGAN_model.py:475-533).  A later sr_conv2d_dev / sr_conv2d_dev_views on this context whose (d_w, d_bias, K, Cin,
 * Cout, rot) equals a listed use takes the pack made here instead of packing again; Cin / Cout are those of the CALL (for rot = 1, the gradient's channels in, the
 * layer's input channels out).  Every call replaces the whole list; n = 0 forgets it.  The caller must call again after changing any listed weight (a trainer: at the
 * start of every step) -- the library cannot see a write to w. */
typedef struct { const float* w; const float* bias; int32_t K, Cin, Cout, rot; } sr_pack_desc;
int  sr_conv_prepack(sr_ctx* ctx, const sr_pack_desc* uses, int n, void* stream);
/* Mixed-precision training: Keras model.fit of EDSR_model.py:127-176 with bf16 activations and activation gradients between kernels, fp32 master weights, fp32 weight /
 * bias gradients, fp32 loss and optimiser ("Mixed-precision training").  Every kernel widens its operands to fp32, accumulates and applies its epilogue in
 * fp32 and rounds once, to nearest even, on store.  All asynchronous on `stream`; one stream per context.
 * sr_conv2d_dev_bf16 (EDSR_model.py:127-176, the forward and input-gradient convs): sr_conv2d_dev with x, skip1, skip2 and y in bf16; d_w (fp32 device kernel, HWIO or with
 *   rot = 1 the forward kernel of the layer whose input gradient is wanted) and d_bias stay fp32.  The kernel is rounded to bf16 once by a device pack kernel, into the very
 *   image sr_conv2d packs on the host, and runs on the bf16 conv kernels sr_conv2d runs: the same bits as sr_conv2d on the same values.
 * sr_conv_prepack_bf16 (EDSR_model.py:127-176, once per step): sr_conv_prepack for sr_conv2d_dev_bf16 -- one launch for all of a step's uses; every call replaces the whole
 *   bf16 list, n = 0 forgets it.  The bf16 list and sr_conv_prepack's fp32 list are separate: the same (w, K, Cin, Cout, rot) may stand in both.
 * sr_conv2d_wgrad_bf16 (EDSR_model.py:127-176, the kernel and bias gradients): dw HWIO [3,3,Cin,Cout] = scale * sum over pixels of x[b, y+ky-1, x+kx-1, ci] * dy[b,y,x,co] and
 *   db [Cout] = scale * sum of dy (NULL to skip), fp32, from bf16 x [B,H,W,x_cs] and dy [B,H,W,dy_cs] of which the first Cin / Cout channels of every pixel count (a
 *   channel-padded input buffer: x_cs = 8, Cin = 3).  Products of bf16 values are exact in fp32; only the fp32 summation rounds, in a fixed order (no atomics).  K must be 3.
 * sr_relu_bwd_bf16 (EDSR_model.py:127-176, ReLU's gradient): out = dy where y > 0, else +0, on n bf16 elements; a select, no rounding.
 * sr_space_to_depth_bf16 (EDSR_model.py:127-176, depth_to_space's gradient): sr_space_to_depth on bf16, a permutation.
 * sr_mse_clip_grad_bf16 (EDSR_model.py:127-176, the clip, loss = mean_squared_error and its gradient): pre bf16 [n], t fp32 [n] (the target is NOT rounded) ->
 *   loss1 fp32 [1] = mean((clip(pre, 0, 1) - t)^2), summed in fp64 in a fixed order; dpre bf16 [n] = bf16(fp32(2 / n) * (clip(pre, 0, 1) - t)) where 0 <= pre <= 1, else 0;
 *   y fp32 [n] = clip(pre, 0, 1) (NULL to skip). */
int  sr_conv2d_dev_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int Cin, const float* d_w, const float* d_bias, int K, int Cout,
                        int rot, int act, float alpha, const void* skip1, float beta1, const void* skip2, float beta2, int clip01,
                        int d2s_r, void* y, void* stream);
int  sr_conv_prepack_bf16(sr_ctx* ctx, const sr_pack_desc* uses, int n, void* stream);
int  sr_conv2d_wgrad_bf16(sr_ctx* ctx, const void* x, int64_t x_cs, const void* dy, int64_t dy_cs, int B, int H, int W, int Cin, int Cout, int K, float scale,
                          float* dw_hwio, float* db, void* stream);
int  sr_relu_bwd_bf16(sr_ctx* ctx, const void* dy, const void* y, void* out, int64_t n, void* stream);
int  sr_space_to_depth_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int C, int r, void* y, void* stream);
int  sr_mse_clip_grad_bf16(sr_ctx* ctx, const void* pre, const float* t, int64_t n, float* loss1, void* dpre, float* y, void* stream);
/* Mixed-precision training of ESRGAN's RRDB trunk (ESRGAN_model.py:212-300 under _train_step, :475-533): the dense blocks' virtual-concat plumbing on bf16 buffers
 * (DESIGN.md 3.26).  sr_view here addresses bf16 elements: cs and coff multiples of 8 (16 bytes).
 * sr_conv2d_dev_views_bf16 (ESRGAN_model.py:212-254, a dense block's forward and input-gradient convs): sr_conv2d_dev_views with x, skip1, skip2 and y channel ranges of
 *   bf16 buffers and fp32 device kernels, out = alpha * act(conv + b) + beta1 * skip1 + beta2 * skip2 in fp32, rounded once; a skip may be the output range itself.  Cin
 *   is a whole number of 32-channel chunks.  The kernel is rounded to bf16 as sr_conv2d_dev_bf16 rounds it (sr_conv_prepack_bf16's list answers for it).
 * sr_conv2d_wgrad_group_bf16 (ESRGAN_model.py:212-254, the kernel and bias gradients of a dense block's layers): sr_conv2d_wgrad_bf16 of n = 1..SR_WGRAD_GROUP_MAX 3x3
 *   layers that share [B,H,W], by one main and one finish launch: job j gives dw [3,3,Cin,Cout] = scale * sum x * dy and db [Cout] = scale * sum dy (NULL to skip) from
 *   the views x and dy.  The job table travels in the kernel arguments: no copy, no sync.  One job alone gives sr_conv2d_wgrad_bf16's bits; a view that is not 16-byte
 *   aligned, or a channel count that is no multiple of 8, is staged element by element.
 * sr_eltwise_views_bf16 (ESRGAN_model.py:212-300, ReLU's gradient read off the concat buffers; an RRDB's two gradient paths joined): SR_ELT_RELU_BWD -- out = a where
 *   b > 0, else +0, a select on bits -- and SR_ELT_AXPBY -- out = bf16(alpha * a + beta * b) in fp32, b may be NULL -- over npix pixels x C channels of bf16 views. */
#define SR_WGRAD_GROUP_MAX 8
typedef struct { sr_view x; sr_view dy; int32_t Cin, Cout; float scale; float* dw; float* db; } sr_wgrad_job;
int  sr_conv2d_dev_views_bf16(sr_ctx* ctx, const sr_view* x, int B, int H, int W, int Cin, const float* d_w, const float* d_bias, int K, int Cout, int rot,
                              int act, float alpha, const sr_view* skip1, float beta1, const sr_view* skip2, float beta2, const sr_view* y, void* stream);
int  sr_conv2d_wgrad_group_bf16(sr_ctx* ctx, const sr_wgrad_job* jobs, int n, int B, int H, int W, void* stream);
int  sr_eltwise_views_bf16(sr_ctx* ctx, int op, const sr_view* a, const sr_view* b, float alpha, float beta, const sr_view* out, int64_t npix, int C, void* stream);
/* ---- a G = 8 dense block trained on the LDS-resident image (ESRGAN_model.py:212-254 at the notebook's growth width) ----
 * The arithmetic is that of the bf16 trunk above: fp32 master kernels rounded to bf16 once per step, bf16 tensors between stages, fp32 accumulation and epilogues, one
 * rounding per store.  All buffers are NHWC bf16; sr_view as above (cs, coff multiples of 8).
 * sr_dense_block_pack_sizes: bytes of the forward fragments, floats of the bias table and bytes of the input-gradient fragments of ONE block.
 * sr_dense_block_pack_dev: one launch packs nblocks blocks.  d_table: device array of nblocks x 10 pointers -- per block the five fp32 HWIO kernels [3,3,64 + 8 i,8] (i < 4) /
 *   [3,3,96,64], then the five biases.  fwd / bias / bwd: nblocks consecutive images of the sizes above; the forward half is bit for bit what sr_model_finalize packs for
 *   the same weights, the backward half holds the kernels rotated by 180 degrees with cin and cout swapped.
 * sr_dense_block_fwd_bf16: F [B,H,W,f_cs >= 96]: channels [0,64) are read, slice k = bf16(relu(conv_k(F[:64 + 8 (k - 1)]) + b_k)) is written into [64,96) of the same buffer;
 *   out (64 channels, not in F's buffer) = bf16(alpha * (conv5(F) + b5) + beta1 * F[:64] + beta2 * skip2), skip2 NULL for none.  sr_dense_block_lds_bytes(8, H, W) must be > 0.
 * sr_dense_block_bwd_bf16: from dY (64 channels) and the stored F: G = bf16(a5 * dgrad(dY, conv5)); for k = 4 .. 2 dz_k = G slice k where F slice k > 0, else +0 (a select on
 *   bits), G[:cin_k] = bf16(dgrad(dz_k, conv_k) + G[:cin_k]); dz_1 likewise; dX (64 channels) = bf16(dgrad(dz_1, conv1) + G[:64] + bx * dY).  dz [B,H,W,32]: dz_k in channels
 *   [8 (k - 1), 8 k).  stages: NULL, or [4,B,H,W,96] receiving G after conv5's input gradient and after the accumulate of k = 4, 3, 2 (channels >= cin_k of the later stages
 *   hold the dz already selected).  The image must also have (H + 2)(W + 2) <= sr_dense_block_train_max_pixels().  G never leaves the CU's LDS. */
int  sr_dense_block_train_max_pixels(void);
void sr_dense_block_pack_sizes(int64_t* fwd_bytes, int64_t* bias_floats, int64_t* bwd_bytes);
int  sr_dense_block_pack_dev(sr_ctx* ctx, const void* d_table, int nblocks, void* fwd, float* bias, void* bwd, void* stream);
int  sr_dense_block_fwd_bf16(sr_ctx* ctx, const void* fwd_w, const float* bias, void* F, int64_t f_cs, int B, int H, int W, const sr_view* out, const sr_view* skip2, float alpha,
                             float beta1, float beta2, void* stream);
int  sr_dense_block_bwd_bf16(sr_ctx* ctx, const void* bwd_w, const sr_view* dY, const void* F, int64_t f_cs, int B, int H, int W, float a5, float bx, void* dz, const sr_view* dX,
                             void* stages, void* stream);
/* ---- 3x3 convs over many small images with hundreds of channels (the frozen VGG19 of ESRGAN's perceptual loss on training patches, whose blocks 4-5 see 6 x 6 and
 * 3 x 3 images of 512 channels; the trainer sends a call here only where this kernel measured fastest -- images up to 3 x 3, or up to 6 x 6 with at most 1008 pixels
 * in the call; 12 x 12 images stay on sr_conv2d_dev_bf16 -- ESRGAN_model.py:379-408, 514-524) ----
 * sr_conv3x3_small_bf16 (ESRGAN_model.py:379-408 the extractor's convs, :514-524 their input gradients under the tape): Conv2D(3 x 3, SAME, stride 1) on bf16 x [B,H,W,Cin]
 *   -> bf16 y [B,H,W,Cout] with H * W <= 144, Cin and Cout multiples of 32, any B >= 1; anything else is SR_ERR_INVALID.  The contract is sr_conv2d_dev_bf16's: d_w is the
 *   fp32 device kernel (HWIO [3,3,Cin,Cout], or with rot = 1 the forward kernel [3,3,Cout,Cin] of the layer whose input gradient is wanted), rounded to bf16 once by a device
 *   pack; fp32 accumulation on MFMA; fp32 bias (NULL: none); y = bf16(act(conv + b)), act SR_ACT_LINEAR or SR_ACT_RELU, the whole epilogue in fp32 and one rounding to nearest
 *   even.  mask (NULL: none) is a bf16 tensor of y's shape: where mask <= 0 (sr_relu_bwd_bf16's predicate, on the bits) the stored value is +0 -- the ReLU gradient of
 *   the layer in front, as a select on the rounded result.  The GEMM's pixel axis runs over all images together and K is split over the four waves of a workgroup in a way
 *   that depends on Cin alone: an image's bits depend neither on B nor on its place in the batch; a tap outside its own image is a zero operand that is never loaded.
 *   packed: NULL, or a kernel packed by sr_conv3x3_small_pack_bf16 for the same (Cin, Cout); then d_w and rot are not looked at.
 * sr_conv3x3_small_pack_bytes / sr_conv3x3_small_pack_bf16 (ESRGAN_model.py:379-400, the extractor's weights are frozen): the packed-kernel handle for weights that outlive a
 *   step.  The caller owns the buffer (pack_bytes bytes, 16-byte aligned; 0 for channel counts the kernel refuses); it is no part of sr_conv_prepack_bf16's per-step list
 *   and never answers for it.  The caller packs again after changing the weights.
 * The other kernels of the bf16 perceptual branch (bf16 values travel as their bits: a select never rounds):
 * sr_vgg_preprocess_bf16 (ESRGAN_model.py:401-408, keras vgg19.preprocess_input of both feature passes of :514-516): fake and hr fp32 [B,H,W,3] RGB in [-1,1] -> out bf16
 *   [2B,H,W,6], fake first.  Per pixel v = (x + 1) * 127.5 in BGR order minus the caffe means, as SR_SP_VGG_PREPROCESS computes it in fp32; channels 0-2 hold
 *   hi = bf16(v), channels 3-5 lo = bf16(v - hi): with block1_conv1's kernel stacked twice along Cin the entry carries 16 bits of v at no MFMA cost (Cin pads to 8 anyway).
 * sr_vgg_preprocess_bwd (ESRGAN_model.py:514-524, the tape through preprocess_input): dv bf16 [npix,3], the gradient of v -> dfake fp32 [npix,3] = 127.5 * dv with the
 *   channels flipped back.
 * sr_maxpool2_bf16 / sr_maxpool2_bwd_bf16 (ESRGAN_model.py:379-400, VGG19's MaxPooling2D(2,2) and its gradient under the tape): x bf16 [B,H,W,C] -> y [B,H/2,W/2,C], VALID
 *   (an odd last row / column is dropped); the winner of a window is the first of (0,0), (0,1), (1,0), (1,1) that equals the maximum -- sr_maxpool2_bwd's order and tie
 *   rule.  The backward takes the pre-pool activation x and dy [B,H/2,W/2,C]: dx = dy at the window's winner where x > 0 (the ReLU of the conv in front of the pool,
 *   sr_relu_bwd_bf16's predicate), else +0.  C a multiple of 8, H, W >= 2.
 * sr_mse_grad_bf16 (ESRGAN_model.py:514-516, mean_squared_error of the two feature maps and its gradient): feats bf16 = [ff | fr], n elements each -> perc1 fp32 [1] =
 *   mean((ff - fr)^2), summed in fp64 in a fixed order; dff bf16 [n] = bf16(fp32(2 / n) * (ff - fr)), both operations rounded on their own, where ff > 0 (block5_conv4's
 *   own ReLU), else +0. */
int64_t sr_conv3x3_small_pack_bytes(int Cin, int Cout);
int  sr_conv3x3_small_pack_bf16(sr_ctx* ctx, const float* d_w, int Cin, int Cout, int rot, void* packed, void* stream);
int  sr_conv3x3_small_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int Cin, const float* d_w, const void* packed, const float* d_bias, int Cout, int rot, int act,
                           const void* mask, void* y, void* stream);
int  sr_vgg_preprocess_bf16(sr_ctx* ctx, const float* fake, const float* hr, int B, int H, int W, void* out, void* stream);
int  sr_vgg_preprocess_bwd(sr_ctx* ctx, const void* dv, int64_t npix, float* dfake, void* stream);
int  sr_maxpool2_bf16(sr_ctx* ctx, const void* x, int B, int H, int W, int C, void* y, void* stream);
int  sr_maxpool2_bwd_bf16(sr_ctx* ctx, const void* x, const void* dy, int B, int H, int W, int C, void* dx, void* stream);
int  sr_mse_grad_bf16(sr_ctx* ctx, const void* feats, int64_t n, float* perc1, void* dff, void* stream);
int  sr_eltwise(sr_ctx* ctx, int op, const void* a, const void* b, float alpha, float beta, void* out, int64_t n, void* stream);
/* keras.optimizers.Adam's dense update (the optimiser of ESRGAN_model.py:176-195, SRCNN_model.py:55-60, EDSR_model.py:127-140) over one flat
 * fp32 bucket of n parameters, in place on the device: g is first multiplied by grad_scale (1 / world size after a summing all-reduce; 1 leaves
 * it alone), then m = b1 m + (1-b1) g, v = b2 v + (1-b2) g g, w -= lr_t m / (sqrt(v) + epsilon); lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) is the
 * caller's (it knows the step count).  Each operation is rounded on its own: bit for bit NumPy's fp32 evaluation of the same expression. */
int  sr_adam(sr_ctx* ctx, void* w, const void* g, void* m, void* v, int64_t n, float lr_t, float beta1, float one_minus_beta1, float beta2,
             float one_minus_beta2, float epsilon, float grad_scale, void* stream);
int  sr_space_to_depth(sr_ctx* ctx, const void* x, int B, int H, int W, int C, int r, void* y, void* stream);
/* More halves of ESRGAN._train_step's backward pass (ESRGAN_model.py:475-533), fp32 device tensors:
 * sr_matmul: C[b] = alpha * op(A[b]) op(B[b]) (row-major, op = transpose when the flag is set) -- the MATERIALISED SelfAttention of the
 *   24x24 / 48x48 training patches (:57-65) and its six backward products; sr_softmax_rows / sr_softmax_bwd: softmax over the last axis in
 *   place, and ds = p * (dp - <dp, p>).
 * sr_maxpool2_bwd: MaxPooling2D(2,2) gradient (VGG19 extractor); sr_zero_insert2: adjoint of the stride-2 pick of the discriminator's
 *   strided convs (dy [B,ceil(H/2),ceil(W/2),C] -> [B,H,W,C]); sr_spectral_l1_bwd: gradient of scale * sr_spectral_l1 w.r.t. a. */
/* sr_spatial_op: the non-conv layers of the discriminator / VGG19 graphs as single ops, x f32 [B,H,W,C] -> y:
 *   SR_SP_MAXPOOL2 [B,H/2,W/2,C] (MaxPooling2D(2,2) VALID), SR_SP_GAP [B,C] (GlobalAveragePooling2D), SR_SP_PICK2 [B,ceil(H/2),ceil(W/2),C]
 *   (the sampling half of a stride-2 SAME conv, see SR_MODEL_ESRGAN_D), SR_SP_VGG_PREPROCESS [B,H,W,3] (ESRGAN_model.py:401-408). */
enum { SR_SP_MAXPOOL2 = 0, SR_SP_GAP = 1, SR_SP_PICK2 = 2, SR_SP_VGG_PREPROCESS = 3 };
int  sr_spatial_op(sr_ctx* ctx, int op, const void* x, int B, int H, int W, int C, void* y, void* stream);
int  sr_matmul(sr_ctx* ctx, const void* A, const void* B, void* C, int batch, int M, int N, int K, int transA, int transB, float alpha, void* stream);
int  sr_softmax_rows(sr_ctx* ctx, void* s, int64_t rows, int cols, void* stream);
int  sr_softmax_bwd(sr_ctx* ctx, const void* p, const void* dp, void* ds, int64_t rows, int cols, void* stream);
/* The STREAMED SelfAttention of training (ESRGAN_model.py:57-65: s = g f^T, beta = softmax(s), o = beta h, with q = g, k = f, v = h): the same
 * core without any N x N tensor in memory, so that a training patch may be as large as an inference patch.  fp32; q, k: 8 channels, v: 32 channels,
 * each a device pointer to its first element plus a row stride in ELEMENTS (token i of image b is row b * N + i; three dense tensors: 8, 8, 32; one
 * fused f | g | h buffer [B,N,64]: pointers 0 / 8 / 16 floats in, all strides 64; pointers 16-byte aligned, strides multiples of 4).  o, dO, dv
 * [B,N,32], dq, dk [B,N,8] and lse [B,N] are dense.
 * sr_attention_fwd_lse: o as sr_self_attention's core computes it, and lse[b,i] = max_j s_ij + log sum_j exp(s_ij - max) (natural log).
 * sr_attention_bwd: with P_ij = exp(s_ij - lse_i) recomputed tile by tile and D_i = <dO_i, o_i>:  dv_j = sum_i P_ij dO_i,
 *   dS_ij = P_ij (dO_i . v_j - D_i),  dk_j = sum_i dS_ij q_i,  dq_i = sum_j dS_ij k_j.  No atomics: bit-identical from run to run.
 * Wrong sizes, strides or alignment: SR_ERR_INVALID with a message. */
int  sr_attention_fwd_lse(sr_ctx* ctx, const void* q, const void* k, const void* v, int64_t q_rs, int64_t k_rs, int64_t v_rs, int B, int N,
                          void* o, void* lse, void* stream);
int  sr_attention_bwd(sr_ctx* ctx, const void* q, const void* k, const void* v, const void* o, const void* dO, const void* lse,
                      int64_t q_rs, int64_t k_rs, int64_t v_rs, int B, int N, void* dq, void* dk, void* dv, void* stream);
int  sr_maxpool2_bwd(sr_ctx* ctx, const void* x, const void* dy, int B, int H, int W, int C, void* dx, void* stream);
int  sr_zero_insert2(sr_ctx* ctx, const void* dy, int B, int H, int W, int C, void* out, void* stream);
int  sr_spectral_l1_bwd(sr_ctx* ctx, const void* a, const void* b, int B, int H, int W, int C, float scale, void* da, void* stream);
/* add_padding + sliding-window extraction (SRCNN_model.py:127-162, EDSR_model.py:201-223,
 * ESRGAN_model.py:883-901, VGG16_model.py:216-239): img f32 [H,W,C] (unpadded), reflect padding
 * bottom/right computed from (patch,stride); out [P,patch,patch,C] of out_dtype, each value
 * v*mul+add (ESRGAN: *2-1), product and sum rounded separately as NumPy's two ufuncs round them.  *n_patches receives P.  out may be
 * NULL to query P only. */
int  sr_extract_patches(sr_ctx* ctx, const float* img, int H, int W, int C, int patch, int stride,
                        float mul, float add, int out_dtype, void* out, int64_t out_capacity,
                        int* n_patches, void* stream);
/* reconstruct_from_patches (SRCNN_model.py:164-188, EDSR_model.py:225-256, ESRGAN_model.py:903-921):
 * overlap-add of [P,patch*scale,patch*scale,C] patches (in_dtype; value v*mul+add first, ESRGAN:
 * (v+1)/2), divide by coverage count, crop to [H*scale,W*scale,C], clip[0,1]; out f32.
 * H,W = unpadded LR size; patch,stride in LR pixels. */
int  sr_overlap_add(sr_ctx* ctx, const void* patches, int in_dtype, int H, int W, int C, int patch,
                    int stride, int scale, float mul, float add, float* out, void* stream);

/* ---- classifying a stack of frames and scoring a comparison of SR methods (VGG16_model.py:168-270 for F frames at once;
 *      deep_lerning_visualizations.py:230-314, 454-495) ----
 * sr_extract_patches_batch: sr_extract_patches for F frames of one size in one launch.  imgs [F,H,W,C] of in_dtype (SR_DTYPE_F32 or
 *   SR_DTYPE_U8, the value float(u8)); out [F*P,patch,patch,C] of out_dtype (f32 or bf16), frame-major, a frame's P patches in
 *   sr_extract_patches' order with its reflect padding (bottom/right, from (patch,stride)) and its v*mul+add.  Frame f's slice is bit for bit
 *   what sr_extract_patches writes for frame f alone (for u8 input: for float(u8)).  *patches_per_image receives P; out may be NULL to query P
 *   only.  out_capacity counts elements; too small -> SR_ERR_CAPACITY and nothing is written.  Element indices are 64-bit.
 * sr_patch_vote: the majority vote of VGG16_model.py:252-268 for F frames.  probs f32 [F*P,K], 1 <= K <= 64 (else SR_ERR_INVALID).  Per frame:
 *   each patch votes for its argmax (first maximum); the class with the most votes wins; on a tie of votes, the tied class with the highest
 *   mean probability over the frame's P patches, the lowest index on equal means.  cls_F int32 [F]; conf_F f32 [F] = the winner's mean
 *   probability, accumulated in fp64 in a fixed order (one workgroup per frame, a tree, no float atomics: the same bits on every run) and
 *   rounded once to fp32; votes_FxK int32 [F,K] (may be NULL) the vote counts.
 * sr_classification_counts: for each of A methods the K x K confusion matrix (rows = true class, columns = predicted class; int64
 *   [A,K,K], zeroed by the call) of preds_AxN int32 [A,N] against y_true_N int32 [N], and conf_sums_Ax2 f64 [A,2] = (sum of conf, sum of conf
 *   over the correct predictions) of conf_AxN f32 [A,N] (may be NULL: the sums are 0), fixed-order fp64.  A pair with a label outside [0,K)
 *   is counted in no cell.  The correct counts are the matrices' traces: a whole study ends in one small read-back. */
int  sr_extract_patches_batch(sr_ctx* ctx, const void* imgs, int in_dtype, int F, int H, int W, int C, int patch, int stride,
                              float mul, float add, int out_dtype, void* out, int64_t out_capacity, int* patches_per_image, void* stream);
int  sr_patch_vote(sr_ctx* ctx, const float* probs, int F, int P, int K, int32_t* cls_F, float* conf_F, int32_t* votes_FxK, void* stream);
int  sr_classification_counts(sr_ctx* ctx, const int32_t* y_true_N, const int32_t* preds_AxN, const float* conf_AxN, int A, int N, int K,
                              int64_t* confusion_AxKxK, double* conf_sums_Ax2, void* stream);

/* ---- the classical study's other four up-scalers (classic_algorithms.py:23-108), 2-D uint8 grayscale, B images of one size ----
 * sr_back_projection: back_projection (classic_algorithms.py:23-43).  hr_u8 [B,H,W] is the starting estimate (the reference starts
 *   from its first argument), lr_u8 [B,h,w] the observation, H >= h, W >= w.  Each of `iterations` rounds: diff = float32(lr) -
 *   resize(est, (w, h), INTER_LINEAR); est += resize(diff, (W, H), INTER_LINEAR), sr_resize's float32 rules (an exact 2x shrink is the
 *   2 x 2 area mean).  y_u8 [B,H,W] = clip(est, 0, 255) truncated; y_f32 [B,H,W] (may be NULL) receives est before the clip.  Every
 *   product and every sum is rounded on its own, in sr_resize's order (horizontal taps, then vertical, then the difference or the
 *   update): y_f32 is bit for bit the float32 NumPy evaluation.
 * sr_noise_sigma: estimate_sigma(x) as non_local_means calls it (classic_algorithms.py:45): median of |dd band of pywt.dwtn(x, 'db2')|
 *   ('symmetric' mode, 0..255 units) over its non-zero entries / norm.ppf(0.75) -> sigma_f64 [B] (device; NaN when every entry is 0).
 *   Per axis (axis 0 first) d[o] = sum_{j<3} dec_hi[j] * (x[2o+1-j] - x[2o-2]) in fp64, j ascending, every product and sum rounded on its
 *   own; the median is exact (the mean of the middle two for an even count): bit for bit the NumPy evaluation.
 * sr_nl_means: denoise_nl_means(x / 255, h = h_scale * sigma_f64[b], patch_size = patch (odd, <= 9), patch_distance = distance (<= 12),
 *   fast_mode=True) (classic_algorithms.py:47-53): y_f32 [B,h,w]; sigma_f64 is read on the device.
 * sr_edge_guided: edge_guided_interpolation (classic_algorithms.py:64-85): clip(addWeighted(resize_u8(x, (W, H), INTER_LINEAR), 1,
 *   resize(hypot(Sobel_x, Sobel_y), (W, H)), weight, 0), 0, 255) truncated -> y_u8 [B,H,W]; up_e_f32 [B,H,W] (may be NULL) receives the
 *   float32 up-sized edge magnitude.  H >= h, W >= w.  The edge resize is OpenCV's fp64 path (float tap weights widened, horizontal
 *   pass first, e0 * w0 + e1 * w1 with every product and sum rounded on its own), addWeighted float32(up) * 1 + up_e * weight + 0
 *   likewise in float32: both outputs are bit for bit the NumPy evaluation.
 * sr_freq_extrapolate: frequency_extrapolation (classic_algorithms.py:87-108): |ifft2 of the centred LR spectrum zero-padded to H x W|
 *   as the separable fp64 map |A_H X A_W^T| -> y_f64 [B,H,W].  H >= h, W >= w. */
int  sr_back_projection(sr_ctx* ctx, const uint8_t* hr_u8, const uint8_t* lr_u8, int B, int H, int W, int h, int w, int iterations,
                        uint8_t* y_u8, float* y_f32, void* stream);
int  sr_noise_sigma(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, double* sigma_f64, void* stream);
int  sr_nl_means(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int patch, int distance, const double* sigma_f64,
                 double h_scale, float* y_f32, void* stream);
int  sr_edge_guided(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int H, int W, float weight, uint8_t* y_u8,
                    float* up_e_f32, void* stream);
int  sr_freq_extrapolate(sr_ctx* ctx, const uint8_t* x_u8, int B, int h, int w, int H, int W, double* y_f64, void* stream);

/* ---- the classical study's image-quality scores (profiling_methods.py:45-167 and skimage.metrics), B pairs of one shape ----
 * sr_classic_scores: hr, sr DEVICE [B,H,W,C] (C 1: gray, 3: RGB), each SR_DTYPE_U8 or SR_DTYPE_F32 (hr_dtype, sr_dtype); H, W >= 7,
 *   B <= 65535.  data_range_f64 DEVICE [B].  scores_f64 DEVICE [B,SR_NUM_SCORES], fp64, in SR_SCORE_* order:
 *   psnr      skimage peak_signal_noise_ratio: 10 log10(dr^2 / mean((hr - sr)^2)), +inf for identical images;
 *   ssim      skimage structural_similarity defaults: 7 x 7 uniform window, K1 0.01, K2 0.03, covariances x 49/48, S averaged over the
 *             centres 3 pixels inside the border; RGB: the mean of the per-channel means;
 *   mae       mean |hr - sr| over every channel (profiling_methods.py:45-47);
 *   rmse      sqrt(mean((hr - sr)^2) + 1e-9) (:49-53);
 *   grad_mse  mean((M_hr - M_sr)^2) (:79-85), M = sobel_mag (:58-77): ksize-3 Sobel magnitude, BORDER_REFLECT_101, of the gray image
 *             divided by 255 when its own max > 1.5;
 *   epi       (sum M_sr + 1e-9) / (sum M_hr + 1e-9) (:87-94);
 *   hf_ratio  (sum_mask |F_sr| + 1e-9) / (sum_mask |F_hr| + 1e-9), F = fftshift(fft2(gray)) of the unscaled values, mask r >
 *             hf_radius_frac (r_max + 1e-9) around (H / 2, W / 2) (:98-114);
 *   kl_luma   sum P log(P / Q) of the 256-bin gray histograms (:116-137);
 *   kl_color  the per-channel 64-bin form averaged over the channels (:139-167); NaN for C = 1.
 *   Histograms bin as np.histogram(range=(0, 255), density=True) + 1e-12: uint8 values as they are, float as clip(x, 0, 1) * 255.
 *   The gray image is the image itself for C = 1 and OpenCV's fixed-point COLOR_RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14, for
 *   uint8 RGB; for RGB with a float image columns grad_mse .. kl_luma are NaN.
 *   Optional raw outputs (NULL: not written; written only where the gray columns are defined): gray_f32 [B,2,H,W] the unscaled gray
 *   images (hr, sr), sobel_f32 [B,2,H,W] their M, hist_luma_i32 [B,2,256] and hist_color_i32 [B,2,3,64] (C = 3) the counts.
 *   Every reduction runs in a fixed order: a pair's scores are bitwise the same on every run and for any B. */
enum { SR_SCORE_PSNR = 0, SR_SCORE_SSIM, SR_SCORE_MAE, SR_SCORE_RMSE, SR_SCORE_GRAD_MSE, SR_SCORE_EPI, SR_SCORE_HF_RATIO,
       SR_SCORE_KL_LUMA, SR_SCORE_KL_COLOR, SR_NUM_SCORES };
int  sr_classic_scores(sr_ctx* ctx, const void* hr, int hr_dtype, const void* sr, int sr_dtype, int B, int H, int W, int C,
                       const double* data_range_f64, double hf_radius_frac, double* scores_f64, float* gray_f32, float* sobel_f32,
                       int* hist_luma_i32, int* hist_color_i32, void* stream);

/* ---- the classical study's loop glue (super_resolucion_clasica.ipynb cell 8) and its SSIM similarity maps (visualization_methods.py:
 *      553-591), B images of one shape, csrc/metrics.hip.  Asynchronous on `stream`; on a refusal (negative code, sr_last_error) nothing
 *      is written ----
 * sr_rgb2gray_u8: cv2.cvtColor(x, COLOR_RGB2GRAY) as the notebook calls it on uint8 images (cell 8; visualization_methods.py:554-555):
 *   x_u8 DEVICE [B,H,W,3] -> y_u8 DEVICE [B,H,W], (4899 R + 9617 G + 1868 B + 8192) >> 14, the device function sr_classic_scores' gray
 *   columns use.  Any H, W and any pointer alignment (a tensor that is not 4-byte aligned takes a byte path).
 * sr_freq_to_u8: cell 8's normalisation of frequency_extrapolation's output, `(f / np.max(f) * 255.0).astype(np.uint8) if np.max(f) > 0
 *   else f.astype(np.uint8)`: f_f64 DEVICE [B,H,W] (what sr_freq_extrapolate writes) -> y_u8 DEVICE [B,H,W] and max_f64 DEVICE [B], each
 *   image's maximum (a fixed-order reduction; a NaN, once met, is the maximum, as for np.max).  The quotient and then the product are
 *   rounded fp64 operations in that order (no reciprocal, no fused multiply-add) and the result is truncated toward zero: bit for bit
 *   NumPy's expression.  B <= 65535, H W <= 2^28.
 * sr_ssim_map: skimage.metrics.structural_similarity(a, b, data_range=..., full=True) with its defaults (visualization_methods.py:578-579):
 *   a, b DEVICE [B,H,W,C], C 1 or 3, each SR_DTYPE_U8 or SR_DTYPE_F32 (mixed pairs allowed); data_range_f64 DEVICE [B]; H, W >= 7,
 *   B <= 65535.  map_f64 DEVICE [B,H,W,C] receives S over the WHOLE image: fp64, 7 x 7 uniform window, K1 0.01, K2 0.03, covariances x
 *   49/48, the window means at the border as scipy.ndimage.uniform_filter's default mode='reflect' takes them (d c b a | a b c d: the
 *   edge pixel repeated, NumPy's 'symmetric' -- not the BORDER_REFLECT_101 of this library's Sobel and resize code).  mean_f64 DEVICE [B]
 *   receives mssim: the mean of S over the centres 3 pixels inside the border, for C = 3 the mean of the per-channel means -- the sums
 *   sr_classic_scores' ssim column is made of.  Every reduction runs in a fixed order: a pair's outputs are bitwise the same on every run
 *   and for any B. */
int  sr_rgb2gray_u8(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, uint8_t* y_u8, void* stream);
int  sr_freq_to_u8(sr_ctx* ctx, const double* f_f64, int B, int H, int W, uint8_t* y_u8, double* max_f64, void* stream);
int  sr_ssim_map(sr_ctx* ctx, const void* a, int a_dtype, const void* b, int b_dtype, int B, int H, int W, int C,
                 const double* data_range_f64, double* map_f64, double* mean_f64, void* stream);

/* ---- the dataset EDA's per-pair image statistics and global accumulators (reference data/EDA.ipynb: ImageDatasetAnalyzer, cell
 * 87582ba8; MetricsAggregator.collect, cell eb5cc926), csrc/eda.hip.  B aligned pairs of one shape, lr_u8 and hr_u8 DEVICE uint8
 * [B,H,W,3] in BGR order (lr already resized to hr's size); 7 <= H, W <= 4096, H W <= 2^22, B <= 32767 (anything else: SR_ERR_INVALID).
 * The 8-bit OpenCV paths are restated from OpenCV's documented behaviour (cv2 is not installed where this project runs, so they are
 * not pinned against cv2 itself):
 *   gray    COLOR_BGR2GRAY, (1868 B + 9617 G + 4899 R + 8192) >> 14 (imgproc/src/color_yuv, the 14-bit RGB2Gray coefficients);
 *   blurs   GaussianBlur (3,3) / (5,5) with sigma 0: the fixed taps (1 2 1) / 4 and (1 4 6 4 1) / 16 (getGaussianKernel's small-kernel
 *           table), separable, the exact integer sum rounded half up once, (s + 8) >> 4 / (s + 128) >> 8, BORDER_REFLECT_101;
 *   HSV     COLOR_BGR2HSV's V = max(B, G, R) and S = ((V - min) sdiv[V] + 2^11) >> 12, sdiv[v] = round(255 2^12 / v), sdiv[0] = 0
 *           (color_hsv's RGB2HSV_b tables); H is not computed;
 *   Canny   (gray, 100, 200), aperture 3, L1 magnitude |gx| + |gy| of the 3 x 3 Sobel pair with replicated borders; a pixel with
 *           magnitude m > 100 survives when, with x = |gx|, y = |gy| 2^15: y < 13573 x: m > left and m >= right; y > 13573 x + x 2^16:
 *           m > above and m >= below; otherwise, s = -1 where gx and gy differ in sign, else 1: m > (above, column - s) and
 *           m > (below, column + s) (imgproc/src/canny.cpp).  A survivor is strong when m > 200; an edge is a survivor that is strong or
 *           8-connected to a strong one through survivors.  The outermost rows and columns are never edges and carry no connection
 *           (their magnitudes still take part in their neighbours' suppression).  The other reading of canny.cpp: it pads its
 *           magnitude and label buffers by one pixel and runs the same test on border pixels against zero magnitude outside, so
 *           border pixels could be edges; the project's contract fixes the first reading;
 *   dilate  5 x 5 ones, centred anchor, pixels outside the image ignored.
 * sr_eda_pair_stats: stats_f64 DEVICE [B,SR_NUM_EDA_STATS] in SR_EDA_* order, _LR / _HR of the pair's two images:
 *   psnr, ssim        sr_classic_scores' columns for (hr, lr), data range 255 (skimage, channel_axis=2);
 *   glcm_*            glcm_features on lr's gray: quantised to glcm_levels (64 or 256) as (uint8)(float32(g) / 255 * (levels - 1)),
 *                     graycomatrix(distance 1, symmetric, normed) for the angles of angle_mask (bit 0: 0, 1: 45, 2: 90, 3: 135 deg;
 *                     offsets (row, col) (0,1), (1,1), (1,0), (1,-1)), graycoprops contrast / homogeneity / correlation (1 where the
 *                     marginal variance is 0), mean over the angles;
 *   rms_noise         sqrt(mean((gray - blur3(gray))^2));   lap_var  population variance of the 0 1 0 / 1 -4 1 / 0 1 0 Laplacian of
 *                     gray, BORDER_REFLECT_101;
 *   blocking          (mean|D[7::8, :]| + mean|D[:, 7::8]|) / 2, D the orthonormal 2-D DCT-II of gray in fp64 (NaN below 8 rows or columns);
 *   color_noise       mean over the three channels of |img - blur5(img)|;
 *   ringing           population std of gray over dilate(E) and not E, E = Canny's edges; 0 when that region is empty;
 *   saturation_mean, brightness_mean   means of S and V;
 *   edge_diff         sobel_mean_hr - sobel_mean_lr, skimage.filters.sobel: sqrt((h^2 + v^2) / 2) of the (1 2 1) x (1 0 -1) / 4 pair on
 *                     gray / 255, edge pixels repeated;
 *   chN_skew, chN_kurt, chN_mean, chN_std   per B, G, R channel: m3 / m2^1.5, m4 / m2^2 - 3 (NaN for a constant channel), mean,
 *                     population std, the central moments formed exactly from integer power sums.
 *   Optional raw outputs (NULL: not written): gray_u8, sat_u8, val_u8, blur3_u8 (of gray), edges_u8 (0 / 255) [B,2,H,W] (lr, hr);
 *   blur5_u8 [B,2,H,W,3]; glcm_i32 [B,nangles,L,L] lr's counts before symmetrisation, angles in bit order; dct_f64 [B,2,H,W].
 *   Every reduction is an integer sum or runs in a fixed order: a pair's row is bitwise the same on every run and for any B.
 * sr_eda_accumulate: collect's global_data, added pair after pair into caller-owned DEVICE buffers: fft_lr_sum_f64, fft_hr_sum_f64
 *   [H,W] += |fftshift(fft2(gray))|; grad_hr_sum_f64 [H,W] += hypot of hr gray's ksize-5 Sobel pair (1 4 6 4 1 x -1 -2 0 2 1,
 *   BORDER_REFLECT_101); glcm_sum_f64 [256,256] += lr gray's 256-level, angle-0, symmetric normed matrix (integer counts divided in
 *   fp64); sat_counts_i64 [2,50] (lr, hr) += np.histogram(S, linspace(0, 256, 51)).  One call on 3 pairs equals three calls. */
enum { SR_EDA_PSNR = 0, SR_EDA_SSIM, SR_EDA_GLCM_CONTRAST, SR_EDA_GLCM_HOMOGENEITY, SR_EDA_GLCM_CORRELATION, SR_EDA_RMS_NOISE_LR,
       SR_EDA_RMS_NOISE_HR, SR_EDA_LAP_VAR_LR, SR_EDA_LAP_VAR_HR, SR_EDA_BLOCKING_LR, SR_EDA_BLOCKING_HR, SR_EDA_COLOR_NOISE_LR,
       SR_EDA_COLOR_NOISE_HR, SR_EDA_RINGING_LR, SR_EDA_RINGING_HR, SR_EDA_SATURATION_MEAN_LR, SR_EDA_SATURATION_MEAN_HR,
       SR_EDA_BRIGHTNESS_MEAN_LR, SR_EDA_BRIGHTNESS_MEAN_HR, SR_EDA_EDGE_DIFF,
       SR_EDA_CH0_SKEW_LR, SR_EDA_CH0_SKEW_HR, SR_EDA_CH1_SKEW_LR, SR_EDA_CH1_SKEW_HR, SR_EDA_CH2_SKEW_LR, SR_EDA_CH2_SKEW_HR,
       SR_EDA_CH0_KURT_LR, SR_EDA_CH0_KURT_HR, SR_EDA_CH1_KURT_LR, SR_EDA_CH1_KURT_HR, SR_EDA_CH2_KURT_LR, SR_EDA_CH2_KURT_HR,
       SR_EDA_SOBEL_MEAN_LR, SR_EDA_SOBEL_MEAN_HR,
       SR_EDA_CH0_MEAN_LR, SR_EDA_CH0_MEAN_HR, SR_EDA_CH1_MEAN_LR, SR_EDA_CH1_MEAN_HR, SR_EDA_CH2_MEAN_LR, SR_EDA_CH2_MEAN_HR,
       SR_EDA_CH0_STD_LR, SR_EDA_CH0_STD_HR, SR_EDA_CH1_STD_LR, SR_EDA_CH1_STD_HR, SR_EDA_CH2_STD_LR, SR_EDA_CH2_STD_HR, SR_NUM_EDA_STATS };
int  sr_eda_pair_stats(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, int glcm_levels, int angle_mask,
                       double* stats_f64, uint8_t* gray_u8, uint8_t* sat_u8, uint8_t* val_u8, uint8_t* blur3_u8, uint8_t* blur5_u8,
                       uint8_t* edges_u8, int* glcm_i32, double* dct_f64, void* stream);
int  sr_eda_accumulate(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, double* fft_lr_sum_f64,
                       double* fft_hr_sum_f64, double* grad_hr_sum_f64, double* glcm_sum_f64, int64_t* sat_counts_i64, void* stream);
/* sr_eda_pair_panels: the maps of the EDA's per-pair panels (cell 769cc582: create_advanced_visualizations, save_visual_example), one pair
 *   after the other and unsummed; same pairs, limits and 8-bit contract as above.  Every output is optional (NULL: not computed; the two DFT
 *   products are skipped when both spectra are NULL):
 *   spec_lr_f64, spec_hr_f64 [B,H,W]   |fftshift(fft2(gray))| of lr / hr: the magnitude, not its log -- the panel's np.log(mag + 1e-8) is
 *                                      the host's to take, on these bits;
 *   grad_hr_f64 [B,H,W]                hypot of hr gray's ksize-5 Sobel pair;
 *   glcm_lr_f64 [B,256,256]            lr gray's 256-level, angle-0, symmetric normed matrix (C + C^T) / T, T = 2 H (W - 1);
 *   noise_lr_f64 [B,H,W]               np.mean(|lr - blur5(lr)|, axis=2): the exact integer sum of the three channels divided by 3.0 once;
 *   diff_u8 [B,H,W]                    cvtColor(absdiff(lr, hr), BGR2GRAY), the 14-bit gray above of the per-channel |lr - hr|
 *                                      (convertScaleAbs of a uint8 image and cv2.resize to the same size are the identity);
 *   sat_hist_i64 [B,2,256]             counts of S per value, lr then hr;
 *   scalars_f64 [B,SR_NUM_EDA_PANEL_SCALARS]   graycoprops(glcm_lr, contrast)[0,0] and mean(noise_lr).
 *   For one pair spec_*, grad_hr and glcm_lr are the bits sr_eda_accumulate adds into zeroed buffers (the same kernels, storing), sat_hist
 *   folded by s * 25 / 128 is its sat_counts, and the scalars are the bits of sr_eda_pair_stats(256 levels, angle_mask 1)'s glcm_contrast and
 *   color_noise_lr.  Integer sums and fixed orders only: a pair's outputs are bitwise the same on every run, for any B and at any
 *   position in the batch. */
enum { SR_EDA_PANEL_GLCM_CONTRAST = 0, SR_EDA_PANEL_NOISE_MEAN, SR_NUM_EDA_PANEL_SCALARS };
int  sr_eda_pair_panels(sr_ctx* ctx, const uint8_t* lr_u8, const uint8_t* hr_u8, int B, int H, int W, double* spec_lr_f64, double* spec_hr_f64,
                        double* grad_hr_f64, double* glcm_lr_f64, double* noise_lr_f64, uint8_t* diff_u8, int64_t* sat_hist_i64,
                        double* scalars_f64, void* stream);

/* ---- dataset synthesis: the per-pixel stages of degrade_image (reference data/common_methods.py:52-107), csrc/degrade.hip ----
 * B images of one shape, x_u8 and y_u8 DEVICE uint8 [B,H,W,3] in BGR order; 16 <= H, W <= 4096, B <= 32767 (anything else: SR_ERR_INVALID).
 * params_i32 DEVICE int32 [B,SR_DEG_PARAMS], one row per image, in SR_DEG_* order; a stage whose flag is 0 in a row copies that image
 * through bit for bit.  The stage entries only launch.  A row outside the contract (below) is never acted on: its image is copied through
 * and the first such row is recorded on the device; sr_degrade_status waits for the stream, returns SR_ERR_INVALID with the stage, row
 * and value in sr_last_error when a row was recorded, and clears the record.  Integer arithmetic throughout, no reduction: the same
 * bits on every run and for any B.  (degrade_image's resize between the blurs and the noise is sr_resize on uint8.)
 * sr_degrade_gauss: cv2.GaussianBlur(x, (k, k), sigmaX=sigma), k = row[SR_DEG_GAUSS_KSIZE] in {3, 5, 7}, with the integer 8.8 taps
 *   t[0..k) = row[SR_DEG_GAUSS_TAP0 ..] (each 0..256, sum 256): y = (sum_j t_j sum_i t_i x[y + j - r, x + i - r] + 32768) >> 16 per channel,
 *   r = k / 2, rounded once after both passes, BORDER_REFLECT_101.  The host derives the taps (sr355.runtime.gauss_taps): g_i =
 *   exp(-(i - r)^2 / (2 sigma^2)) in fp64, t_i = floor(256 g_i / sum g + 0.5), the centre tap then takes 256 - sum t.  This restates
 *   OpenCV's 8-bit fixed-point GaussianBlur from its documented structure (8.8 taps, exact integer sums, one rounding); OpenCV spreads the
 *   tap-rounding residue differently, so a tap may differ by 1/256.  It is not pinned against cv2, which is installed nowhere this project
 *   runs -- the caveat the EDA's blurs above already carry.
 * sr_degrade_motion: cv2.filter2D(x, -1, K), K the size x size kernel whose centre row is 1 / size, size = row[SR_DEG_MOTION_SIZE] in
 *   {5, 7, 9}: a horizontal box, y = (2 S + size) / (2 size) rounded down, S the sum of the size neighbours, BORDER_REFLECT_101.  filter2D
 *   accumulates in float and rounds half to even; S / size for odd size is never a tie (its fraction is a multiple of 1 / size, at
 *   least 1/18 from 1/2), and fp32's error on a sum of nine products below 255 is of the order 1e-5, so both round every S alike and
 *   the integer form is the same function.
 * sr_degrade_noise: y = (uint8) trunc(min(max(float(x) + n, 0), 255)) where row[SR_DEG_NOISE_ON] != 0, n fp32.  field_f32 DEVICE fp32
 *   [B,H,W,3] (may be NULL) supplies n: the reference-faithful path, np.random.normal(0, std, shape).astype(np.float32) drawn on the host.
 *   NULL: n = std * z, std the fp32 whose bits are row[SR_DEG_NOISE_STD] (finite, >= 0), product and sum rounded separately (no
 *   contraction), z standard normal from Philox4x32-10: key = the 64-bit seed (low word first), counter = (e / 4, 0, image index, 0) for
 *   element e of the image's flattened (y, x, c), word e % 4 of the block; Box-Muller in fp32 per pair of words (x0, x1), (x2, x3): u1 =
 *   ((x0 >> 8) + 1) 2^-24, u2 = (x1 >> 8) 2^-24, z = sqrt(-2 ln u1) (cos, sin)(2 pi u2) for the pair's two elements.  z_f32 DEVICE fp32
 *   [B,H,W,3] (may be NULL; only with field_f32 NULL) receives z for every image, whatever its flag.
 * sr_degrade_jpeg: cv2.imdecode(cv2.imencode('.jpeg', x, [IMWRITE_JPEG_QUALITY, q])[1], 1), q = row[SR_DEG_JPEG_QUALITY] in 1..100, as
 *   libjpeg computes it with its defaults, without the lossless entropy coding: BGR -> YCbCr by the 16-bit fixed-point tables; the
 *   image's last column repeated up to whole blocks, its last row up to an even count; h2v2 chroma down-sampling (a + b + c + d + bias)
 *   >> 2, bias 1, 2, 1, 2 .. along a row, the last chroma row then repeated up to whole blocks; level shift and the integer "islow"
 *   forward DCT (13-bit constants, 2 extra bits after the row pass); quantisation by the Annex K tables scaled by quality (scale = 5000 / q
 *   below 50, 200 - 2 q from 50 up; (base scale + 50) / 100 clamped to 1..255), rounding half away from zero; dequantisation; the "islow"
 *   inverse DCT, columns first, clamped to 0..255 after the level shift (the SIMD decoders' saturation; libjpeg's C table wraps beyond
 *   -384..639, which no block of an 8-bit image reaches short of pathological quantisation); h2v2 "fancy" chroma up-sampling (3/4
 *   nearer + 1/4 further sample per axis, the first and last rows / columns of the chroma image taking themselves, biases 8 / 7 for
 *   even / odd columns); YCbCr -> BGR.  Pinned bit for bit against libjpeg-turbo through Pillow (tests/golden/degrade_jpeg.npz).
 *   Optional raw outputs (NULL: not written), with mx = ceil(W / 16), my = ceil(H / 16): coef_y_i16 [B,16 my,16 mx], coef_cb_i16,
 *   coef_cr_i16 [B,8 my,8 mx] the quantised coefficients, block (i, j)'s coefficient (v, u) at (8 i + v, 8 j + u); plane_y_u8
 *   [B,16 my,16 mx], plane_cb_u8, plane_cr_u8 [B,8 my,8 mx] the decoded planes (8-byte aligned).  Blocks beyond ceil(H / 8) x ceil(W / 8)
 *   (chroma: ceil(H / 16) x ceil(W / 16)) come from repeated samples and reach no output pixel.  Untouched for images whose flag is 0. */
enum { SR_DEG_GAUSS_KSIZE = 0, SR_DEG_GAUSS_TAP0 = 1, SR_DEG_MOTION_SIZE = 8, SR_DEG_NOISE_ON = 9, SR_DEG_NOISE_STD = 10, SR_DEG_JPEG_QUALITY = 11,
       SR_DEG_INTERP = 12 /* the host's resize grouping; no kernel reads it */, SR_DEG_PARAMS = 16 };
int  sr_degrade_gauss(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, void* stream);
int  sr_degrade_motion(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, void* stream);
int  sr_degrade_noise(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, const float* field_f32, uint64_t seed,
                      uint8_t* y_u8, float* z_f32, void* stream);
int  sr_degrade_jpeg(sr_ctx* ctx, const uint8_t* x_u8, int B, int H, int W, const int32_t* params_i32, uint8_t* y_u8, int16_t* coef_y_i16,
                     int16_t* coef_cb_i16, int16_t* coef_cr_i16, uint8_t* plane_y_u8, uint8_t* plane_cb_u8, uint8_t* plane_cr_u8, void* stream);
int  sr_degrade_status(sr_ctx* ctx, void* stream);

/* ---- dataset synthesis: smart_square_crop (reference data/common_methods.py:4-49) for a stack of frames, csrc/crop.hip ----
 * B frames of one shape, bgr_u8 DEVICE uint8 [B,H,W,3] in BGR order; 2 <= H, W <= 4096, B <= 32767 (anything else: SR_ERR_INVALID).  The
 * reference thresholds the gray frame with Otsu, takes findContours(RETR_EXTERNAL)'s contour of the largest contourArea, and cuts the
 * square of side S = min(W, H) centred on that contour's boundingRect.  No contour is traced here; each stage is stated as what it computes:
 *   gray      COLOR_BGR2GRAY exactly as the EDA section above states it;
 *   otsu_t    OpenCV 4's getThreshVal_Otsu_8u on the frame's 256-bin histogram h, in fp64, every operation rounded on its own (no fused
 *             multiply-add): scale = 1 / (W H); mu = scale sum_i i h[i], the sum in ascending i; then, from mu1 = q1 = 0, for i = 0 .. 255:
 *             p = h[i] scale; mu1 *= q1; q1 += p; q2 = 1 - q1; i is skipped when min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1 - FLT_EPSILON;
 *             else mu1 = (mu1 + i p) / q1, mu2 = (mu - q1 mu1) / q2, sigma = q1 q2 (mu1 - mu2)^2, and i is kept when sigma exceeds every
 *             earlier sigma (strictly; 0 to begin with).  A constant frame gives 0;
 *   mask      gray > otsu_t (255 / 0);
 *   filled    findContours pads the frame with one ring of background (OpenCV >= 3.2; border pixels count as image).  `outside` is the
 *             4-connected component of the background (mask == 0) that holds that ring: every background pixel 4-connected to the frame's
 *             border.  F = not outside: the foreground, its holes and whatever lies inside them;
 *   labels    the external contours correspond one to one to the 8-connected components of F.  A pixel's label is the smallest raster index
 *             y W + x of its component (the pixel at which the border follower's raster scan starts that contour), -1 outside F;
 *   area      contourArea of a component's traced outer border = sum over the 2 x 2 pixel cells of the frame: 1 for a cell with all four
 *             pixels in the component, 1/2 for exactly three, 0 otherwise (kept as twice the area, an integer);
 *   winner    the component of the largest area; among equal areas the one with the LARGEST label.  (max(contours, key=contourArea) takes
 *             the first maximum of a list that OpenCV returns last-found first.  That order is the one point of this contract that is not
 *             pinned against OpenCV itself, which is installed nowhere this project runs; ties occur only among zero-area contours, single
 *             pixels and one-pixel lines.)  A component nested in another's hole is part of that other's F component and never competes;
 *   box       boundingRect = the winner's pixel bounding box (x, y, ww, hh); cx = x + ww / 2, cy = y + hh / 2 (integer division);
 *             left = max(0, cx - S / 2), top = max(0, cy - S / 2), then pulled back to W - S / H - S where the square would leave the frame.
 *             Without any foreground pixel: found = 0, x = y = ww = hh = 0 and the centre crop left = (W - S) / 2, top = (H - S) / 2.
 * sr_object_boxes: boxes_i32 DEVICE int32 [B,SR_BOX_COLS] in SR_BOX_* order.  Optional raw outputs (NULL: not written): gray_u8, mask_u8
 *   [B,H,W], labels_i32 [B,H,W].  Launches only; every sum is an integer atomic: a frame's row is the same bits on every run and for any B.
 * sr_square_crop: y_u8 DEVICE uint8 [B,S,S,3] = bgr_u8[b, top : top + S, left : left + S] with left, top of the frame's row of boxes_i32
 *   (as sr_object_boxes wrote it, or the caller's own); a left or top outside 0 .. W - S / 0 .. H - S is clamped into that range, so no
 *   table reads outside the frame.  y_u8 must not be bgr_u8.  A square frame is copied whole. */
enum { SR_BOX_FOUND = 0, SR_BOX_X, SR_BOX_Y, SR_BOX_W, SR_BOX_H, SR_BOX_LEFT, SR_BOX_TOP, SR_BOX_OTSU, SR_BOX_COLS };
int  sr_object_boxes(sr_ctx* ctx, const uint8_t* bgr_u8, int B, int H, int W, int32_t* boxes_i32, uint8_t* gray_u8, uint8_t* mask_u8,
                     int32_t* labels_i32, void* stream);
int  sr_square_crop(sr_ctx* ctx, const uint8_t* bgr_u8, int B, int H, int W, const int32_t* boxes_i32, uint8_t* y_u8, void* stream);

/* ---- FineTunedVGG16.fit's per-batch work besides the frozen base (reference VGG16_model.py:111-157), csrc/head_train.hip ----
 * sr_affine_warp: the ImageDataGenerator transform of VGG16_model.py:129-134 as FineTunedVGG16._augment computes it (scipy
 *   affine_transform order=1, mode="nearest", per channel, then the flip), with the batch's gather fused in.  x DEVICE fp32 [N,H,W,C];
 *   idx DEVICE int32 [n], rows of x; params DEVICE fp32 [n,16] per image: the fp64 values a00 a01 a10 a11 o0 o1 split into fp32 hi [0..5]
 *   and lo = x - hi [6..11], flip flag [12] (non-zero: mirror the columns after the warp), [13..15] unused.  Output pixel (oy, ox) samples
 *   (a00 oy + a01 ox + o0, a10 oy + a11 ox + o1) bilinearly, every tap index clamped to the image.  y DEVICE fp32 [n,H,W,C].  An index
 *   outside [0, N) writes NaN for that image and reads nothing.  An integer sample point (identity, flip, integer shift) copies bits.
 * sr_dense_head_step: one step of the head GAP -> Dropout -> Dense(in_dim=512 -> hidden=256, ReLU) -> Dropout -> Dense(num_classes) softmax
 *   with mean sparse categorical CE + l2_reg sum(dense kernel^2) (VGG16_model.py:84-97; the host reference is sr355/train.py head_forward /
 *   head_backward / sparse_cce).  feats DEVICE fp32 [n,512], labels DEVICE int32 [n], params DEVICE fp32: the flat head bucket dense kernel
 *   [512,256], dense bias [256], predictions kernel [256,C], predictions bias [C].  keep0 [n,512] / keep1 [n,256] DEVICE uint8 dropout
 *   keep masks (both or neither, training only); kept values are multiplied by keep_scale = 1 / (1 - rate).  grads DEVICE fp32, the bucket's
 *   layout: training step when non-NULL, inference (no dropout) when NULL.  stats DEVICE fp64 [3]: sum over rows of -log(clip(p[y], 1e-7,
 *   1 - 1e-7)), number of rows whose argmax is y, sum of the dense kernel's squares.  work: sr_dense_head_workspace_bytes(n, C) bytes of
 *   DEVICE memory.  Launches only; every sum runs in a fixed order (no float atomics): the same inputs give the same bits. */
int  sr_affine_warp(sr_ctx* ctx, const float* x, int N, int H, int W, int C, const int32_t* idx, int n, const float* params, float* y,
                    void* stream);
int64_t sr_dense_head_workspace_bytes(int n, int num_classes);
int  sr_dense_head_step(sr_ctx* ctx, const float* feats, int n, int in_dim, int hidden, int num_classes, const int32_t* labels,
                        const uint8_t* keep0, const uint8_t* keep1, float keep_scale, const float* params, float l2_reg, float* grads,
                        double* stats, void* work, int64_t work_bytes, void* stream);
/* Fine-tuning of the conv base's last layers (FineTunedVGG16.setup_model(fine_tune_base=True)): the head step that also returns the gradient
 * at its input, and the backward pass of block5_pool + GlobalAveragePooling2D down to the last conv's pre-activation.
 * sr_dense_head_step_dx: sr_dense_head_step as a training step (grads required) plus dfeats DEVICE fp32 [n,512] = d loss / d feats =
 *   (dz1 k1^T) times the keep0 mask and keep_scale.  grads and stats are the bits sr_dense_head_step writes for the same inputs (the same two
 *   kernels run; a third writes dfeats, its 256-term sums in index order).  params must be 16-byte aligned; n <= 524280.
 * sr_pool_gap_bwd: a DEVICE fp32 [B,H,W,C] the ReLU output of the conv in front of MaxPooling2D(2,2) + GlobalAveragePooling2D, dfeats DEVICE
 *   fp32 [B,C] -> dz DEVICE fp32 [B,H,W,C]: per 2x2 window (floor: an odd last row / column gets zero) dfeats[b,c] / ((H/2)(W/2)) goes to the
 *   first maximum in the order (0,0) (0,1) (1,0) (1,1) -- sr_maxpool2_bwd's rule -- where a > 0, every other element is zero.  Bit for bit the
 *   spread, sr_maxpool2_bwd and SR_ELT_RELU_BWD in sequence.  H, W >= 2.  16-byte accesses when C is a multiple of 4 and the pointers allow. */
int  sr_dense_head_step_dx(sr_ctx* ctx, const float* feats, int n, int in_dim, int hidden, int num_classes, const int32_t* labels,
                           const uint8_t* keep0, const uint8_t* keep1, float keep_scale, const float* params, float l2_reg, float* grads,
                           float* dfeats, double* stats, void* work, int64_t work_bytes, void* stream);
int  sr_pool_gap_bwd(sr_ctx* ctx, const float* a, const float* dfeats, int B, int H, int W, int C, float* dz, void* stream);

/* ---- the discriminator's update inside ESRGAN._train_step besides its convs (reference ESRGAN_model.py:347-377, :475-533), csrc/disc_train.hip ----
 * sr_spectral_norm_bucket: tfa SpectralNormalization.normalize_weights, one power iteration, of n_layers kernels IN PLACE where they lie in a
 *   flat parameter bucket (sr355/train.py ParamBucket), by one launch.  bucket DEVICE fp32 [bucket_len]; u DEVICE fp32 [u_len], every layer's
 *   power-iteration vector; descs HOST [n_layers]: the kernel is bucket[koff : koff + K * Cout] read as w [K, Cout] (K = the product of all axes
 *   but the last), its vector u[uoff : uoff + Cout].  Per layer, in fp64 on the widened fp32 values: v = l2n(u w^T), u' = l2n(v w),
 *   sigma = v w u'^T with l2n(a) = a / sqrt(max(sum a^2, 1e-12)); then kernel <- kernel / float(sigma) (an fp32 division) and u <- u'.  Nothing
 *   else of the bucket is touched.  Any K >= 1 and Cout >= 1.  SR_ERR_INVALID, and no launch, for a null pointer, n_layers <= 0, a descriptor
 *   that reaches past bucket_len / u_len, or two descriptors whose kernels or whose u ranges overlap (each layer is a workgroup of its own).  Every sum runs in a fixed order (no atomics): the same state gives the same bits.
 * sr_disc_head_step: the discriminator's head on the last conv's activation map, forward + loss + backward.  h DEVICE fp32 [B,H,W,in_dim];
 *   params DEVICE fp32: disc_dense1's kernel [in_dim,hidden] and bias [hidden], disc_output's kernel [hidden,out_dim] and bias [out_dim] as they
 *   follow each other in the bucket; (in_dim, hidden, out_dim) must be (256, 256, 1).  g = mean_{H,W} h, z1 = g k1 + b1, a1 = LeakyReLU_0.2(z1),
 *   z2 = a1 k2 + b2, p = sigmoid(z2); loss = mean_B of keras.backend.binary_crossentropy(target, p) on probabilities (clip to [1e-7, 1 - 1e-7],
 *   + 1e-7 inside both logs; the gradient passes only where p lies inside the clip range), target 0 or 1.  Writes *loss (DEVICE fp32, one slot of the
 *   caller's loss buffer), p [B], dh [B,H,W,in_dim] = d loss / d h (d loss / d g spread over the map, / (H W)) and, when grads is non-NULL, the
 *   four parameter gradients into grads (DEVICE fp32, the layout of params: the head's slice of the flat gradient bucket) -- stored, or added
 *   onto what is there when accumulate is non-zero.  Sums in fp64, the batch rows in row order, no atomics. */
typedef struct {
    int64_t koff;       /* first float of the kernel in the bucket */
    int32_t K, Cout;    /* the kernel as a [K, Cout] matrix */
    int64_t uoff;       /* first float of the layer's u in the u tensor */
} sr_sn_desc;
int  sr_spectral_norm_bucket(sr_ctx* ctx, float* bucket, int64_t bucket_len, float* u, int64_t u_len, const sr_sn_desc* descs, int n_layers,
                             void* stream);
int  sr_disc_head_step(sr_ctx* ctx, const float* h, int B, int H, int W, int in_dim, int hidden, int out_dim, const float* params, float target,
                       float* loss, float* p, float* dh, float* grads, int accumulate, void* stream);

/* ---- LPIPS of image pairs: the dataset EDA's first metric (reference data/EDA.ipynb, ImageDatasetAnalyzer.lpips_score / loss_fn), csrc/lpips.hip ----
 * lpips.LPIPS(net="alex"), version 0.1, spatial = False, eval mode.  The lpips package and torchvision are installed nowhere this project runs, so
 * this restates their documented arithmetic and is not pinned against the packages themselves (the caveat the OpenCV paths above carry); the
 * weights are the caller's (torchvision's AlexNet checkpoint and the package's alex.pth), as VGG16's and VGG19's are.
 *   input     uint8 BGR [B,H,W,3] (SR_DTYPE_U8, the EDA's form): x = 2 (v / 255.0) - 1 in fp64, rounded to fp32, BGR -> RGB, then the scaling layer
 *             (x - shift) / scale in fp32 with shift (-.030, -.088, -.188), scale (.458, .448, .450) per R, G, B -- all of it one host-built
 *             [3][256] fp32 table (sr_lpips_input_table) looked up on the device.  fp32 RGB [B,H,W,3] in [-1, 1] (SR_DTYPE_F32): the scaling
 *             layer only, a correctly rounded fp32 subtract and divide.
 *   trunk     torchvision AlexNet `features`, fp32 with fp32 accumulation, floor arithmetic everywhere: conv1 3 -> 64, 11x11, stride 4, zero pad 2
 *             (the zeros pad the scaled image), ReLU = tap 1; max-pool 3x3 stride 2; conv2 64 -> 192, 5x5, pad 2, ReLU = tap 2; max-pool 3x3
 *             stride 2; conv3 192 -> 384, conv4 384 -> 256, conv5 256 -> 256, each 3x3, pad 1, ReLU = taps 3, 4, 5.  conv1's output size is
 *             (n - 7) / 4 + 1, a pool's (n - 3) / 2 + 1; every map needs a pixel, so the smallest image is 31 x 31 (maps 7, 3, 3, 1, 1, 1, 1).
 *             conv1 runs as a 3x3 conv over the 48 channels of the space-to-depth(4) image (csrc/lpips.hip states the identity).
 *   distance  per tap with features fa, fb [h,w,C] and lin weights l[C]: n = f / (sqrt(sum_c f^2) + 1e-10); term = mean_{h,w} sum_c l_c (na_c - nb_c)^2;
 *             score = the sum of the five terms, fp32.  A pixel whose channels are all zero normalises to zeros, never to NaN.
 * sr_lpips_shapes: the five tap sizes hw[l] = {h_l, w_l} of an H x W image.  Pure: no context, no GPU.  SR_ERR_INVALID below 31 or above the EDA's
 *   limits (H, W <= 4096, H W <= 2^22).
 * sr_lpips_input_table: the uint8 form's [3][256] fp32 table, [c][v] for c = R, G, B (HOST, 768 floats).  Pure.
 * sr_lpips_set_weights: conv_w[5] HOST fp32 HWIO [11,11,3,64], [5,5,64,192], [3,3,192,384], [3,3,384,256], [3,3,256,256]; conv_b[5] their
 *   biases; lin_w[5] HOST fp32 [64], [192], [384], [256], [256].  Copies and packs for the kernels once (no per-call packing); the caller's arrays
 *   are not kept.  All three NULL (or every entry NULL) unloads and frees; anything between is SR_ERR_INVALID.  Waits for the device.
 * sr_lpips: a, b DEVICE [B,H,W,3] of `dtype` -> score_B DEVICE fp32 [B].  Optional (NULL: not written): terms_Bx5 DEVICE fp32 [B,5], the five
 *   terms; taps HOST array of five DEVICE fp32 pointers (each may be NULL), taps[l] = [2,B,h_l,w_l,C_l], the raw ReLU features of a then of b
 *   (16-byte aligned; for tests).  SR_ERR_STATE "the weights are not set" without weights; SR_ERR_INVALID, and no launch, for a shape
 *   sr_lpips_shapes refuses, B < 1 or B > 2^20.  The 2 n images of n pairs go through the trunk as one batch; B pairs are processed in chunks
 *   of n = min(SR_LPIPS_CHUNK_PAIRS, SR_LPIPS_WORK_BYTES / one pair's maps) pairs, at least one, so the workspace (counted in sr_mem_info,
 *   kept between calls, freed with the weights) stays below SR_LPIPS_WORK_BYTES unless a single pair needs more (26.6 MB per pair at 478 x 478).
 *   Launches only, asynchronous on `stream`.  Every sum runs in an order fixed by the map sizes (no atomics, no split-K): a pair's five terms
 *   and score are the same bits on every run, for any B and at any position in the batch -- the guarantee sr_eda_pair_stats gives. */
enum { SR_LPIPS_CHUNK_PAIRS = 64, SR_LPIPS_WORK_BYTES = 256 << 20 };
int  sr_lpips_shapes(int H, int W, int hw[5][2]);
int  sr_lpips_input_table(float* table_3x256);
int  sr_lpips_set_weights(sr_ctx* ctx, const float* const conv_w[5], const float* const conv_b[5], const float* const lin_w[5]);
int  sr_lpips(sr_ctx* ctx, const void* a, const void* b, int dtype, int B, int H, int W, float* score_B, float* terms_Bx5, float* const taps[5],
              void* stream);

/* ---- training batches cut from device-resident image stacks (reference SRModels/loading_methods.py:40-191, load_dataset_as_patches and its
 * add_padding), csrc/patch_dataset.hip ----
 * sr_gather_patch_pairs: ONE launch writes a batch of aligned LR / HR patches.  Each side (sr_patch_side) is a stack src DEVICE [N,H,W,3] of
 *   `dtype` SR_DTYPE_U8 or SR_DTYPE_F32 (chosen per side) and a destination out DEVICE fp32: lr->out [B,patch_h,patch_w,3], hr->out
 *   [B,patch_h*scale,patch_w*scale,3].  hr may be NULL (one-sided: the whole-image conversion below).  windows DEVICE int32 [n_windows,3]: image
 *   index, y, x in LR-side pixels of the padded image; order DEVICE int32 [n_order]: rows of `windows`; batch element b is window
 *   order[offset + b], 0 <= offset, offset + B <= n_order.  The HR window starts at (y*scale, x*scale).  Per element:
 *     padding  add_padding's bottom / right reflect as np.pad(mode="reflect") indexes it: row i >= H of the padded image is row 2 (H - 1) - i.
 *              pad_h / pad_w are the caller's, per side; a pad > H - 1 (W - 1) would reflect twice and is SR_ERR_INVALID, as is a patch
 *              larger than the padded image.
 *     order    swap_rb != 0 exchanges channels 0 and 2 (BGR stacks -> the loader's RGB).
 *     uint8    float(u) / 255.0f, a correctly rounded fp32 division: np.float32(u) / 255.0 for all 256 codes (u * (1 / 255.0f) is not: it differs
 *              in 126 of them).
 *     scaling  then v * mul + add, product and sum rounded separately, skipped when mul == 1 and add == 0 (ESRGAN's x * 2 - 1).
 *   One whole-image window per image (patch_h = H, patch_w = W, pads 0) converts a uint8 stack to fp32 [0,1].
 *   Safety: the kernel clamps every order entry, image index and window origin into range, so no table reads outside the stacks, whatever it
 *   holds (a clamped entry gives another valid window, not an error: the host validates tables before upload).  SR_ERR_INVALID, and no
 *   launch, for a null pointer, a dtype other than the two, N, H, W, B, patch or scale < 1, offset < 0 or offset + B > n_order, n_windows < 1,
 *   a pad outside 0 .. n - 1, a patch larger than a side's padded image, or a batch of 2^31 values or more.
 * sr_gather_warp_patches: ONE launch writes an augmented batch y DEVICE fp32 [B,patch_h,patch_w,3] of the classifier's fit
 *   (load_defects_dataset_as_patches, loading_methods.py:194-285, then VGG16_model.py:129-134) from a frame stack src DEVICE [N,H,W,3] of
 *   `dtype` SR_DTYPE_U8 or SR_DTYPE_F32.  windows, order, n_order, offset, B and swap_rb as in sr_gather_patch_pairs (no padding: the
 *   defects loader's windows never reach it); params DEVICE fp32 [B,16] in sr_affine_warp's layout (fp64 values split hi / lo, flip flag at
 *   [12]).  Batch element b is, bit for bit, what sr_affine_warp returns for the patch a one-sided sr_gather_patch_pairs (pads 0) cuts for
 *   window order[offset + b]: output pixel (oy, ox) samples PATCH coordinates (a00 oy + a01 ox + o0, a10 oy + a11 ox + o1) in the same
 *   double-float arithmetic, both tap indices clamped to the patch ([0, patch_h - 1], [0, patch_w - 1]: the frame's pixels next to the window
 *   never enter), the flip mirrors over patch_w, a uint8 tap is float(u) / 255.0f correctly rounded (an fp32 tap its stored bits), and the
 *   four taps are combined by the same rounded products and sums.  An integer sample point (identity, flip, integer shift) copies the
 *   gathered value exactly.  The coordinates are computed once per pixel and serve its three channels.
 *   Safety: every order entry and image index is clamped into range and the window origin into [0, H - patch_h] x [0, W - patch_w], so no
 *   table reads outside the stack (the host validates tables before upload).  SR_ERR_INVALID, and no launch, for a null pointer, a dtype
 *   other than the two, N, H, W, B or a patch size < 1, a patch larger than the frame (or >= 2^24), offset < 0 or offset + B > n_order,
 *   n_windows < 1, B > 65535, or a batch of 2^31 values or more.
 * sr_clip_by_norm_bucket: tf.clip_by_norm per variable of a flat fp32 gradient bucket, in place (sr355/train.py Adam.apply): table DEVICE
 *   int64 [n_vars,2] = (offset, length) per variable; nrm = sqrt(sum g^2) accumulated in fp64 from the fp32 values; where nrm > clipnorm,
 *   g *= float(clipnorm / nrm) (fp64 division, rounded to fp32, one fp32 product per element); scales_out DEVICE fp32 [n_vars] receives the
 *   factor, 1 where the variable was left alone.  One workgroup of 1024 threads per variable: thread t sums elements t, t + 1024, ... in
 *   index order, the 1024 partial sums are added pairwise in a fixed tree (no atomics): the same bucket gives the same bits on every run.
 *   A table entry is clamped into [0, bucket_len]; overlapping entries are the caller's error (the host builds the table from the bucket's
 *   shapes).  SR_ERR_INVALID for a null pointer, n_vars outside 1 .. 65535, bucket_len < 1 or a clipnorm that is not finite and positive. */
typedef struct {
    const void* src;            /* DEVICE [N,H,W,3] */
    float* out;                 /* DEVICE fp32 batch */
    int32_t dtype;              /* SR_DTYPE_U8 or SR_DTYPE_F32 */
    int32_t N, H, W;            /* the stack, unpadded */
    int32_t pad_h, pad_w;       /* bottom / right reflect padding */
    int32_t swap_rb;
    float mul, add;
} sr_patch_side;
int  sr_gather_patch_pairs(sr_ctx* ctx, const sr_patch_side* lr, const sr_patch_side* hr, const int32_t* windows, int n_windows,
                           const int32_t* order, int64_t n_order, int64_t offset, int B, int patch_h, int patch_w, int scale, void* stream);
int  sr_gather_warp_patches(sr_ctx* ctx, const void* src, int dtype, int N, int H, int W, const int32_t* windows, int n_windows,
                            const int32_t* order, int64_t n_order, int64_t offset, int B, int patch_h, int patch_w, int swap_rb,
                            const float* params, float* y, void* stream);
int  sr_clip_by_norm_bucket(sr_ctx* ctx, float* flat_g, int64_t bucket_len, const int64_t* table, int n_vars, double clipnorm, float* scales_out,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SR355_H */
