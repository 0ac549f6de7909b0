"""Capped 1-D launch grids of csrc/*.hip and *.h: the caps, read out of the source text, every launch site that uses one, and the
case tables of tests/test_grid_caps_gpu.py -- for each site the smallest input whose thread count, as the host code computes it,
exceeds the cap, so that the kernel's grid-stride loop goes round a second, shorter time.

`CAPS` holds each cap in threads; `capped_sites()` finds the launch sites by a search of the source; `CASES` names the sites each
case crosses, with the thread count restated from the launch code; `COVERED_ELSEWHERE` and `UNREACHABLE` account for the rest with
a reason each.  tests/test_grid_caps_cpu.py holds the three together.  Nothing here touches a GPU.
"""
import os
import re
from collections import namedtuple

from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd", "csrc")
BLOCK = 256

# clamp helper -> the file that defines it (imgops.hip and study.hip each have a grid_for of their own)
HELPERS = {"train_ops.hip": "grid_n", "imgops.hip": "grid_for", "study.hip": "grid_for", "classic.hip": "cls_grid", "metrics.hip": "met_grid",
           "eda.hip": "grid1d"}
_NUM = r"(\d+(?:\s*(?:\*|<<)\s*\d+)*)"                         # 65535, 256 * 8 * 4, 1 << 20
# the inline idioms: std::min(... / 256, K), std::min<int64_t>((n + 255) / 256, K), g > K ? K : g
_INLINE = [re.compile(r"std::min(?:<\w+>)?\(\s*\([^;]*?\+\s*255\)\s*/\s*256\s*,\s*" + _NUM + r"\s*\)"),
           re.compile(r">\s*" + _NUM + r"\s*\?\s*\1\s*:")]


def _value(expr):
    assert re.fullmatch(r"[\d\s*<]+", expr), expr
    return int(eval(expr))                                      # digits, * and << only


def source_files(csrc=CSRC):
    return sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))


def helper_cap(text, name):
    """Blocks a clamp helper lets through, from its body: `g > K ? K : g`, K a number or a `cap = <product>` defined beside it."""
    m = re.search(r"unsigned\s+%s\s*\(int64_t n[^)]*\)\s*\{(.*?)\n?\}" % name, text, re.S)
    assert m, f"clamp helper {name} not found"
    body = m.group(1)
    k = re.search(r"g\s*>\s*(\w+)\s*\?\s*\1\s*:\s*g", body)
    assert k, f"{name}: no clamp expression"
    if k.group(1).isdigit():
        return int(k.group(1))
    d = re.search(r"\b%s\s*=\s*%s\s*[;,]" % (k.group(1), _NUM), body)
    assert d, f"{name}: {k.group(1)} is not defined in the helper"
    return _value(d.group(1))


def _launches(text):
    """(kernel, grid argument, offset) of every hipLaunchKernelGGL statement."""
    out = []
    for m in re.finditer(r"hipLaunchKernelGGL\(", text):
        depth, i, args, start = 1, m.end(), [], m.end()
        while depth and len(args) < 2:                          # a kernel name with a comma in its template list stands in parentheses
            ch = text[i]
            depth += (ch == "(") - (ch == ")")
            if ch == "," and depth == 1:
                args.append(text[start:i].strip())
                start = i + 1
            i += 1
        assert len(args) == 2, text[m.start():m.start() + 120]
        kernel = re.sub(r"^\(|\)$", "", args[0])
        out.append((re.sub(r"\s+", "", kernel), args[1], m.start()))
    return out


def _function_start(text, pos):
    """Offset of the last line before `pos` that opens a function at column 0 (or inside `extern "C"` / a namespace: no indentation)."""
    starts = [m.start() for m in re.finditer(r"^[A-Za-z_][^\n;]*\)\s*\{\s*$|^[A-Za-z_][^\n;]*,\s*$", text[:pos], re.M)]
    return starts[-1] if starts else 0


def capped_sites(csrc=CSRC):
    """{(file, kernel): cap in threads per grid row} of every launch whose 1-D grid extent goes through a clamp helper or an inline
    clamp -- in the launch statement itself, or in the definition of a variable the grid argument names, within the same function."""
    sites = {}
    for f in source_files(csrc):
        text = open(os.path.join(csrc, f)).read()
        helper = HELPERS.get(f)
        hcap = helper_cap(text, helper) if helper else None
        for kernel, grid, pos in _launches(text):
            cap = None
            scope = text[_function_start(text, pos):pos]
            exprs = [grid]
            for ident in set(re.findall(r"[A-Za-z_]\w*", grid)):
                # the latest definition of that name before the launch, in this function
                defs = re.findall(r"\b(?:const\s+)?(?:unsigned|int|int64_t|dim3)\s+%s\b\s*(?:=|\()([^;]*);" % ident, scope)
                if defs:
                    exprs.append(defs[-1])
            for e in exprs:
                for rx in _INLINE:
                    for m in rx.finditer(e):
                        v = _value(m.group(1))
                        cap = v if cap is None else min(cap, v)
                if helper and re.search(r"\b%s\(" % helper, e) and (cap is None or hcap < cap):
                    cap = hcap
            if cap is not None:
                key = (f, kernel)
                assert sites.get(key, cap * BLOCK) == cap * BLOCK, f"{key}: two launches with different caps"
                sites[key] = cap * BLOCK
    return sites


def _caps():
    out = {}
    for f, helper in HELPERS.items():
        out[f] = helper_cap(open(os.path.join(CSRC, f)).read(), helper) * BLOCK
    return out


CAPS = _caps()                                                   # file -> threads its clamp helper lets through
SITES = capped_sites()
TRAIN_CAP, IMG_CAP, STUDY_CAP, CLS_CAP, MET_CAP = (CAPS[f] for f in ("train_ops.hip", "imgops.hip", "study.hip", "classic.hip", "metrics.hip"))
PAIRS_CAP = SITES[("patch_dataset.hip", "gather_patch_pairs_kernel")]
WARP_PATCH_CAP = SITES[("patch_dataset.hip", "gather_warp_patches_kernel")]
AFFINE_CAP = SITES[("head_train.hip", "affine_warp_kernel<4>")]
CROP_MASK_CAP = SITES[("crop.hip", "crop_mask_kernel")]
PACK_CAP = SITES[("conv.hip", "pack_weights_f32_kernel")]

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC, O.INTER_AREA, O.INTER_LANCZOS4

# id: the test's name for it; sites: the (file, kernel) launches it takes past their cap; cap: threads of one round (per grid row
# where the grid has a y extent); threads: what the host code hands the clamp, restated from the launch; per_thread: output
# elements one thread writes per round (the flat index of a mismatch divided by cap * per_thread is its round); arg: the shape
Case = namedtuple("Case", "id sites cap threads per_thread arg")
CASES = []


def _case(cid, file, kernels, cap, threads, arg, per_thread=1):
    CASES.append(Case(cid, tuple((file, k) for k in ([kernels] if isinstance(kernels, str) else kernels)), cap, int(threads), per_thread, arg))


def patch_grid(H, W, patch, stride):
    return ((H + O.pad_amount(H, patch, stride) - patch) // stride + 1, (W + O.pad_amount(W, patch, stride) - patch) // stride + 1)


# ------------------------------------------------------------------------------------------------ train_ops.hip
ADAM_N = TRAIN_CAP + 257
_case("adam", "train_ops.hip", "adam_kernel", TRAIN_CAP, ADAM_N, ADAM_N)
_case("eltwise", "train_ops.hip", "eltwise_kernel", TRAIN_CAP, ADAM_N, ADAM_N)
VIEW_NPIX, VIEW_C, VIEW_BUFS = 524289, 32, (40, 48, 36)          # a, b, out buffers' channel counts
_case("eltwise_view", "train_ops.hip", "eltwise_view_kernel", TRAIN_CAP, VIEW_NPIX * VIEW_C, (VIEW_NPIX, VIEW_C))
S2D_X, S2D_R = (1, 4098, 4096, 1), 2
_case("space_to_depth", "train_ops.hip", "space_to_depth_kernel", TRAIN_CAP, (4098 // 2) * (4096 // 2) * 4, S2D_X)
POOL_BWD_X = (1, 4097, 4096, 1)
_case("maxpool2_bwd", "train_ops.hip", "maxpool2_bwd_kernel", TRAIN_CAP, 4097 * 4096, POOL_BWD_X)
_case("zero_insert2", "train_ops.hip", "zero_insert2_kernel", TRAIN_CAP, 4097 * 4096, POOL_BWD_X)

# ------------------------------------------------------------------------------------------------ imgops.hip
RS_OUT = (837, 836)
RS_N = RS_OUT[0] * RS_OUT[1] * 3                                 # 2 099 196 = cap + 2044
# id, dtype, (B, H, W, C), interpolation, kernel: resize_launch counts output ELEMENTS
RESIZE_CASES = [
    ("nearest_f32", "f32", (1, 419, 418, 3), NEAREST, "resize_nearest_kernel<float>"),
    ("nearest_u8", "u8", (1, 419, 418, 3), NEAREST, "resize_nearest_kernel<uint8_t>"),
    ("linear_f32", "f32", (1, 419, 418, 3), LINEAR, "resize_apply_f32_kernel"),
    ("lanczos_f32", "f32", (1, 419, 418, 3), LANCZOS4, "resize_apply_f32_kernel"),
    ("area_up_f32", "f32", (1, 419, 418, 3), AREA, "resize_apply_f32_kernel"),
    ("area_frac_f32", "f32", (1, 1255, 1254, 3), AREA, "resize_apply_f32_kernel"),
    ("linear_u8", "u8", (1, 419, 418, 3), LINEAR, "resize_apply_u8_kernel"),
    ("lanczos_u8", "u8", (1, 419, 418, 3), LANCZOS4, "resize_apply_u8_kernel"),
    ("area_up_u8", "u8", (1, 419, 418, 3), AREA, "resize_apply_u8_kernel"),
    ("area_whole_u8", "u8", (1, 1674, 1672, 3), AREA, "resize_area_fast_u8_kernel"),
    ("area_frac_u8", "u8", (1, 1255, 1254, 3), AREA, "resize_apply_area_u8_kernel"),
]
for _id, _dt, _shape, _ip, _k in RESIZE_CASES:
    _case("resize_" + _id, "imgops.hip", _k, IMG_CAP, _shape[0] * RS_N // 3 * _shape[3], (_dt, _shape, RS_OUT, _ip))
# bicubic_launch counts output PIXELS (one thread serves a pixel's channels), so three images of 837 x 836 make the 2 099 196
# id, dtype, (B, H, W, C), kernel
BICUBIC_CASES = [
    ("pixel_down_f32", "f32", (3, 1674, 1672, 1), "bicubic_f32_kernel"),     # shrinking by 2: the window of a tile has 22 rows > BT_ROWS
    ("pixel_c5_up_f32", "f32", (3, 419, 418, 5), "bicubic_f32_kernel"),      # C > 4
    ("u8_up", "u8", (3, 419, 418, 1), "bicubic_u8_kernel"),
    ("u8_down_c3", "u8", (3, 1255, 1254, 3), "bicubic_u8_kernel"),
]
for _id, _dt, _shape, _k in BICUBIC_CASES:
    _case("bicubic_" + _id, "imgops.hip", _k, IMG_CAP, _shape[0] * RS_OUT[0] * RS_OUT[1], (_dt, _shape, RS_OUT), per_thread=_shape[3])
PATCH_HW, PATCH, STRIDE = (456, 456), 48, 24                     # padded by 24 to 480 x 480: 19 x 19 = 361 patches of 6912 values, 2 495 232
_ny, _nx = patch_grid(*PATCH_HW, PATCH, STRIDE)
PATCH_COUNT = _ny * _nx
_case("extract_patches", "imgops.hip", "extract_patches_kernel", IMG_CAP, PATCH_COUNT * PATCH * PATCH * 3, (PATCH_HW, PATCH, STRIDE))
OVERLAP_HW = {1: (837, 836), 2: (419, 418)}                      # scale -> (H, W): the output is H * scale x W * scale x 3
for _s, _hw in OVERLAP_HW.items():
    _case(f"overlap_add_x{_s}", "imgops.hip", "overlap_add_kernel", IMG_CAP, _hw[0] * _s * _hw[1] * _s * 3, (_hw, PATCH, STRIDE, _s))
PICK2_X = (1, 1025, 1025, 8)                                     # SP_PICK2: 513 x 513 x 8 outputs
_case("pick2", "imgops.hip", "subsample2_kernel", IMG_CAP, 513 * 513 * 8, PICK2_X)
PREPROC_X = (1, 837, 836, 3)                                     # SP_VGG_PREPROCESS: npix * 3
_case("vgg_preprocess", "imgops.hip", "vgg_preproc_kernel", IMG_CAP, RS_N, PREPROC_X)
PAD_X = (1, 725, 725, 3)                                         # a thin fp32 conv pads 3 channels to 4: 525 625 * 4 elements of the padded copy
_case("convert_pad", "imgops.hip", "convert_pad_kernel", IMG_CAP, 725 * 725 * 4, PAD_X)
REDUCE_BLOCKS = 1024                                             # psnr_launch / mse_launch / l1_launch clamp grid_for's result again
L1_SHAPE = (3, 300, 301, 3)                                      # 812 700 elements against 1024 x 256 threads: three rounds and a part
_case("l1", "imgops.hip", "absdiff_partial_kernel", REDUCE_BLOCKS * BLOCK, 3 * 300 * 301 * 3, L1_SHAPE)
# VGG16 in bf16 on one 1027 x 1026 image, layer by layer: block 1's pool writes 513 x 513 x 64 values, eight per thread; the taps on it
# and on the conv in front of it (1027 x 1026 x 64 values) go through tap_copy_kernel, one value per thread
POOL_X8 = (1, 1027, 1026, 3)
_case("maxpool2_bf16x8", "imgops.hip", "maxpool2_bf16x8_kernel", IMG_CAP, 513 * 513 * 64 // 8, POOL_X8, per_thread=8)
_case("tap_copy", "imgops.hip", "tap_copy_kernel", IMG_CAP, 513 * 513 * 64, POOL_X8)

# The ESRGAN generator in bf16 moves the trunk's 64 channels into the dense blocks' row-blocked concat buffer and back, one 16-byte
# unit (8 values) per thread, in the layout choose_layout (api.hip) picks: two 24-pixel-wide images per 48-pixel row when every fused
# dense-block path is on (pack_pairs pads an odd batch to an even one); a cell grid when none is and the grid fills the tiles better
# (24 x 24 does, 32 x 32 does not); the plain row-blocked layout otherwise.
ESRGAN_CASES = {"two_up": (457, 24, 24), "cells": (457, 24, 24), "blocked": (257, 32, 32)}
_case("esrgan_two_up", "imgops.hip", ("pack_pairs_kernel", "unpack_pairs_kernel"), IMG_CAP, 457 * 24 * 24 * 64 // 8, ESRGAN_CASES["two_up"], per_thread=8)
_case("esrgan_cells", "imgops.hip", ("cell_pack_kernel", "cell_unpack_kernel"), IMG_CAP, 457 * 24 * 24 * 64 // 8, ESRGAN_CASES["cells"], per_thread=8)
_case("esrgan_blocked", "imgops.hip", "nhwc_to_blocked_kernel", IMG_CAP, 257 * 32 * 32 * 64 // 8, ESRGAN_CASES["blocked"], per_thread=8)

# ------------------------------------------------------------------------------------------------ study.hip
QUAD_FRAMES = (4,) + PATCH_HW + (3,)                             # patch * C % 4 == 0: four values per thread
_case("extract_batch_quad", "study.hip", ("extract_batch_quad_kernel<TIn>",), STUDY_CAP, 4 * PATCH_COUNT * PATCH * PATCH * 3 // 4, (QUAD_FRAMES, PATCH, STRIDE),
      per_thread=4)
SCALAR_PATCH, SCALAR_STRIDE = 11, 5                              # patch * C = 33
_sny, _snx = patch_grid(200, 200, SCALAR_PATCH, SCALAR_STRIDE)
SCALAR_FRAMES = (-(-(STUDY_CAP + 1) // (_sny * _snx * SCALAR_PATCH * SCALAR_PATCH * 3)), 200, 200, 3)
_case("extract_batch_scalar", "study.hip", ("extract_batch_scalar_kernel<TIn>",), STUDY_CAP,
      SCALAR_FRAMES[0] * _sny * _snx * SCALAR_PATCH * SCALAR_PATCH * 3, (SCALAR_FRAMES, SCALAR_PATCH, SCALAR_STRIDE))

# ------------------------------------------------------------------------------------------------ patch_dataset.hip
PAIRS_B, PAIRS_PATCH, PAIRS_SCALE = 228, 24, 4                   # 228 * (24^2 + 96^2) = 2 232 576 pixels, three values each
_case("gather_patch_pairs", "patch_dataset.hip", "gather_patch_pairs_kernel", PAIRS_CAP, PAIRS_B * (PAIRS_PATCH ** 2 + (PAIRS_PATCH * PAIRS_SCALE) ** 2),
      (PAIRS_B, PAIRS_PATCH, PAIRS_SCALE), per_thread=3)
WARP_PATCH = (513, 512)                                          # pixels of one patch; the cap holds per batch element
_case("gather_warp_patches", "patch_dataset.hip", "gather_warp_patches_kernel", WARP_PATCH_CAP, 513 * 512, (2,) + WARP_PATCH, per_thread=3)

# ------------------------------------------------------------------------------------------------ head_train.hip
_case("affine_warp_v4", "head_train.hip", "affine_warp_kernel<4>", AFFINE_CAP, 592 * 592 * 3 // 4, (2, 592, 592, 3), per_thread=4)
_case("affine_warp_scalar", "head_train.hip", "affine_warp_kernel<1>", AFFINE_CAP, 513 * 513, (2, 513, 513, 1))

# ------------------------------------------------------------------------------------------------ crop.hip
CROP_FRAME = (513, 512)
_case("crop_mask", "crop.hip", "crop_mask_kernel", CROP_MASK_CAP, 513 * 512, (3,) + CROP_FRAME)

# ------------------------------------------------------------------------------------------------ classic.hip, metrics.hip
CLS_B, CLS_HR, CLS_LR = 294, 478, 239
CLS_NH, CLS_NL = CLS_B * CLS_HR * CLS_HR, CLS_B * CLS_LR * CLS_LR
_case("classic_hr", "classic.hip", ("ibp_init_kernel", "ibp_hr_kernel", "egi_hr_kernel"), CLS_CAP, CLS_NH, (CLS_B, CLS_HR, CLS_HR))
_case("classic_lr", "classic.hip", ("ibp_lr_kernel", "sobel_mag_kernel"), CLS_CAP, CLS_NL, (CLS_B, CLS_LR, CLS_LR))
FREQ_B, FREQ_HW = 4200, 64                                       # 4200 images of 64 x 64 = 17 203 200 bytes widened
_case("u8_to_f64", "classic.hip", "u8_to_f64_kernel", CLS_CAP, FREQ_B * FREQ_HW * FREQ_HW, (FREQ_B, FREQ_HW, FREQ_HW))
_case("rgb2gray", "metrics.hip", ("rgb2gray_kernel<true>", "rgb2gray_kernel<false>"), MET_CAP, (CLS_NH + 3) // 4, (CLS_B, CLS_HR, CLS_HR, 3), per_thread=4)
SIGMA_B, SIGMA_HW = 16385, 61                                    # db2 detail band of 61 x 61: 32 x 32 coefficients per image
_case("noise_sigma", "classic.hip", "db2_hh_abs_kernel", CLS_CAP, SIGMA_B * ((SIGMA_HW + 3) // 2) ** 2, (SIGMA_B, SIGMA_HW, SIGMA_HW))

# ------------------------------------------------------------------------------------------------ eda.hip
# sr_eda_pair_stats with a caller's DCT buffer works on chunks of EDA_CHUNK_BYTES / (16 HW) images: 4096 images of 64 x 64 make one
# chunk of exactly 2^24 gray values, 256 more than grid1d lets through
EDA_CHUNK_BYTES = _value(re.search(r"EDA_CHUNK_BYTES\s*=\s*\(size_t\)\s*" + _NUM, open(os.path.join(CSRC, "eda.hip")).read()).group(1))
EDA_PAIRS, EDA_HW = 2048, 64
EDA_CHUNK = min(2 * EDA_PAIRS, EDA_CHUNK_BYTES // (16 * EDA_HW * EDA_HW))
_case("eda_dct", "eda.hip", "gray_to_f64_kernel", CAPS["eda.hip"], EDA_CHUNK * EDA_HW * EDA_HW, (EDA_PAIRS, EDA_HW, EDA_HW))

# ------------------------------------------------------------------------------------------------ conv.hip
PACK_KERNEL = (3, 3, 512, 512)
_case("pack_weights_f32", "conv.hip", "pack_weights_f32_kernel", PACK_CAP, 3 * 3 * 512 * 512, PACK_KERNEL)

BY_ID = {c.id: c for c in CASES}


def images_crossed(cap, per_image, count):
    """Indices of the images (of per_image elements each) inside which a round of `cap` threads ends."""
    return sorted({(k * cap) // per_image for k in range(1, (count - 1) // cap + 1)})


# ------------------------------------------------------------------------------------------------ the sites without a case here
# (file, kernel) -> the test that takes the launch past its cap, and what it compares
COVERED_ELSEWHERE = {
    ("imgops.hip", "maxpool2_kernel"): "test_classifier_ops_gpu.py::test_maxpool2_signed_and_odd at (6, 194, 130, 64): 2 421 120 outputs, bit for bit "
                                       "O.maxpool2x2",
    ("imgops.hip", "sqdiff_partial_kernel"): "test_image_ops_gpu.py::test_psnr_mse_sizes at (3, 300, 300, 3): 270 000 elements per image (psnr) and 810 000 "
                                             "(mse) against 1024 x 256 threads per grid row; 2e-4 dB / 1e-5 relative of fp64",
}
# (file, kernel) -> why no test crosses it: what an input would have to be, from the launch code
UNREACHABLE = {
    ("metrics.hip", "gray_f64_kernel"): "a chunk holds FFT_CHUNK_BYTES / (24 HW) images, at most 2^28 / 24 = 11.2 M values; only a single image above "
                                        "16 776 960 pixels (a side of 4096) crosses, and its score needs the operator below",
    ("cgemm_f64.h", "dft_full_operator_kernel"): "one thread per element of an N x N operator: N >= 4096, an image side of 4096 or more (the dataset's is 478); "
                                                 "the fp64 reference of the nine scores at that size takes minutes",
    ("classic.hip", "dft_operator_kernel"): "one thread per element of an N x n operator, n sincospi terms each: N n > 16 776 960 means 7e10 fp64 sincospi "
                                            "evaluations on the device and hours for the NumPy restatement",
    ("eda.hip", "dct_operator_kernel"): "one thread per element of an N x N operator: N >= 4096, an image side of 4096 or more",
    ("degrade.hip", "degrade_motion_kernel"): "the cap is 2^20 blocks: more than 2^28 output bytes, a stack of 392 frames of 478 x 478 x 3, whose "
                                              "reference (degrade_ref, frame by frame in Python) takes minutes",
}
