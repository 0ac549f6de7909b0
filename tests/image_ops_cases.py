"""Case tables of tests/test_image_ops_gpu.py, and the host-side choices of csrc/imgops.hip they are built around, restated.

`bicubic_route` restates bicubic_launch's choice between bicubic_f32_tile_kernel and the per-pixel kernels together with the tile
kernel's dynamic-LDS byte count; `resize_route` restates resize_launch's choice among its kernels, the LINEAR-halving -> AREA
rewrite and the RS_MAXT refusal.  The constants come out of the source by regex, so a changed constant moves the predicates with
it and tests/test_image_ops_cases_cpu.py then reports the predicate side that lost its witness, instead of the cases silently
changing kernels.  Nothing here touches a GPU.
"""
import math
import os
import re
from collections import namedtuple

import numpy as np

from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGOPS = os.path.join(ROOT, "super-resolution-images-for-3d-printing-defect-detection_amd", "csrc", "imgops.hip")


def _constants():
    src = open(IMGOPS).read()
    out = {}
    for name in ("BT_X", "BT_Y", "BT_WIN", "BT_ROWS", "RS_MAXT"):
        m = re.search(r"constexpr\s+int\b[^;]*\b%s\s*=\s*(\d+)" % name, src)
        assert m, f"{name} not found in {IMGOPS}"
        out[name] = int(m.group(1))
    return out


K = _constants()
BT_X, BT_Y, BT_WIN, BT_ROWS, RS_MAXT = (K[n] for n in ("BT_X", "BT_Y", "BT_WIN", "BT_ROWS", "RS_MAXT"))
# bicubic_launch starts the tile kernel without raising its dynamic-LDS attribute.  A C = 4 window can ask for more than 64 KB; the
# runtime serves such a launch on gfx950 as it is (a CU has 160 KB; DESIGN.md, image ops), so the size is no term of the predicate.
# The tables keep a case on each side of 64 KB all the same.
DEFAULT_LDS_LIMIT = 65536

NEAREST, LINEAR, CUBIC, AREA, LANCZOS4 = O.INTER_NEAREST, O.INTER_LINEAR, O.INTER_CUBIC, O.INTER_AREA, O.INTER_LANCZOS4

# ------------------------------------------------------------------------------------------------ bicubic_launch
BicubicRoute = namedtuple("BicubicRoute", "kernel win_rows win lds C_ok win_ok rows_ok sy sx")


def bicubic_route(dtype, shape, out):
    """dtype "f32" / "u8", shape (B, H, W, C), out (oH, oW) -> BicubicRoute; kernel is "tile", "pixel" or "u8".  The entry points
    sr_bicubic / sr_resize always ask for a dense output of the input's type, so those two terms of the predicate are constant."""
    B, H, W, C = shape
    oH, oW = out
    sy, sx = 1.0 / (float(oH) / float(H)), 1.0 / (float(oW) / float(W))
    win_rows = int(BT_Y * sy) + 6
    win = (int(BT_X * sx) + 6) * win_rows * C
    C_ok, win_ok, rows_ok = C <= 4, win <= BT_WIN, win_rows <= BT_ROWS
    lds = (win + max(win_rows, BT_Y) * BT_X * C) * 4
    grid_ok = B <= 65535 and (oH + BT_Y - 1) // BT_Y <= 65535
    if dtype == "u8":
        kernel = "u8"
    else:
        kernel = "tile" if (C_ok and win_ok and rows_ok and grid_ok) else "pixel"
    return BicubicRoute(kernel, win_rows, win, lds, C_ok, win_ok, rows_ok, sy, sx)


# id, dtype, (B, H, W, C), (oH, oW)
BICUBIC_CASES = [
    # ---- tile route
    ("tile_c1", "f32", (1, 10, 10, 1), (37, 23)),
    ("tile_c2_ragged_xy_b2", "f32", (2, 9, 13, 2), (20, 300)),           # 2 x 3 tiles per image, last ones 44 columns / 4 rows
    ("tile_c3_ragged_xy_b2", "f32", (2, 5, 40, 3), (13, 300)),
    ("tile_c3_b3", "f32", (3, 23, 31, 3), (46, 62)),
    ("tile_c4", "f32", (1, 8, 8, 4), (24, 24)),
    ("tile_c4_lds_above_64k", "f32", (1, 24, 24, 4), (30, 60)),          # win_rows == BT_ROWS, 69 888 bytes of LDS
    ("tile_c3_lds_max_win_edge", "f32", (1, 8, 25, 3), (10, 39)),        # win_rows == BT_ROWS, 170 window columns: one more would not fit
    ("tile_c1_x_downscale", "f32", (1, 4, 60, 1), (40, 45)),             # shrinking in x alone still fits the window
    ("tile_tiny_source_clamped", "f32", (1, 3, 5, 3), (130, 70)),        # every tap clamped somewhere
    # ---- per-pixel route, one reason each
    ("pixel_c5", "f32", (1, 6, 7, 5), (18, 21)),
    ("pixel_rows_13", "f32", (1, 9, 5, 3), (10, 20)),                    # win_rows == BT_ROWS + 1, window fits
    ("pixel_win_171_columns", "f32", (1, 8, 20, 3), (10, 31)),           # win_rows == BT_ROWS, 171 window columns: 12 floats over
    ("pixel_downscale_b2", "f32", (2, 21, 17, 3), (9, 11)),
    ("pixel_downscale_c1", "f32", (1, 33, 20, 1), (8, 7)),
    # ---- uint8 (one kernel)
    ("u8_up_b3", "u8", (3, 9, 11, 3), (31, 40)),
    ("u8_down_b2", "u8", (2, 37, 29, 3), (11, 13)),
    ("u8_c1_ragged", "u8", (2, 7, 5, 1), (17, 23)),
    ("u8_c4_mixed", "u8", (1, 12, 30, 4), (29, 11)),                     # up in y, down in x
]


# ------------------------------------------------------------------------------------------------ resize_launch
ResizeRoute = namedtuple("ResizeRoute", "kernel rewritten TX TY shrink")


def _taps(interp, area_up, ns, nd):
    if interp == LANCZOS4:
        return 8
    if interp == AREA and not area_up:
        return int(math.ceil(float(ns) / nd)) + 2
    return 2


def resize_route(dtype, shape, out, interp):
    """-> ResizeRoute; kernel is one of "bicubic", "nearest", "area_fast_u8", "area_taps_u8", "fixed_u8", "float_taps", "refused";
    rewritten says that an INTER_LINEAR halving was turned into INTER_AREA first; shrink that both axes shrink or keep their size."""
    B, H, W, C = shape
    oH, oW = out
    shrink = oW <= W and oH <= H
    if interp == CUBIC:
        return ResizeRoute("bicubic", False, 4, 4, shrink)
    if interp == NEAREST:
        return ResizeRoute("nearest", False, 1, 1, shrink)
    assert interp in (LINEAR, AREA, LANCZOS4)
    rewritten = interp == LINEAR and W == 2 * oW and H == 2 * oH
    if rewritten:
        interp = AREA
    area_up = interp == AREA and not shrink
    if dtype == "u8" and interp == AREA and not area_up and W % oW == 0 and H % oH == 0:
        return ResizeRoute("area_fast_u8", rewritten, W // oW, H // oH, shrink)
    TX, TY = _taps(interp, area_up, W, oW), _taps(interp, area_up, H, oH)
    if TX > RS_MAXT or TY > RS_MAXT:
        return ResizeRoute("refused", rewritten, TX, TY, shrink)
    if dtype == "f32":
        return ResizeRoute("float_taps", rewritten, TX, TY, shrink)
    if interp == AREA and not area_up:
        return ResizeRoute("area_taps_u8", rewritten, TX, TY, shrink)
    return ResizeRoute("fixed_u8", rewritten, TX, TY, shrink)


REFUSAL_MESSAGE = "resize: INTER_AREA shrink factor above 14 is not supported"

# id, dtype, (B, H, W, C), (oH, oW), interpolation
RESIZE_CASES = [
    # ---- float taps
    ("f32_linear_up", "f32", (2, 9, 13, 3), (20, 31), LINEAR),
    ("f32_linear_shrink", "f32", (2, 37, 50, 3), (11, 17), LINEAR),          # factors 3.36 / 2.94: no rewrite
    ("f32_linear_halving", "f32", (2, 22, 18, 3), (11, 9), LINEAR),          # rewritten to AREA
    ("f32_lanczos_up", "f32", (1, 9, 11, 2), (20, 25), LANCZOS4),
    ("f32_lanczos_shrink", "f32", (2, 37, 50, 3), (11, 17), LANCZOS4),
    ("f32_area_up", "f32", (1, 9, 13, 3), (20, 13), AREA),                   # one axis kept, one enlarged: linear taps in area coordinates
    ("f32_area_shrink", "f32", (2, 37, 50, 1), (11, 17), AREA),
    ("f32_area_factor_14", "f32", (1, 28, 10, 1), (2, 7), AREA),             # exactly 14 in y: TY == RS_MAXT
    ("f32_area_factor_15", "f32", (1, 30, 10, 1), (2, 7), AREA),             # refused
    ("f32_nearest", "f32", (2, 17, 9, 3), (40, 5), NEAREST),
    ("f32_cubic_shrink", "f32", (2, 37, 50, 3), (11, 17), CUBIC),
    # ---- uint8, three independent images each
    ("u8_linear_up", "u8", (3, 9, 13, 3), (20, 31), LINEAR),
    ("u8_linear_shrink", "u8", (3, 37, 50, 3), (11, 17), LINEAR),
    ("u8_linear_halving", "u8", (3, 22, 18, 3), (11, 9), LINEAR),            # rewritten, then the whole-number box mean
    ("u8_lanczos_up", "u8", (3, 9, 11, 1), (20, 25), LANCZOS4),
    ("u8_lanczos_shrink", "u8", (3, 37, 50, 3), (11, 17), LANCZOS4),
    ("u8_area_up", "u8", (3, 9, 13, 3), (20, 31), AREA),
    ("u8_area_fast_3x5", "u8", (3, 36, 45, 3), (12, 9), AREA),
    ("u8_area_fast_15", "u8", (1, 30, 15, 1), (2, 1), AREA),                 # whole-number factor 15: no tap table, not refused
    ("u8_area_taps", "u8", (3, 37, 50, 3), (11, 17), AREA),
    ("u8_area_taps_factor_14", "u8", (3, 28, 10, 3), (2, 7), AREA),
    ("u8_area_taps_factor_15", "u8", (1, 30, 10, 3), (2, 7), AREA),          # refused
    ("u8_nearest", "u8", (3, 17, 9, 3), (40, 5), NEAREST),
    ("u8_cubic_shrink", "u8", (3, 37, 50, 3), (11, 17), CUBIC),
]

# one case per kernel for the guard-band test
GUARD_BICUBIC = ["tile_c2_ragged_xy_b2", "pixel_downscale_b2", "u8_up_b3"]
GUARD_RESIZE = ["f32_nearest", "u8_nearest", "u8_area_fast_3x5", "u8_area_taps", "u8_linear_up", "f32_lanczos_up"]


def case_rng(cid):
    return np.random.default_rng(sum(ord(c) * (i + 1) for i, c in enumerate(cid)) % (2 ** 31))


def case_input(cid, dtype, shape):
    """U[0,1) floats / uniform bytes; every image of the batch is its own draw."""
    rng = case_rng(cid)
    if dtype == "f32":
        return rng.uniform(0, 1, shape).astype(np.float32)
    return rng.integers(0, 256, shape, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ uint8 saturation
def saturation_image():
    """[24, 30, 3] uint8: 0 / 255 steps of width 5 (rows and columns), a one-pixel checkerboard, and random bytes."""
    rng = np.random.default_rng(41)
    img = rng.integers(0, 256, (24, 30, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:24, 0:30]
    steps = (((yy // 5) + (xx // 5)) % 2 * 255).astype(np.uint8)
    checker = ((yy + xx) % 2 * 255).astype(np.uint8)
    img[:, :12] = steps[:, :12, None]
    img[:, 12:22] = checker[:, 12:22, None]
    return img


# (interpolation, (oH, oW)) on saturation_image(): up and down, no whole-number factor
SATURATION_RUNS = [(CUBIC, (53, 71)), (CUBIC, (17, 19)), (LANCZOS4, (53, 71)), (LANCZOS4, (17, 19))]


# ------------------------------------------------------------------------------------------------ reductions
# shape, per-image noise sd
REDUCE_CASES = [
    ((3, 300, 300, 3), (0.5, 0.05, 0.0005)),      # 270 000 elements per image: more than the 1024 x 256 threads of a grid row
    ((2, 1, 1, 1), (0.5, 0.05)),
    ((2, 1, 85, 3), (0.5, 0.0005)),               # 255
    ((1, 1, 257, 1), (0.05,)),
]
MAX_REDUCE_BLOCKS, REDUCE_BLOCK = 1024, 256       # psnr_launch / mse_launch


def reduce_pair(shape, sds):
    rng = np.random.default_rng(shape[1] * 1000 + shape[2])
    a = rng.uniform(0, 1, shape).astype(np.float32)
    b = a.copy()
    for i, sd in enumerate(sds):
        b[i] = (a[i] + sd * rng.standard_normal(shape[1:])).astype(np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------ SSIM
SSIM_TILE = 32                                    # windows per tile side (ST in ssim_partial_kernel)
SSIM_MEAN_SHAPES = [(2, 11, 11, 3), (1, 11, 75, 2), (1, 75, 11, 4), (2, 42, 42, 1), (1, 43, 43, 1), (1, 43, 43, 2), (2, 43, 43, 3),
                    (1, 43, 43, 4)]


def ssim_pair(shape):
    rng = np.random.default_rng(shape[1] * 100 + shape[2] + shape[3])
    a = rng.uniform(0, 1, shape)
    b = np.clip(a + 0.05 * rng.standard_normal(shape), 0, 1)
    return a.astype(np.float32), b.astype(np.float32)


SSIM_255_SHAPE = (2, 43, 50, 3)
# |O.ssim(float32) - O.ssim(float64)| on ssim_255_pair(), measured on the CPU: 1.2e-06 per image at most.
# Four times that is below the floor, so the bound is the floor.
SSIM_255_FP32_GAP = 1.2e-06
SSIM_255_FLOOR = 5e-5


def ssim_255_pair():
    """A [0, 255] image whose windows have a variance of the order of c2 = (0.03 * 255)^2: a ramp over the full range along x plus a
    little texture, and b = a + noise.  SSIM is invariant under a common scaling of the images AND max_val, so on a full-contrast
    image the constants hardly matter; here a kernel that ignored max_val would be off by 0.1."""
    rng = np.random.default_rng(255)
    B, H, W, C = SSIM_255_SHAPE
    a = np.clip(np.linspace(0, 1, W)[None, None, :, None] + 0.02 * rng.uniform(-1, 1, SSIM_255_SHAPE), 0, 1)
    b = np.clip(a + 0.05 * rng.standard_normal(SSIM_255_SHAPE), 0, 1)
    return (a * 255.0).astype(np.float32), (b * 255.0).astype(np.float32)


def ssim_255_bound(a, b):
    gap = float(np.max(np.abs(O.ssim(a, b, max_val=255.0, dtype=np.float32).astype(np.float64) - O.ssim(a, b, max_val=255.0, dtype=np.float64))))
    return max(4.0 * gap, SSIM_255_FLOOR), gap


# localised test: 75 x 75 x 3, 65 x 65 windows = 3 x 3 tiles (32, 32, 1 windows a side); b differs from a in one 6 x 6 block
SSIM_LOCAL_HW, SSIM_LOCAL_BLOCK = 75, 6
SSIM_LOCAL_DELTA = 128.0                          # added to the block: see ssim_local_pair
SSIM_LOCAL_BLOCKS = {                             # name -> (y0, x0) of the block
    "seam_x_tile0_tile1": (12, 34),               # windows 24..39 in x: both sides of 31 | 32
    "seam_y_tile0_tile1": (34, 12),
    # the same seams met by the block's fringe, where the deficit climbs steeply from window to window (in the middle of the block
    # neighbouring windows both lose about 1, and one taken for the other would hardly move the sum)
    "seam_x_fringe_left": (12, 27),               # windows 17..32 in x: window 32, the first of tile 1, sees the block's last column only
    "seam_x_fringe_right": (12, 41),              # windows 31..46 in x: window 31, the last of tile 0, sees the block's first column only
    "seam_y_fringe_above": (27, 12),
    "seam_y_fringe_below": (41, 12),
    "last_window_column": (20, 69),               # windows 59..64 in x: the one-window tile column
    "last_window_row": (69, 20),
    "corner": (69, 69),
    "origin": (0, 0),
}
SSIM_MIN_DEFICIT = 0.02


def ssim_local_pair(name):
    """A window that meets the block only with its corner pixel weighs it with g[0]^2 = 1.06e-6.  For that window to lose 0.02 the
    block's change must carry a variance of the order of the image's own (1/12) through that weight: delta^2 * 1e-6 ~ 1e-2, so delta
    is of order 100.  128 keeps a + delta on a coarse fp32 grid."""
    rng = np.random.default_rng(75)
    a = rng.uniform(0, 1, (1, SSIM_LOCAL_HW, SSIM_LOCAL_HW, 3)).astype(np.float32)
    b = a.copy()
    y0, x0 = SSIM_LOCAL_BLOCKS[name]
    n = SSIM_LOCAL_BLOCK
    b[0, y0:y0 + n, x0:x0 + n, :] += np.float32(SSIM_LOCAL_DELTA)
    return a, b


def affected_windows(name):
    """(ys, xs): the window rows / columns whose 11 x 11 footprint meets the block."""
    y0, x0 = SSIM_LOCAL_BLOCKS[name]
    nwin = SSIM_LOCAL_HW - 10
    rng_ = lambda p: range(max(0, p - 10), min(nwin - 1, p + SSIM_LOCAL_BLOCK - 1) + 1)
    return rng_(y0), rng_(x0)


def ssim_window_deficits(a, b, name):
    """|1 - s_w| of every affected window and channel from the fp64 reference: each window is an 11 x 11 single-channel image."""
    ys, xs = affected_windows(name)
    ca = np.stack([a[0, y:y + 11, x:x + 11, c:c + 1] for y in ys for x in xs for c in range(a.shape[3])])
    cb = np.stack([b[0, y:y + 11, x:x + 11, c:c + 1] for y in ys for x in xs for c in range(a.shape[3])])
    return np.abs(1.0 - O.ssim(ca, cb, dtype=np.float64))


def ssim_deficit_sum(a, b, ssim_value):
    """D = (1 - ssim) * oH * oW * C: the summed deficit of all windows."""
    return (1.0 - float(ssim_value)) * (a.shape[1] - 10) * (a.shape[2] - 10) * a.shape[3]


# ------------------------------------------------------------------------------------------------ patches
# (H, W), patch, stride
PATCH_CASES = [((50, 37), 24, 12), ((48, 48), 48, 24), ((25, 30), 24, 12),
               ((13, 14), 24, 12)]                # pad 12 of 13 rows, 12 of 14 columns: the last sizes the pad < size rule lets through
PATCH_REFUSED = ((12, 30), 24, 12)                # pad 12 of 12 rows
OVERLAP_SCALES = [1, 2, 4]


def overlap_counts(hw, patch, stride):
    """How many patches cover each pixel of the padded image."""
    ph, pw = hw[0] + O.pad_amount(hw[0], patch, stride), hw[1] + O.pad_amount(hw[1], patch, stride)
    cnt = np.zeros((ph, pw), np.int64)
    for i, j in O.patch_positions(ph, pw, patch, stride):
        cnt[i:i + patch, j:j + patch] += 1
    return cnt
