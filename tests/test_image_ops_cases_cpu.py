"""The case tables of tests/image_ops_cases.py reach every side of every term of the launch predicates they restate, and the
oracle-only conditions test_image_ops_gpu.py relies on hold.  No GPU: the routes come from the restated predicates, whose constants
are read out of csrc/imgops.hip, so a changed constant or a deleted sole witness fails here."""
import numpy as np
import pytest

import image_ops_cases as T
from oracle import ops as O


def _bicubic():
    return [(cid, shape, out, T.bicubic_route(dtype, shape, out)) for cid, dtype, shape, out in T.BICUBIC_CASES]


def _resize():
    return [(cid, dtype, shape, out, interp, T.resize_route(dtype, shape, out, interp)) for cid, dtype, shape, out, interp in T.RESIZE_CASES]


def test_constants_are_the_ones_the_tables_were_built_for():
    """The tables below hold witnesses for whatever the constants are; this only documents the values in use."""
    assert all(v > 0 for v in T.K.values())
    assert T.BT_X == 256 and T.BT_Y == 8       # threads per block / rows per tile of bicubic_f32_tile_kernel: the kernel's own layout


def test_case_ids_are_unique_and_guard_cases_exist():
    for table in (T.BICUBIC_CASES, T.RESIZE_CASES):
        ids = [c[0] for c in table]
        assert len(ids) == len(set(ids))
    assert set(T.GUARD_BICUBIC) <= {c[0] for c in T.BICUBIC_CASES}
    assert set(T.GUARD_RESIZE) <= {c[0] for c in T.RESIZE_CASES}


def test_guard_band_cases_name_one_case_per_kernel():
    """The per-element GPU tests put every case behind guard bands; these lists name the minimum set, one per kernel."""
    rows = {c[0]: c for c in T.BICUBIC_CASES + T.RESIZE_CASES}
    assert [T.bicubic_route(*rows[c][1:]).kernel for c in T.GUARD_BICUBIC] == ["tile", "pixel", "u8"]
    ragged = rows[T.GUARD_BICUBIC[0]]
    assert ragged[3][1] > T.BT_X and ragged[3][1] % T.BT_X and ragged[3][0] % T.BT_Y
    got = {(rows[c][1], T.resize_route(*rows[c][1:]).kernel) for c in T.GUARD_RESIZE}
    assert got == {("f32", "nearest"), ("u8", "nearest"), ("u8", "area_fast_u8"), ("u8", "area_taps_u8"), ("u8", "fixed_u8"), ("f32", "float_taps")}


def test_bicubic_tile_route_cases():
    tile = [(cid, shape, out, r) for cid, shape, out, r in _bicubic() if r.kernel == "tile"]
    for C in (1, 2, 3, 4):
        assert any(shape[3] == C for _, shape, _, _ in tile), f"no tile-route case with C = {C}"
    assert any(out[1] > T.BT_X and out[1] % T.BT_X for _, _, out, _ in tile), "no tile-route case with a ragged last tile in x"
    assert any(out[0] % T.BT_Y for _, _, out, _ in tile), "no tile-route case with a ragged last tile in y"
    assert any(shape[0] > 1 for _, shape, _, _ in tile), "no tile-route case with B > 1"
    assert any(out[1] > T.BT_X and out[1] % T.BT_X and out[0] % T.BT_Y and out[0] > T.BT_Y and shape[0] > 1 for _, shape, out, _ in tile), \
        "no batched tile-route case ragged on both axes with more than one tile each way"
    assert any(r.sx > 1.0 for _, _, _, r in tile), "no tile-route case that shrinks in x"


def test_bicubic_per_pixel_route_for_each_reason_alone():
    pix = [(cid, shape, out, r) for cid, shape, out, r in _bicubic() if r.kernel == "pixel"]
    assert any(shape[3] == 5 and r.win_ok and r.rows_ok for _, shape, _, r in pix), "no case that is per-pixel for C = 5 alone"
    assert any(r.C_ok and r.win_ok and r.win_rows == T.BT_ROWS + 1 for _, _, _, r in pix), "no case with win_rows = BT_ROWS + 1 while win fits"
    assert any(r.C_ok and r.rows_ok and not r.win_ok for _, _, _, r in pix), "no case with win > BT_WIN while win_rows fits"
    assert any(r.C_ok and r.sy > 1.0 and r.sx > 1.0 for _, _, _, r in pix), "no down-scale case"
    for _, shape, _, r in pix:                      # and each is per-pixel for a reason the predicate names
        assert not (r.C_ok and r.win_ok and r.rows_ok)


def test_bicubic_limits():
    tile = [r for _, _, _, r in _bicubic() if r.kernel == "tile"]
    assert any(r.win_rows == T.BT_ROWS for r in tile), "no tile-route case with win_rows == BT_ROWS"
    col = lambda r, C: r.win_rows * C              # floats one more window column costs
    both = [(shape[3], r) for _, shape, _, r in _bicubic()]
    assert any(r.kernel == "tile" and T.BT_WIN - r.win < col(r, C) for C, r in both), "no tile-route case within one tap column of BT_WIN"
    assert any(r.kernel == "pixel" and r.rows_ok and 0 < r.win - T.BT_WIN <= col(r, C) for C, r in both), "no per-pixel case one tap column over BT_WIN"
    assert any(r.lds > T.DEFAULT_LDS_LIMIT for r in tile), "no tile-route case above the default dynamic-LDS limit"
    assert any(r.lds <= T.DEFAULT_LDS_LIMIT for r in tile)
    # the C = 3 maximum: BT_ROWS window rows and as many window columns as BT_WIN admits
    assert any(C == 3 and r.kernel == "tile" and r.win_rows == T.BT_ROWS and T.BT_WIN - r.win < col(r, 3) for C, r in both), "no case at the C = 3 LDS maximum"
    assert all(r.lds <= (T.BT_WIN + T.BT_ROWS * T.BT_X * 3) * 4 for C, r in both if C == 3 and r.kernel == "tile")


def test_bicubic_u8_cases():
    u8 = [(shape, out) for cid, dtype, shape, out in T.BICUBIC_CASES if dtype == "u8"]
    assert any(s[0] > 1 for s, _ in u8), "no batched uint8 bicubic"
    assert any(o[0] < s[1] and o[1] < s[2] for s, o in u8), "no uint8 down-scale"
    assert any(s[3] == 1 for s, _ in u8), "no single-channel uint8 bicubic"
    assert any(o[0] % 2 and o[1] % 2 and o[0] % s[1] and o[1] % s[2] for s, o in u8), "no ragged uint8 size"


def test_resize_routes():
    rows = _resize()
    for dtype, kernel in (("f32", "nearest"), ("u8", "nearest"), ("u8", "area_fast_u8"), ("u8", "area_taps_u8"), ("u8", "fixed_u8"),
                          ("f32", "float_taps"), ("f32", "refused"), ("u8", "refused"), ("f32", "bicubic"), ("u8", "bicubic")):
        assert any(dt == dtype and r.kernel == kernel for _, dt, _, _, _, r in rows), f"no {dtype} case on the {kernel} route"
    for dtype in ("f32", "u8"):
        assert any(dt == dtype and r.rewritten for _, dt, _, _, _, r in rows), f"no {dtype} LINEAR halving"
    for kernel in ("nearest", "area_fast_u8", "area_taps_u8", "fixed_u8", "bicubic"):
        assert any(dt == "u8" and r.kernel == kernel and shape[0] == 3 for _, dt, shape, _, _, r in rows), f"no uint8 {kernel} case with B = 3"
    # the fixed-point kernel's two vertical forms: 2 x 2 taps (VResizeLinear) and the generic shift
    assert any(r.kernel == "fixed_u8" and (r.TX, r.TY) == (2, 2) for *_, r in rows)
    assert any(r.kernel == "fixed_u8" and (r.TX, r.TY) == (8, 8) for *_, r in rows)


def test_resize_shrinking_with_every_interpolation():
    rows = _resize()
    whole = lambda shape, out: shape[1] % out[0] == 0 or shape[2] % out[1] == 0
    for dtype in ("f32", "u8"):
        for interp in (T.LINEAR, T.CUBIC, T.LANCZOS4):
            assert any(dt == dtype and ip == interp and out[0] < shape[1] and out[1] < shape[2] and not whole(shape, out) and not r.rewritten
                       for _, dt, shape, out, ip, r in rows), f"no {dtype} shrinking case with interpolation {interp}"


def test_resize_area_factor_limit():
    rows = _resize()
    for dtype in ("f32", "u8"):
        at = [r for _, dt, shape, out, ip, r in rows if dt == dtype and ip == T.AREA and shape[1] == 14 * out[0]]
        over = [r for _, dt, shape, out, ip, r in rows if dt == dtype and ip == T.AREA and shape[1] == 15 * out[0] and shape[2] % out[1]]
        assert at and all(r.kernel in ("float_taps", "area_taps_u8") and r.TY == T.RS_MAXT for r in at), f"{dtype}: factor 14 must sit exactly on RS_MAXT"
        assert over and all(r.kernel == "refused" and r.TY == T.RS_MAXT + 1 for r in over), f"{dtype}: factor 15 must be refused"
    # a whole-number factor of 15 on both axes needs no tap table and is served
    assert any(r.kernel == "area_fast_u8" and r.TY == 15 for *_, r in rows)


def test_saturation_image_clips_at_both_ends_in_the_reference():
    img = T.saturation_image()
    assert img.dtype == np.uint8 and (img == 0).any() and (img == 255).any()
    for interp, out in T.SATURATION_RUNS:
        pre = O.bicubic_resize_u8(img, out[0], out[1], preclip=True) if interp == T.CUBIC else O.cv_resize_u8(img, out[0], out[1], interp, preclip=True)
        assert pre.min() < 0 and pre.max() > 255, (interp, out, int(pre.min()), int(pre.max()))
        ref = O.bicubic_resize_u8(img, out[0], out[1]) if interp == T.CUBIC else O.cv_resize_u8(img, out[0], out[1], interp)
        assert np.array_equal(ref, np.clip(pre, 0, 255).astype(np.uint8))
    ups = [o for _, o in T.SATURATION_RUNS if o[0] > img.shape[0] and o[1] > img.shape[1]]
    downs = [o for _, o in T.SATURATION_RUNS if o[0] < img.shape[0] and o[1] < img.shape[1]]
    assert {i for i, _ in T.SATURATION_RUNS} == {T.CUBIC, T.LANCZOS4} and len(ups) == 2 and len(downs) == 2


def test_reduction_sizes():
    per_image = [int(np.prod(shape[1:])) for shape, _ in T.REDUCE_CASES]
    assert any(n > T.MAX_REDUCE_BLOCKS * T.REDUCE_BLOCK for n in per_image), "no image larger than one capped grid row: the grid-stride loop never runs"
    assert {1, 255, 257} <= set(per_image)
    big = [(shape, sds) for shape, sds in T.REDUCE_CASES if np.prod(shape[1:]) > T.MAX_REDUCE_BLOCKS * T.REDUCE_BLOCK]
    assert any(shape[0] >= 3 and max(sds) / min(sds) >= 100 for shape, sds in big), "the large batch must hold images of very different error"
    for shape, sds in T.REDUCE_CASES:
        a, b = T.reduce_pair(shape, sds)
        assert len(sds) == shape[0] and all((a[i] != b[i]).any() for i in range(shape[0]))


def test_ssim_mean_shapes():
    hw = {(s[1], s[2]) for s in T.SSIM_MEAN_SHAPES}
    assert {(11, 11), (11, 75), (75, 11), (42, 42), (43, 43)} <= hw
    assert T.SSIM_TILE + 10 == 42
    assert {s[3] for s in T.SSIM_MEAN_SHAPES} == {1, 2, 3, 4}
    assert any(s[0] > 1 for s in T.SSIM_MEAN_SHAPES)


def test_ssim_255_bound_is_the_measured_one():
    a, b = T.ssim_255_pair()
    assert a.max() == 255 and a.min() == 0 and a.shape == T.SSIM_255_SHAPE
    bound, gap = T.ssim_255_bound(a, b)
    assert gap <= 1.5 * T.SSIM_255_FP32_GAP, gap          # the figure recorded beside the case still describes the input
    assert bound == max(4 * gap, T.SSIM_255_FLOOR)
    # the constants matter on this input: the same images scored with max_val = 1 are 0.09 away
    assert np.min(np.abs(O.ssim(a, b, max_val=1.0, dtype=np.float64) - O.ssim(a, b, max_val=255.0, dtype=np.float64))) > 1000 * bound


@pytest.mark.parametrize("name", sorted(T.SSIM_LOCAL_BLOCKS))
def test_ssim_local_sensitivity_floor(name):
    """Every window that meets the block loses at least SSIM_MIN_DEFICIT in the fp64 reference, every other window is identical in a
    and b, and the summed deficit of the reference is the affected windows' alone."""
    a, b = T.ssim_local_pair(name)
    y0, x0 = T.SSIM_LOCAL_BLOCKS[name]
    n = T.SSIM_LOCAL_BLOCK
    diff = (a != b).any(axis=(0, 3))
    assert diff[y0:y0 + n, x0:x0 + n].all() and diff.sum() == n * n
    d = T.ssim_window_deficits(a, b, name)
    assert d.min() >= T.SSIM_MIN_DEFICIT, float(d.min())
    D = T.ssim_deficit_sum(a, b, O.ssim(a, b, dtype=np.float64)[0])
    assert abs(D - d.sum()) <= 1e-9 * d.size + 1e-9 * D      # s_w <= 1 + tiny here, so |1 - s_w| sums to D up to sign conventions
    ys, xs = T.affected_windows(name)
    t = T.SSIM_TILE
    if name.startswith("seam_x"):
        assert xs[0] < t <= xs[-1] and ys[-1] < t
    if name.startswith("seam_y"):
        assert ys[0] < t <= ys[-1] and xs[-1] < t
    if name.endswith("fringe_left") or name.endswith("fringe_above"):
        assert (xs if "_x_" in name else ys)[-1] == t            # the first window of tile 1 is the last one affected
    if name.endswith("fringe_right") or name.endswith("fringe_below"):
        assert (xs if "_x_" in name else ys)[0] == t - 1         # the last window of tile 0 is the first one affected
    if name == "last_window_column":
        assert xs[-1] == 2 * t and ys[-1] < t
    if name == "last_window_row":
        assert ys[-1] == 2 * t and xs[-1] < t
    if name == "corner":
        assert ys[-1] == 2 * t and xs[-1] == 2 * t


def test_ssim_local_blocks_cover_the_seams():
    assert T.SSIM_LOCAL_HW - 10 == 2 * T.SSIM_TILE + 1      # 3 x 3 tiles, the last a single window
    assert {"seam_x_tile0_tile1", "seam_y_tile0_tile1", "last_window_column", "last_window_row", "corner"} <= set(T.SSIM_LOCAL_BLOCKS)


def test_patch_cases():
    assert {((50, 37), 24, 12), ((48, 48), 48, 24), ((25, 30), 24, 12)} <= set(T.PATCH_CASES)
    for hw, p, s in T.PATCH_CASES:
        assert O.pad_amount(hw[0], p, s) < hw[0] and O.pad_amount(hw[1], p, s) < hw[1]
        cnt = T.overlap_counts(hw, p, s)[:hw[0], :hw[1]]
        assert set(np.unique(cnt)) <= {1, 2, 4}, np.unique(cnt)      # sums and quotients of k/64 values stay exact
    hw, p, s = T.PATCH_REFUSED
    assert O.pad_amount(hw[0], p, s) == hw[0] or O.pad_amount(hw[1], p, s) == hw[1]      # the limit itself
    assert any(O.pad_amount(hw[0], p, s) == hw[0] - 1 for hw, p, s in T.PATCH_CASES)     # and the size just inside it
    assert any(np.unique(T.overlap_counts(hw, p, s)[:hw[0], :hw[1]]).size == 3 for hw, p, s in T.PATCH_CASES)
