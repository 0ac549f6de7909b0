"""The square crop without a device: the contour-free restatement the device implements (tests/crop_ref.py: hole filling, 8-connected
components, the 2 x 2 cell area, the pixel bounding box) against what it replaces, a Suzuki-Abe outer-border follower with the shoelace
area; the flood fill against scipy.ndimage where that is installed; hand-computed Otsu thresholds; the box arithmetic at its clamps; and
the argument checks of data.common_methods.square_crop_batch / synthesize_pairs, which run before any device is touched.  Every comparison
is exact equality."""
import numpy as np
import pytest

import crop_ref as R


def components(mask):
    """The 8-connected components of the hole-filled mask, as bool images, in raster order of their first pixel."""
    lab = R.label(R.fill_holes(mask), 8)
    return [lab == r for r in np.unique(lab[lab >= 0])]


def check_traced_equals_counted(mask):
    comps = components(mask)
    for c in comps:
        pts = R.trace_outer_border(c)
        assert R.shoelace_area2(pts) == R.cell_area2(c)
        assert R.points_bbox(pts) == R.pixel_bbox(c)
    return len(comps)


def random_masks():
    rng = np.random.default_rng(2024)
    for k in range(160):
        H, W = (int(v) for v in rng.integers(3, 20, 2))
        m = rng.random((H, W)) < rng.choice([0.3, 0.5, 0.7])
        if k % 3 == 1:                                            # dilated: blobs with holes
            p = np.pad(m, 1)
            m = p[1:-1, 1:-1] | p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:]
        elif k % 3 == 2:                                          # eroded: thin remains and single pixels
            p = np.pad(m, 1)
            m = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[1:-1, :-2]
        yield m


def test_traced_area_and_rectangle_equal_the_cell_count_on_random_masks():
    n = sum(check_traced_equals_counted(m) for m in random_masks())
    assert n >= 300, n


def named_shapes():
    z = lambda H=9, W=11: np.zeros((H, W), bool)
    s = {}
    m = z(); m[4, 5] = True; s["single pixel"] = m
    m = z(); m[3, 2:9] = True; s["horizontal line"] = m
    m = z(); m[1:8, 6] = True; s["vertical line"] = m
    m = z(); m[np.arange(1, 8), np.arange(2, 9)] = True; s["diagonal line"] = m
    m = z(); m[np.arange(1, 8), 9 - np.arange(1, 8)] = True; s["anti-diagonal line"] = m
    m = z(); m[1:8, 2:9] = True; m[3:6, 4:7] = False; s["ring"] = m
    m = z(11, 13); m[1:10, 1:12] = True; m[3:8, 3:10] = False; m[5, 5:8] = True; s["ring with a blob inside its hole"] = m
    s["checkerboard"] = R.checkerboard(8, 9)
    m = z(); m[1:4, 1:5] = True; m[4:8, 5:9] = True; s["two blobs touching only at a corner"] = m
    m = z(); m[4, :] = True; m[:, 5] = True; s["component touching all four image edges"] = m
    s["all foreground"] = np.ones((5, 6), bool)
    s["spiral"] = R.spiral(19, 17)
    s["serpentine"] = R.serpentine(13, 15)
    s["nested rings"] = R.nested_rings(23, 25)
    return s


@pytest.mark.parametrize("name", sorted(named_shapes()))
def test_traced_area_and_rectangle_equal_the_cell_count_on_named_shapes(name):
    assert check_traced_equals_counted(named_shapes()[name]) >= 1


def test_named_shapes_are_what_their_names_say():
    s = named_shapes()
    one = lambda m: len(components(m))
    assert one(s["ring with a blob inside its hole"]) == 1          # the blob lies inside the ring's filled hole: one external contour
    assert one(s["two blobs touching only at a corner"]) == 1       # 8-connectivity
    assert one(s["checkerboard"]) == 1 and one(s["spiral"]) == 1 and one(s["serpentine"]) == 1 and one(s["nested rings"]) == 1
    assert R.cell_area2(s["single pixel"]) == 0 and R.cell_area2(s["diagonal line"]) == 0 and R.cell_area2(s["horizontal line"]) == 0
    assert R.cell_area2(R.fill_holes(s["ring"])) == 2 * 6 * 6       # 7 x 7 pixels: the contour runs through the pixel centres
    lab = R.label(s["spiral"], 4)
    assert (lab[s["spiral"]] == 0).all()                            # one 4-connected line from the first pixel on


def test_fill_holes_keeps_background_that_reaches_the_border_only_diagonally_inside():
    m = np.zeros((5, 5), bool)
    m[1, 2] = m[2, 1] = m[2, 3] = m[3, 2] = True                    # a diamond: its centre is 4-enclosed -> a hole
    assert R.fill_holes(m)[2, 2] and R.fill_holes(m).sum() == 5
    m[1, 2] = False                                                 # opened: the centre reaches the outside
    assert not R.fill_holes(m)[2, 2]
    b = np.ones((4, 4), bool)
    b[0, 0] = False                                                 # a background pixel on the frame's border joins the ring: not a hole
    assert not R.fill_holes(b)[0, 0]


def test_flood_fill_agrees_with_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for m in list(random_masks())[:60] + list(named_shapes().values()):
        assert np.array_equal(R.fill_holes(m), ndi.binary_fill_holes(m))
        for conn, st in ((4, ndi.generate_binary_structure(2, 1)), (8, np.ones((3, 3), bool))):
            mine = R.label(m, conn)
            theirs, n = ndi.label(m, structure=st)
            assert len(np.unique(mine[mine >= 0])) == n
            for k in range(1, n + 1):                               # same partition, and my label is the component's smallest raster index
                assert (mine[theirs == k] == np.flatnonzero(theirs == k)[0]).all()


def test_otsu_by_hand():
    for v in (0, 7, 200, 255):
        assert R.otsu(np.full((6, 5), v, np.uint8)) == 0            # one class only: every step is skipped
    for a, b in ((0, 255), (10, 11), (3, 200), (100, 254)):
        g = np.array([a, b] * 18, np.uint8).reshape(6, 6)
        assert R.otsu(g) == a                                       # sigma is the same for a <= t < b; the first wins (strict >)
    g = np.array([10] * 30 + [20] * 3 + [200] * 30, np.uint8)       # the small middle class joins the nearer side
    assert 20 <= R.otsu(g) < 200
    h = np.zeros(256, np.int64)
    h[[5, 250]] = 1
    h[100] = 1 << 25
    assert R.otsu_from_hist(h) == 0                                 # classes lighter than FLT_EPSILON are skipped: 1 / 2^25 < 2^-23


def test_gray_is_opencv_fixed_point():
    px = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]]], np.uint8)
    assert R.gray(px).tolist() == [[255, 0, 29, 150, 76, 2]]


@pytest.mark.parametrize("W,H", [(40, 24), (24, 40), (30, 30)])
def test_box_arithmetic_at_the_clamps(W, H):
    S = min(W, H)
    corners = {"top-left": (0, 0), "top-right": (W - 3, 0), "bottom-left": (0, H - 2), "bottom-right": (W - 3, H - 2)}
    for name, (x, y) in corners.items():
        left, top = R.crop_origin(W, H, (x, y, 3, 2))
        assert 0 <= left <= W - S and 0 <= top <= H - S, name
        assert left == (0 if "left" in name else W - S) and top == (0 if "top" in name else H - S), name
    cx, cy = W // 2, H // 2                                         # a centred object: the square is centred on it where it has room
    left, top = R.crop_origin(W, H, (cx - 1, cy - 1, 3, 3))
    assert (left, top) == (max(0, min(cx - S // 2, W - S)), max(0, min(cy - S // 2, H - S)))
    assert R.crop_origin(W, H, None) == ((W - S) // 2, (H - S) // 2)
    if W == H:
        assert all(R.crop_origin(W, H, (x, y, 3, 2)) == (0, 0) for x, y in corners.values())


def test_boxes_of_a_whole_frame_and_the_tie_rule():
    m = np.zeros((20, 31), bool)
    m[3:9, 4:12] = True                                             # area 5 * 7
    m[12:18, 20:28] = True                                          # the same area, later in raster order: wins the tie
    row, lab = R.boxes_from_mask(m)
    assert row[:5] == [1, 20, 12, 8, 6] and row[5:] == list(R.crop_origin(31, 20, (20, 12, 8, 6)))
    m[3:9, 4:13] = True                                             # now larger: wins outright
    assert R.boxes_from_mask(m)[0][:5] == [1, 4, 3, 9, 6]
    dots = np.zeros((20, 31), bool)
    dots[2, 3] = dots[10, 29] = dots[15, 1] = True                  # zero areas all round: the last found
    assert R.boxes_from_mask(dots)[0][:5] == [1, 1, 15, 1, 1]
    assert R.boxes_from_mask(np.zeros((20, 31), bool))[0] == [0, 0, 0, 0, 0, 5, 0]
    out = R.object_boxes(R.frames_from_mask(m)[None])
    assert out["boxes"][0].tolist() == [1, 4, 3, 9, 6] + list(R.crop_origin(31, 20, (4, 3, 9, 6))) + [0]
    assert np.array_equal(out["mask"][0] > 0, m)


def test_batch_functions_exist_and_check_their_arguments_without_a_device():
    from data import common_methods as M
    for fn in (M.square_crop_batch, M.synthesize_pairs):
        with pytest.raises(NotImplementedError):
            fn(np.zeros((2, 32, 40, 3), np.float32))
        with pytest.raises(ValueError):
            fn(np.zeros((32, 40, 3), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((0, 32, 40, 3), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 32, 40, 4), np.uint8))
        with pytest.raises(ValueError):
            fn(np.zeros((2, 1, 40, 3), np.uint8))
    with pytest.raises(ValueError):
        M.synthesize_pairs(np.zeros((2, 24, 40, 3), np.uint8))      # the LR frames would fall below the degrade stages' 16 pixels
    assert "square_crop_batch" in M.__doc__


def test_binding_names_the_box_columns_as_the_header_does():
    import os
    import re
    from sr355 import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sr355.h")).read()
    cols = re.search(r"enum \{ (SR_BOX_FOUND = 0,[^}]*) \};", header).group(1).split(", ")
    assert cols[-1] == "SR_BOX_COLS" and len(cols) - 1 == len(_lib.BOX_NAMES) == 8
    assert _lib.BOX_NAMES == ("found", "x", "y", "w", "h", "left", "top", "otsu_t")
    assert len(_lib.SIGNATURES["sr_object_boxes"][1]) == 10 and len(_lib.SIGNATURES["sr_square_crop"][1]) == 8
