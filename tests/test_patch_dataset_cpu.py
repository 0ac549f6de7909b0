"""The device patch datasets' host side (sr355/patches.py), without a GPU: the window-table builder and a NumPy restatement of the gather
kernel (tests/patch_dataset_ref.py) against load_dataset_as_patches(mode="scale"), which is pure host code, on PNG sets written with PIL;
and the validation of subsets, sizes, pads, indices and views."""
import os

import numpy as np
import pytest
from PIL import Image

import patch_dataset_ref as R
from sr355.patches import PatchPairs, pad_amount, views_dataset, window_table
from SRModels.loading_methods import load_dataset_as_patches


def loader_windows(n_images, lr_hw, patch, stride, scale):
    """The loader's double loop restated on sizes alone: which (i, j) it appends, per image."""
    h, w = lr_hw
    hp, wp = h + pad_amount(h, patch, stride), w + pad_amount(w, patch, stride)
    Hp, Wp = h * scale + pad_amount(h * scale, patch * scale, stride), w * scale + pad_amount(w * scale, patch * scale, stride)
    rows = []
    for n in range(n_images):
        for i in range(0, hp - patch + 1, stride):
            for j in range(0, wp - patch + 1, stride):
                if min(Hp, i * scale + patch * scale) - i * scale == patch * scale and min(Wp, j * scale + patch * scale) - j * scale == patch * scale:
                    rows.append((n, i, j))
    return np.array(rows, np.int32).reshape(-1, 3)


# what each case is there for: windows the loader walks per image, how many of them the short-HR filter drops, whether a corner window reflects in both axes
EXPECT = {((30, 21), 8, 7, 2): (15, 3, None), ((20, 25), 8, 4, 2): (None, None, True), ((19, 26), 8, 5, 4): (None, None, True),
          ((17, 22), 6, 4, 3): (None, None, None), ((239, 239), 24, 12, 2): (361, 0, True)}          # the notebooks' geometry: 361 per image


@pytest.mark.parametrize("case", R.SCALE_CASES)
def test_table_and_patches_equal_the_loader(case, tmp_path):
    lr_hw, patch, stride, scale = case
    hr_root, lr_root, hr, lr = R.write_pairs(tmp_path, 3, lr_hw, scale, seed=sum(lr_hw))
    X, Y = load_dataset_as_patches(hr_root, lr_root, mode="scale", patch_size=patch, stride=stride, scale_factor=scale)
    ds = PatchPairs.from_dirs(hr_root, lr_root, "scale", patch, stride, scale)
    assert len(ds) == len(X) == len(Y) and ds.X.shape == X.shape and ds.Y.shape == Y.shape and ds.X.dtype == X.dtype
    assert np.array_equal(ds.windows, loader_windows(3, lr_hw, patch, stride, scale))
    gx, gy = R.gather_pairs(ds)
    assert gx.dtype == np.float32 and np.array_equal(gx.view(np.uint32), X.view(np.uint32))
    assert np.array_equal(gy.view(np.uint32), Y.view(np.uint32))
    per, dropped, corner = EXPECT[case]
    h, w = lr_hw
    hp, wp = h + pad_amount(h, patch, stride), w + pad_amount(w, patch, stride)
    walked = len(range(0, hp - patch + 1, stride)) * len(range(0, wp - patch + 1, stride))
    if per is not None:
        assert walked == per and len(ds) == 3 * (per - dropped)
    if corner:
        last = ds.windows[-1]
        assert last[1] + patch > h and last[2] + patch > w and (last[1] * scale + patch * scale > h * scale) and (last[2] * scale + patch * scale > w * scale)
    if case == ((20, 25), 8, 4, 2):
        assert h % stride == 0 and pad_amount(h, patch, stride) == patch - stride          # the n % stride == 0 branch


def test_notebook_geometry_gives_361_windows_per_image():
    table, lr_pad, hr_pad, s = window_table(2, (239, 239), (478, 478), "scale", 24, 12, 2)
    assert len(table) == 2 * 361 and s == 2
    assert np.array_equal(table, loader_windows(2, (239, 239), 24, 12, 2))
    assert lr_pad == (pad_amount(239, 24, 12),) * 2 and hr_pad == (pad_amount(478, 48, 12),) * 2


def test_srcnn_table_walks_the_padded_extents():
    table, lr_pad, hr_pad, s = window_table(1, (46, 58), (46, 58), "srcnn", 11, 5)
    assert s == 1 and lr_pad == hr_pad and len(table) == 99
    Hp, Wp = 46 + lr_pad[0], 58 + lr_pad[1]
    assert table[-1, 1] + 11 > 46 and table[-1, 2] + 11 > 58 and table[-1, 1] + 11 <= Hp and table[-1, 2] + 11 <= Wp


def small_ds(n=2):
    rng = np.random.default_rng(5)
    lr = rng.integers(0, 256, (n, 17, 22, 3), dtype=np.uint8)
    hr = rng.integers(0, 256, (n, 51, 66, 3), dtype=np.uint8)
    return PatchPairs.from_stacks(lr, hr, "scale", 6, 4, 3)


def test_subset_composes_and_shares_the_stacks():
    ds = small_ds()
    n = len(ds)
    a = np.random.default_rng(0).permutation(n)[: n // 2]
    sub = ds.subset(a)
    b = np.array([3, 0, len(a) - 1, 3])
    subsub = sub.subset(b)
    assert sub._s is ds._s and subsub._s is ds._s
    assert np.array_equal(subsub.windows, ds.windows[a[b]]) and len(subsub) == 4 and subsub.X.shape[0] == 4
    full = R.gather_pairs(ds)
    got = R.gather_pairs(subsub)
    assert np.array_equal(got[0], full[0][a[b]]) and np.array_equal(got[1], full[1][a[b]])
    assert np.array_equal(R.gather_pairs(sub, rows=b)[1], full[1][a[b]])


def test_scaling_is_the_loaders_value_times_two_minus_one():
    ds = small_ds()
    X, Y = R.gather_pairs(ds)
    x2, y2 = R.gather_pairs(ds, mul=2.0, add=-1.0)
    assert np.array_equal(x2, X * np.float32(2.0) - np.float32(1.0)) and np.array_equal(y2, Y * 2.0 - 1.0)


def test_uint8_quotient_is_not_the_reciprocal_product():
    u = np.arange(256, dtype=np.uint8)
    q = R.unit(u)
    assert np.array_equal(q, np.arange(256, dtype=np.float32) / np.float32(255.0))
    assert int(np.sum(q != np.arange(256, dtype=np.float32) * (np.float32(1.0) / np.float32(255.0)))) == 126


def test_mixed_sizes_name_the_first_file_that_differs(tmp_path):
    hr_root, lr_root, hr, lr = R.write_pairs(tmp_path, 3, (17, 22), 3)
    Image.fromarray(lr[1][:-1]).save(os.path.join(lr_root, "img_01.png"))
    with pytest.raises(ValueError, match="img_01.png"):
        PatchPairs.from_dirs(hr_root, lr_root, "scale", 6, 4, 3)


def test_a_pad_beyond_size_minus_one_is_refused():
    with pytest.raises(ValueError, match="reflect padding"):
        window_table(1, (5, 40), (10, 80), "scale", 12, 4, 2)          # pad 8 on 5 rows: np.pad would reflect twice
    rng = np.random.default_rng(1)
    with pytest.raises(ValueError, match="reflect padding"):
        PatchPairs.from_stacks(rng.integers(0, 255, (1, 5, 40, 3), dtype=np.uint8), rng.integers(0, 255, (1, 10, 80, 3), dtype=np.uint8), "scale", 12, 4, 2)


def test_out_of_range_indices_are_refused_on_the_host():
    ds = small_ds()
    n = len(ds)
    for bad in ([0, n], [-1], np.array([n + 5])):
        with pytest.raises(ValueError, match="indices must lie"):
            ds.subset(bad)
        with pytest.raises(ValueError, match="indices must lie"):
            ds.rows(bad)                                                    # what set_order validates before it uploads
    with pytest.raises(ValueError):
        ds.subset(np.array([0.5, 1.0]))
    with pytest.raises(ValueError, match="indices must lie"):
        ds.subset([0, 1]).subset([2])


def test_mixed_views_are_refused():
    ds, other = small_ds(), small_ds()
    arr = np.zeros((len(ds), 6, 6, 3), np.float32)
    assert views_dataset(ds.X, ds.Y) is ds and views_dataset(arr, arr) is None
    for X, Y in ((ds.X, arr), (arr, ds.Y), (ds.X, other.Y), (ds.subset([0, 1]).X, ds.Y), (ds.Y, ds.X)):
        with pytest.raises(ValueError):
            views_dataset(X, Y)
