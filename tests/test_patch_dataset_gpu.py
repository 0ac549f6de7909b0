"""sr_gather_patch_pairs and sr355.patches.PatchPairs on the device against load_dataset_as_patches: every batch bit for bit the loader's
X[idx], Y[idx], at the window-rule cases of tests/patch_dataset_ref.py (odd sizes, corner windows reflecting in both axes, scales 2 / 3 / 4),
in a shuffled order, with batch sizes that end in a partial batch."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

import patch_dataset_ref as R
from sr355.patches import PatchPairs
from SRModels.loading_methods import load_dataset_as_patches

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_batches_equal(ds, X, Y, B, seed, mul=1.0, add=0.0):
    """Every patch of ds, in a shuffled order, in batches of B (the last one partial), equals the arrays' rows bit for bit."""
    n = len(ds)
    assert n == len(X) == len(Y) and n % B != 0
    perm = np.random.default_rng(seed).permutation(n)
    order = ds.set_order(perm)
    for i in range(0, n, B):
        k = min(B, n - i)
        x, y = ds.batch(order, i, k, mul, add)
        idx = perm[i:i + k]
        ex, ey = (X[idx], Y[idx]) if mul == 1.0 and add == 0.0 else (X[idx] * np.float32(mul) + np.float32(add), Y[idx] * np.float32(mul) + np.float32(add))
        assert x.shape == ex.shape and y.shape == ey.shape and x.dtype == torch.float32
        assert np.array_equal(bits(x.cpu().numpy()), bits(ex)), (i, "X")
        assert np.array_equal(bits(y.cpu().numpy()), bits(ey)), (i, "Y")
    assert n - 1 in perm and len(ds.windows) - 1 == int(np.argmax(ds.windows[:, 0] * 10 ** 6 + ds.windows[:, 1] * 10 ** 3 + ds.windows[:, 2]))   # last image's corner window is in


@pytest.mark.parametrize("case", R.SCALE_CASES)
def test_scale_mode_batches_are_the_loaders(ctx, case, tmp_path):
    lr_hw, patch, stride, scale = case
    n_img = 4 if scale == 2 else 3
    hr_root, lr_root, _, _ = R.write_pairs(tmp_path, n_img, lr_hw, scale, seed=sum(lr_hw))
    X, Y = load_dataset_as_patches(hr_root, lr_root, mode="scale", patch_size=patch, stride=stride, scale_factor=scale)
    ds = PatchPairs.from_dirs(hr_root, lr_root, "scale", patch, stride, scale)
    B = 7 if len(X) % 7 else 5
    assert_batches_equal(ds, X, Y, B, seed=3)
    # the loader's own switch returns views of one such dataset; .numpy() is the whole array
    Xd, Yd = load_dataset_as_patches(hr_root, lr_root, mode="scale", patch_size=patch, stride=stride, scale_factor=scale, on_device=True)
    assert Xd.ds is Yd.ds and Xd.shape == X.shape and Yd.shape == Y.shape
    assert np.array_equal(bits(Xd.numpy(chunk=11)), bits(X)) and np.array_equal(bits(Yd.numpy(chunk=11)), bits(Y))
    # a subset batches its own patches
    sub = ds.subset(np.arange(len(ds))[::3])
    x, y = sub.batch(sub.set_order(np.arange(len(sub))), 1, len(sub) - 1)
    assert np.array_equal(bits(x.cpu().numpy()), bits(X[::3][1:])) and np.array_equal(bits(y.cpu().numpy()), bits(Y[::3][1:]))


@pytest.mark.parametrize("hw,patch,stride,expect", [((46, 58), 11, 5, 99), ((40, 52), 11, 4, None)])
def test_srcnn_mode_batches_are_the_loaders(ctx, hw, patch, stride, expect, tmp_path):
    """LR images of half the size, resized by the loader's own kernel with a per-file interpolation code; five files: LINEAR, CUBIC, AREA,
    LANCZOS4 and one the map does not name (INTER_CUBIC)."""
    rng = np.random.default_rng(hw[0])
    hr_root, lr_root = str(tmp_path / "hr"), str(tmp_path / "lr")
    os.makedirs(hr_root), os.makedirs(lr_root)
    names = [f"f{i}.png" for i in range(5)]
    for f in names:
        Image.fromarray(rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)).save(os.path.join(hr_root, f))
        Image.fromarray(rng.integers(0, 256, (hw[0] // 2, hw[1] // 2, 3), dtype=np.uint8)).save(os.path.join(lr_root, f))
    imap = str(tmp_path / "interpolation_map.pkl")
    with open(imap, "wb") as fh:
        pickle.dump({"f0.png": "INTER_LINEAR", "f1.png": "INTER_CUBIC", "f2.png": "INTER_AREA", "f3.png": "INTER_LANCZOS4"}, fh)
    X, Y, hr_h, hr_w = load_dataset_as_patches(hr_root, lr_root, mode="srcnn", patch_size=patch, stride=stride, interpolation_map_path=imap)
    Xd, Yd, dh, dw = load_dataset_as_patches(hr_root, lr_root, mode="srcnn", patch_size=patch, stride=stride, interpolation_map_path=imap, on_device=True)
    assert (dh, dw) == (hr_h, hr_w) == hw and Xd.ds is Yd.ds
    ds = Xd.ds
    if expect is not None:
        assert len(ds) == 5 * expect
    last = ds.windows[-1]
    assert last[1] + patch > hw[0] and last[2] + patch > hw[1]                       # a corner window reflecting in both axes
    assert_batches_equal(ds, X, Y, 13 if len(X) % 13 else 11, seed=8)


def test_from_device_bgr_stacks_equal_from_dirs_and_scale_exactly(ctx, tmp_path):
    """uint8 BGR stacks as synthesize_pairs leaves them on the device against PNGs written from the same pixels; mul / add give x * 2 - 1."""
    lr_hw, patch, stride, scale = (20, 25), 8, 4, 2
    hr_root, lr_root, hr_rgb, lr_rgb = R.write_pairs(tmp_path, 3, lr_hw, scale, seed=77)
    X, Y = load_dataset_as_patches(hr_root, lr_root, mode="scale", patch_size=patch, stride=stride, scale_factor=scale)
    hr_bgr, lr_bgr = ctx.to_device(np.ascontiguousarray(hr_rgb[..., ::-1])), ctx.to_device(np.ascontiguousarray(lr_rgb[..., ::-1]))
    ds = PatchPairs.from_device(hr_bgr, lr_bgr, channel_order="bgr", mode="scale", patch_size=patch, stride=stride, scale_factor=scale)
    assert_batches_equal(ds, X, Y, 9 if len(X) % 9 else 7, seed=1)
    assert_batches_equal(ds, X, Y, 9 if len(X) % 9 else 7, seed=2, mul=2.0, add=-1.0)
    # srcnn mode from the device: the LR stack resized by name, against the loader reading a map with the same names
    lr_root2 = str(tmp_path / "lr_same")
    os.makedirs(lr_root2)
    small = np.random.default_rng(4).integers(0, 256, (3, 20, 25, 3), dtype=np.uint8)
    for i in range(3):
        Image.fromarray(small[i]).save(os.path.join(lr_root2, f"img_{i:02d}.png"))
    names = ["INTER_AREA", "INTER_LINEAR", "INTER_CUBIC"]
    imap = str(tmp_path / "map.pkl")
    with open(imap, "wb") as fh:
        pickle.dump({f"img_{i:02d}.png": m for i, m in enumerate(names)}, fh)
    Xs, Ys, _, _ = load_dataset_as_patches(hr_root, lr_root2, mode="srcnn", patch_size=11, stride=5, interpolation_map_path=imap)
    ds2 = PatchPairs.from_device(hr_bgr, ctx.to_device(np.ascontiguousarray(small[..., ::-1])), names, "bgr", mode="srcnn", patch_size=11, stride=5)
    assert_batches_equal(ds2, Xs, Ys, 13 if len(Xs) % 13 else 11, seed=5)


def test_all_256_codes_through_the_whole_image_mode(ctx):
    u = np.arange(256, dtype=np.uint8)
    stack = np.stack([np.tile(u, 3).reshape(16, 16, 3), np.tile(u[::-1], 3).reshape(16, 16, 3)])
    got = ctx.u8_to_unit(ctx.to_device(stack)).cpu().numpy()
    assert got.shape == stack.shape and np.array_equal(bits(got), bits(stack.astype(np.float32) / 255.0))
    assert np.array_equal(bits(ctx.u8_to_unit(ctx.to_device(stack), swap=True).cpu().numpy()), bits(stack[..., ::-1].astype(np.float32) / 255.0))
    # a non-square whole-image window
    wide = np.random.default_rng(0).integers(0, 256, (3, 5, 37, 3), dtype=np.uint8)
    assert np.array_equal(bits(ctx.u8_to_unit(ctx.to_device(wide)).cpu().numpy()), bits(wide.astype(np.float32) / 255.0))


def test_bad_arguments_are_refused_before_any_launch(ctx):
    lr = ctx.to_device(np.zeros((1, 5, 40, 3), np.uint8))
    win, order = ctx.to_device(np.zeros((1, 3), np.int32)), ctx.to_device(np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="padding"):
        ctx.gather_patch_pairs(dict(stack=lr, pad=(5, 0)), None, win, order, 0, 1, 4)
    with pytest.raises(ValueError, match="does not fit"):
        ctx.gather_patch_pairs(dict(stack=lr, pad=(0, 0)), None, win, order, 0, 1, 6)
    with pytest.raises(ValueError, match="order"):
        ctx.gather_patch_pairs(dict(stack=lr), None, win, order, 2, 3, 4)
    # the ABI's own checks (the wrapper lets these through): an uneven pair of stacks, a mul that is not finite
    side = dict(stack=lr, mul=float("inf"))
    with pytest.raises(ValueError, match="finite"):
        ctx.gather_patch_pairs(side, None, win, order, 0, 1, 4)
