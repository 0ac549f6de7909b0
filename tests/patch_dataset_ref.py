"""Host references for the device patch datasets (sr355/patches.py, csrc/patch_dataset.hip): a NumPy restatement of sr_gather_patch_pairs,
index by index as the kernel computes it (no np.pad), and small PNG datasets for the loader to read."""
import os

import numpy as np
from PIL import Image

# LR (h, w), patch, stride, scale: every branch of the loader's window rules (see test_patch_dataset_cpu.py for what each one hits)
SCALE_CASES = (((30, 21), 8, 7, 2), ((20, 25), 8, 4, 2), ((19, 26), 8, 5, 4), ((17, 22), 6, 4, 3), ((239, 239), 24, 12, 2))


def reflect_br(i, n):
    """Index into an axis of n pixels of position i of its bottom / right reflect-padded extension: 2 (n - 1) - i for i >= n."""
    i = np.asarray(i)
    return np.where(i < n, i, 2 * (n - 1) - i)


def unit(stack):
    """A stack's values as the loader holds them: np.float32(u) / 255.0 for uint8, fp32 as it is."""
    return stack.astype(np.float32) / 255.0 if stack.dtype == np.uint8 else stack.astype(np.float32)


def gather_side(stack, table, rows, pad, patch, oscale, swap=False, mul=1.0, add=0.0):
    """Patches `rows` of `table` from one side's stack [N,H,W,3] -> fp32 [len(rows),patch,patch,3]."""
    N, H, W, _ = stack.shape
    assert 0 <= pad[0] <= H - 1 and 0 <= pad[1] <= W - 1
    out = np.empty((len(rows), patch, patch, 3), np.float32)
    src = unit(stack)
    for b, k in enumerate(rows):
        img, y0, x0 = (int(v) for v in table[k])
        y0, x0 = y0 * oscale, x0 * oscale
        assert 0 <= img < N and 0 <= y0 <= H + pad[0] - patch and 0 <= x0 <= W + pad[1] - patch
        ys, xs = reflect_br(y0 + np.arange(patch), H), reflect_br(x0 + np.arange(patch), W)
        out[b] = src[img][np.ix_(ys, xs)]
    if swap:
        out = out[..., ::-1]
    if mul != 1.0 or add != 0.0:
        out = out * np.float32(mul) + np.float32(add)
    return np.ascontiguousarray(out, np.float32)


def gather_pairs(ds, rows=None, mul=1.0, add=0.0):
    """The (X, Y) batch a PatchPairs whose stacks are still host arrays would cut for patches `rows` (all of them by default)."""
    s = ds._s
    rows = ds.rows(np.arange(len(ds)) if rows is None else rows)
    X = gather_side(np.asarray(s.lr), s.table, rows, s.lr_pad, s.patch_size, 1, s.swap[0], mul, add)
    Y = gather_side(np.asarray(s.hr), s.table, rows, s.hr_pad, s.patch_size * s.scale, s.scale, s.swap[1], mul, add)
    return X, Y


def write_pairs(root, n_images, lr_hw, scale, seed=0, same_size_lr=False):
    """n_images random RGB PNG pairs: <root>/hr/img_XX.png of size lr_hw * scale and <root>/lr/img_XX.png of size lr_hw (same_size_lr: the HR
    size).  -> (hr_root, lr_root, hr uint8 [N,H,W,3], lr uint8 [N,h,w,3])."""
    rng = np.random.default_rng(seed)
    h, w = lr_hw
    hr = rng.integers(0, 256, (n_images, h * scale, w * scale, 3), dtype=np.uint8)
    lr = rng.integers(0, 256, (n_images, h, w, 3), dtype=np.uint8)
    hr_root, lr_root = os.path.join(str(root), "hr"), os.path.join(str(root), "lr")
    os.makedirs(hr_root, exist_ok=True)
    os.makedirs(lr_root, exist_ok=True)
    for i in range(n_images):
        Image.fromarray(hr[i]).save(os.path.join(hr_root, f"img_{i:02d}.png"))
        Image.fromarray(lr[i]).save(os.path.join(lr_root, f"img_{i:02d}.png"))
    return hr_root, lr_root, hr, lr
