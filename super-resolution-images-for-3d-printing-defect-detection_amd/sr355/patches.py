"""Patch datasets that stay on the device (reference: SRModels/loading_methods.py:40-191, load_dataset_as_patches).

The loader returns two dense fp32 arrays holding every sliding window of every image; neighbouring windows overlap, so each pixel is stored
several times over, on the host, and every training step indexes the arrays and uploads a batch.  A `PatchPairs` keeps the DISTINCT pixels on
the device once -- two image stacks, uint8 as decoded (or the fp32 result of the `srcnn` mode's resize) -- with a host-built table of window
origins, and `batch()` cuts a batch of LR / HR patches from them by one launch (sr_gather_patch_pairs, csrc/patch_dataset.hip).  Patch k of
the dataset is patch k of the loader's arrays, bit for bit: the kernel applies the loader's reflect padding, channel order and
float(u) / 255 division per element.

Window rules (`window_table`), copied from the loader with its quirks:
  * add_padding pads bottom / right by max((patch - n % stride) % stride if n % stride else 0, patch - stride), reflecting without the edge;
  * `scale` mode pads the HR image for patch * scale but with the LR stride, walks the padded LR extents and drops every window whose HR
    slice would come out short;
  * `srcnn` mode pads both (equal-size) sides alike and walks the padded extents.
Everything in this module up to the first `batch()` / `.numpy()` runs without a GPU (scale mode: the stacks are uploaded on first use).

`LabeledPatches` is the classifier's counterpart (reference: loading_methods.py:194-285, load_defects_dataset_as_patches): one frame stack, the
loader's windows over the UNPADDED extents (`window_table_defects`: that loader pads but never walks the padding, so the dataset needs none),
one class id per frame.  `batch()` cuts the loader's patches and `warped_batch()` the augmented ones FineTunedVGG16.fit trains on
(sr_gather_warp_patches), so the fit holds the distinct pixels once, as uint8, instead of every overlapping window in fp32.
"""
import os
import pickle

import numpy as np

MODES = ("srcnn", "scale")


def pad_amount(n, patch, stride):
    """add_padding's bottom / right pad of an axis of n pixels (loading_methods.py:6-26)."""
    pad = (patch - (n % stride)) % stride if n % stride != 0 else 0
    return max(pad, patch - stride)


def window_table(n_images, lr_hw, hr_hw, mode, patch_size, stride, scale_factor=2):
    """The loader's windows for `n_images` images of LR-side size lr_hw and HR-side size hr_hw, in the loader's order (image by image,
    rows then columns).  -> (int32 [n,3] rows (image, y, x) in LR-side pixels, (pad_h, pad_w) of the LR side, (pad_h, pad_w) of the HR side,
    scale).  Pure host code.  ValueError where a pad exceeds size - 1: np.pad would reflect more than once there, the kernel does not."""
    if mode not in MODES:
        raise ValueError("mode must be 'srcnn' or 'scale'")
    for v, name in ((patch_size, "patch_size"), (stride, "stride")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
            raise ValueError(f"{name} must be positive int.")
    (h, w), (H, W) = (int(v) for v in lr_hw), (int(v) for v in hr_hw)
    if mode == "scale":
        if not isinstance(scale_factor, (int, np.integer)) or isinstance(scale_factor, bool) or scale_factor <= 0:
            raise ValueError("scale_factor must be positive int.")
        s = int(scale_factor)
    else:
        s = 1
        if (h, w) != (H, W):
            raise ValueError("srcnn mode: both sides have the HR size")
    P = patch_size * s
    lr_pad = (pad_amount(h, patch_size, stride), pad_amount(w, patch_size, stride))
    hr_pad = (pad_amount(H, P, stride), pad_amount(W, P, stride))          # scale mode: the LR stride on purpose (reference quirk)
    for (n, p), what in (((h, lr_pad[0]), "LR height"), ((w, lr_pad[1]), "LR width"), ((H, hr_pad[0]), "HR height"), ((W, hr_pad[1]), "HR width")):
        if p > n - 1:
            raise ValueError(f"reflect padding of {p} exceeds {what} {n} - 1 (patch {patch_size}, stride {stride}): image too small for this patch")
    hp, wp, Hp, Wp = h + lr_pad[0], w + lr_pad[1], H + hr_pad[0], W + hr_pad[1]
    ys = [i for i in range(0, hp - patch_size + 1, stride) if i * s + P <= Hp]      # a short HR slice drops the window
    xs = [j for j in range(0, wp - patch_size + 1, stride) if j * s + P <= Wp]
    per = np.array([(i, j) for i in ys for j in xs], np.int32).reshape(-1, 2)
    table = np.zeros((n_images * len(per), 3), np.int32)
    if len(per):
        table[:, 0] = np.repeat(np.arange(n_images, dtype=np.int32), len(per))
        table[:, 1:] = np.tile(per, (n_images, 1))
    return table, lr_pad, hr_pad, s


def _check_indices(idx, n, what):
    idx = np.asarray(idx)
    if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"{what}: a 1-D integer array")
    if len(idx) and (idx.min() < 0 or idx.max() >= n):
        raise ValueError(f"{what}: indices must lie in [0, {n})")
    return idx.astype(np.int64)


class _Store:
    """What every subset of one dataset shares: the two stacks (host arrays until their first device use, device tensors after), the full
    window table, the pads, the mode and the scale."""

    def __init__(self, lr, hr, table, lr_pad, hr_pad, mode, scale, patch_size, swap, ctx=None):
        self.lr, self.hr, self.table, self.lr_pad, self.hr_pad = lr, hr, table, tuple(lr_pad), tuple(hr_pad)
        self.mode, self.scale, self.patch_size, self.ctx = mode, int(scale), int(patch_size), ctx
        self.swap = tuple(bool(v) for v in swap) if isinstance(swap, tuple) else (bool(swap), bool(swap))       # (LR side, HR side)
        self.table_dev = None

    def on_device(self):
        """Uploads what is still on the host: one copy per side and the table."""
        import torch
        from . import Context
        if self.ctx is None:
            self.ctx = Context.get()
        if not isinstance(self.lr, torch.Tensor):
            self.lr = self.ctx.to_device(self.lr)
        if not isinstance(self.hr, torch.Tensor):
            self.hr = self.ctx.to_device(self.hr)
        if self.table_dev is None:
            self.table_dev = self.ctx.to_device(self.table)
        return self


class PatchView:
    """`ds.X` / `ds.Y`: what the loader's X / Y array is to a caller that only passes it on -- shape, dtype, len -- and `.numpy()` for the
    values (gathered on the device in chunks).  The fits recognise a pair of views of one dataset and batch from it directly."""
    dtype = np.dtype(np.float32)

    def __init__(self, ds, side):
        self.ds, self.side = ds, side

    def __len__(self):
        return len(self.ds)

    @property
    def shape(self):
        p = self.ds.patch_size * (self.ds.scale if self.side == "Y" else 1)
        return (len(self.ds), p, p, 3)

    @property
    def ndim(self):
        return 4

    def numpy(self, chunk=4096):
        ds = self.ds
        out = np.empty(self.shape, np.float32)
        if len(ds):
            order = ds.set_order(np.arange(len(ds)))
            for i in range(0, len(ds), chunk):
                k = min(chunk, len(ds) - i)
                out[i:i + k] = ds.batch(order, i, k)[0 if self.side == "X" else 1].cpu().numpy()
        return out

    def __repr__(self):
        return f"<PatchView {self.side} {self.shape} float32 of {self.ds!r}>"


def views_dataset(X, Y, what="(X, Y)"):
    """A fit's (X, Y) arguments -> the PatchPairs both are views of, or None when both are plain arrays.  ValueError for a view mixed with
    an array, views of different datasets, or the two sides crossed."""
    vx, vy = isinstance(X, PatchView), isinstance(Y, PatchView)
    if not vx and not vy:
        return None
    if vx != vy:
        raise ValueError(f"{what}: a PatchPairs view cannot be mixed with an array; pass ds.X and ds.Y of one dataset")
    if X.ds is not Y.ds:
        raise ValueError(f"{what}: X and Y are views of different datasets; pass ds.X and ds.Y of one dataset")
    if X.side != "X" or Y.side != "Y":
        raise ValueError(f"{what}: expected (ds.X, ds.Y)")
    return X.ds


class PatchPairs:
    """Aligned LR / HR training patches cut on demand from two device-resident image stacks.

    All images of a side must share one size (the reference's dataset is uniform: 478 x 478 HR crops and their 239 x 239 LR frames); a
    directory that mixes sizes raises ValueError naming the first file that differs.  `len(ds)` patches; `ds.X` / `ds.Y` stand in for the
    loader's arrays; `ds.subset(indices)` is the dataset of those patches, sharing the stacks (so train_test_split over
    np.arange(len(ds)) applies directly); `ds.set_order(permutation)` uploads an epoch's order once and `ds.batch(order, offset, B)` cuts
    patches order[offset : offset + B] by one launch."""

    def __init__(self, store, index=None):
        self._s = store
        self.index = None if index is None else _check_indices(index, len(store.table), "PatchPairs index")
        self.X, self.Y = PatchView(self, "X"), PatchView(self, "Y")

    # ---- constructors
    @classmethod
    def from_stacks(cls, lr, hr, mode="scale", patch_size=24, stride=12, scale_factor=2, swap_rb=False, ctx=None):
        """lr [N,h,w,3] / hr [N,H,W,3]: uint8 or fp32 [0,1] stacks, NumPy (uploaded on first use) or device tensors, channels in the order
        the patches should have unless swap_rb (a bool, or one per side: (LR, HR))."""
        for a, who in ((lr, "LR"), (hr, "HR")):
            if len(a.shape) != 4 or a.shape[3] != 3 or a.shape[0] < 1:
                raise ValueError(f"{who} stack must be [N,H,W,3] with N >= 1")
            if str(a.dtype).replace("torch.", "") not in ("uint8", "float32"):
                raise ValueError(f"{who} stack must be uint8 or float32")
        if lr.shape[0] != hr.shape[0]:
            raise ValueError("the two stacks hold different numbers of images")
        table, lr_pad, hr_pad, s = window_table(int(lr.shape[0]), lr.shape[1:3], hr.shape[1:3], mode, patch_size, stride, scale_factor)
        return cls(_Store(lr, hr, table, lr_pad, hr_pad, mode, s, patch_size, swap_rb, ctx))

    @classmethod
    def from_dirs(cls, hr_root, lr_root, mode="srcnn", patch_size=33, stride=14, scale_factor=2, interpolation_map_path=None):
        """The dataset load_dataset_as_patches(...) returns for the same arguments: the same validation, file matching and sort, PIL decode
        to uint8, one upload per side.  `srcnn` mode stores the LR side as the clipped fp32 result of the loader's ctx.resize calls (per-file
        interpolation code from the map, INTER_CUBIC by default)."""
        from SRModels import loading_methods as LM
        from PIL import Image
        if mode not in MODES:
            raise ValueError("mode must be 'srcnn' or 'scale'")
        LM._check_dirs(hr_root, lr_root)
        if not isinstance(patch_size, int) or patch_size <= 0:
            raise ValueError("patch_size must be positive int.")
        if not isinstance(stride, int) or stride <= 0:
            raise ValueError("stride must be positive int.")
        if mode == "scale" and (not isinstance(scale_factor, int) or scale_factor <= 0):
            raise ValueError("scale_factor must be positive int.")
        hr_paths, lr_paths = LM.get_all_image_paths(hr_root), LM.get_all_image_paths(lr_root)
        if not hr_paths or not lr_paths:
            raise ValueError("No images found in provided directories.")
        hr_by, lr_by = {os.path.basename(p): p for p in hr_paths}, {os.path.basename(p): p for p in lr_paths}
        names = sorted(set(hr_by) & set(lr_by))
        if not names:
            raise ValueError("No matching basenames found between LR and HR roots.")

        def stack(by, who):
            imgs = []
            for f in names:
                with Image.open(by[f]) as im:
                    a = np.asarray(im.convert("RGB"), dtype=np.uint8)
                if imgs and a.shape != imgs[0].shape:
                    raise ValueError(f"{who} image {by[f]} is {a.shape[0]} x {a.shape[1]}, the first ({by[names[0]]}) is "
                                     f"{imgs[0].shape[0]} x {imgs[0].shape[1]}: a PatchPairs needs one size per side")
                imgs.append(a)
            return np.stack(imgs)

        hr, lr = stack(hr_by, "HR"), stack(lr_by, "LR")
        if mode == "scale":
            return cls.from_stacks(lr, hr, "scale", patch_size, stride, scale_factor)
        interp = None
        if interpolation_map_path is not None:
            with open(interpolation_map_path, "rb") as f:
                interp = pickle.load(f)
        codes = []
        for f in names:
            method = interp.get(f, 2) if interp is not None else 2
            codes.append(LM._INTERP_CODES.get(method, 2) if isinstance(method, str) else int(method) if isinstance(method, (int, np.integer)) else 2)
        window_table(len(names), hr.shape[1:3], hr.shape[1:3], "srcnn", patch_size, stride)      # refuse a bad geometry before any upload
        from . import Context
        ctx = Context.get()
        return cls.from_stacks(_resized_unit(ctx, ctx.to_device(lr), hr.shape[1], hr.shape[2], codes, False), hr, "srcnn", patch_size, stride, ctx=ctx)

    @classmethod
    def from_device(cls, hr_u8, lr_u8, interpolation_names=None, channel_order="bgr", mode="scale", patch_size=24, stride=12, scale_factor=2):
        """The output of data.common_methods.synthesize_pairs -- uint8 device stacks hr [N,S,S,3], lr [N,h,w,3] and the per-image interpolation
        names -- as a dataset, without a PNG in between.  channel_order "bgr" (synthesis) is swapped to the loader's RGB in the gather.
        `srcnn` mode resizes each LR image with its interpolation name (INTER_CUBIC without names), as the loader does with its map."""
        if channel_order not in ("bgr", "rgb"):
            raise ValueError("channel_order must be 'bgr' or 'rgb'")
        swap = channel_order == "bgr"
        if mode == "scale":
            return cls.from_stacks(lr_u8, hr_u8, "scale", patch_size, stride, scale_factor, swap_rb=swap)
        from . import Context
        ctx = Context.get()
        n = int(lr_u8.shape[0])
        names = list(interpolation_names) if interpolation_names is not None else ["INTER_CUBIC"] * n
        if len(names) != n:
            raise ValueError("interpolation_names: one name per image")
        from SRModels.loading_methods import _INTERP_CODES
        codes = [_INTERP_CODES.get(m, 2) if isinstance(m, str) else int(m) for m in names]
        window_table(n, hr_u8.shape[1:3], hr_u8.shape[1:3], "srcnn", patch_size, stride)
        lr_up = _resized_unit(ctx, ctx.to_device(lr_u8), int(hr_u8.shape[1]), int(hr_u8.shape[2]), codes, swap)
        return cls.from_stacks(lr_up, hr_u8, "srcnn", patch_size, stride, swap_rb=(False, swap), ctx=ctx)      # the resized side is RGB already

    # ---- the loader's surface
    def __len__(self):
        return len(self._s.table) if self.index is None else len(self.index)

    def __repr__(self):
        return f"PatchPairs({len(self)} patches, mode={self._s.mode!r}, patch={self._s.patch_size}, scale={self._s.scale})"

    patch_size = property(lambda self: self._s.patch_size)
    scale = property(lambda self: self._s.scale)
    mode = property(lambda self: self._s.mode)
    hr_size = property(lambda self: (int(self._s.hr.shape[1]), int(self._s.hr.shape[2])))

    @property
    def windows(self):
        """int32 [len,3]: (image, y, x) of this dataset's patches."""
        return self._s.table if self.index is None else self._s.table[self.index]

    def rows(self, indices):
        """Patch numbers of THIS dataset -> rows of the shared window table."""
        idx = _check_indices(indices, len(self), "patch indices")
        return idx if self.index is None else self.index[idx]

    def subset(self, indices):
        """The dataset of patches `indices` (in that order), sharing the stacks and the table."""
        return PatchPairs(self._s, self.rows(indices))

    def host_bytes(self):
        """Bytes this dataset holds on the host (the window table, the subset's index, and the stacks while they are not uploaded)."""
        n = self._s.table.nbytes + (0 if self.index is None else self.index.nbytes)
        return n + sum(a.nbytes for a in (self._s.lr, self._s.hr) if isinstance(a, np.ndarray))

    # ---- batches
    def set_order(self, host_permutation):
        """An order over this dataset's patches (an epoch's permutation), validated on the host -> int32 device tensor of table rows."""
        s = self._s.on_device()
        return s.ctx.to_device(self.rows(host_permutation).astype(np.int32))

    def batch(self, order_dev, offset, B, mul=1.0, add=0.0):
        """Patches order_dev[offset : offset + B] (order_dev from set_order) -> (X [B,p,p,3], Y [B,p*scale,p*scale,3]) fp32 device tensors,
        each value v * mul + add of the loader's value v."""
        s = self._s.on_device()
        lr = dict(stack=s.lr, pad=s.lr_pad, swap=s.swap[0], mul=mul, add=add)
        hr = dict(stack=s.hr, pad=s.hr_pad, swap=s.swap[1], mul=mul, add=add)
        return s.ctx.gather_patch_pairs(lr, hr, s.table_dev, order_dev, offset, B, s.patch_size, s.scale)


# ---------------------------------------------------------------------------------------------------------------- the classifier's dataset
def window_table_defects(n_images, hw, patch_size, stride):
    """load_defects_dataset_as_patches' windows (loading_methods.py:194-285) for n_images frames of size hw: range(0, n - patch + 1, stride)
    over the UNPADDED extents (the loader pads and then walks the unpadded size, so no window touches the padding), image by image, rows
    then columns -> int32 [n,3] rows (image, y, x).  Pure host code.  ValueError where the patch exceeds the frame: no windows."""
    for v, name in ((patch_size, "patch_size"), (stride, "stride")):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v <= 0:
            raise ValueError(f"{name} must be positive int.")
    h, w = (int(v) for v in hw)
    if patch_size > h or patch_size > w:
        raise ValueError(f"a {patch_size} x {patch_size} patch exceeds the {h} x {w} frame: the dataset would hold no windows")
    per = np.array([(i, j) for i in range(0, h - patch_size + 1, stride) for j in range(0, w - patch_size + 1, stride)], np.int32).reshape(-1, 2)
    table = np.zeros((int(n_images) * len(per), 3), np.int32)
    table[:, 0] = np.repeat(np.arange(int(n_images), dtype=np.int32), len(per))
    table[:, 1:] = np.tile(per, (int(n_images), 1))
    return table


class _LabeledStore:
    """What every subset of one LabeledPatches shares: the frame stack (a host array until its first device use), the full window table and
    the label of every window."""

    def __init__(self, frames, table, labels, patch_size, swap, ctx=None):
        self.frames, self.table, self.labels, self.patch_size, self.swap, self.ctx = frames, table, labels, int(patch_size), bool(swap), ctx
        self.table_dev = None

    def on_device(self):
        """Uploads what is still on the host: the stack, once, and the table."""
        import torch
        from . import Context
        if self.ctx is None:
            self.ctx = Context.get()
        if not isinstance(self.frames, torch.Tensor):
            self.frames = self.ctx.to_device(self.frames)
        if self.table_dev is None:
            self.table_dev = self.ctx.to_device(self.table)
        return self


class LabeledView:
    """`ds.X`: what load_defects_dataset_as_patches' X array is to a caller that passes it on or splits it -- shape, dtype, ndim, len, and
    X[idx] for a 1-D integer array or a slice (the view of ds.subset(idx), so sklearn's train_test_split(X, y) works on it as on the array) --
    and `.numpy()` for the values.  FineTunedVGG16.fit / evaluate / predict recognise it and batch from the dataset directly."""
    dtype = np.dtype(np.float32)

    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    @property
    def shape(self):
        return (len(self.ds), self.ds.patch_size, self.ds.patch_size, 3)

    @property
    def ndim(self):
        return 4

    def __getitem__(self, idx):
        if isinstance(idx, tuple):          # X[idx, ...] / X[idx, :]: scikit-learn indexes the first axis this way
            if not idx or any(not (k is Ellipsis or (isinstance(k, slice) and k == slice(None))) for k in idx[1:]):
                raise ValueError("a patch view is indexed along its first axis only")
            idx = idx[0]
        if isinstance(idx, slice):
            idx = np.arange(len(self.ds))[idx]
        return self.ds.subset(idx).X

    def numpy(self, chunk=4096):
        ds = self.ds
        out = np.empty(self.shape, np.float32)
        if len(ds):
            order = ds.set_order(np.arange(len(ds)))
            for i in range(0, len(ds), chunk):
                k = min(chunk, len(ds) - i)
                out[i:i + k] = ds.batch(order, i, k).cpu().numpy()
        return out

    def __repr__(self):
        return f"<LabeledView {self.shape} float32 of {self.ds!r}>"


def labeled_dataset(X):
    """An image argument of FineTunedVGG16.fit / evaluate / predict -> the LabeledPatches it is a view of, or None for an array."""
    return X.ds if isinstance(X, LabeledView) else None


class LabeledPatches:
    """The classifier's training patches with the class id of their frame, cut on demand from ONE device-resident frame stack: the device
    form of load_defects_dataset_as_patches' (X, y).  All frames share one size (the reference's dataset is uniform: 478 x 478 crops); a
    directory that mixes sizes raises ValueError naming the first file that differs.  `len(ds)` patches; `ds.X` stands in for the loader's X
    and `ds.y` IS the loader's y (int64, host); `ds.subset(indices)` shares the stack; `ds.set_order(permutation)` uploads an epoch's order,
    `ds.batch(order, offset, B)` cuts the plain patches (sr_gather_patch_pairs, one-sided) and `ds.warped_batch(order, offset, B, params)`
    the augmented ones (sr_gather_warp_patches), each by one launch."""

    def __init__(self, store, index=None):
        self._s = store
        self.index = None if index is None else _check_indices(index, len(store.table), "LabeledPatches index")
        self.X = LabeledView(self)

    # ---- constructors
    @classmethod
    def from_stacks(cls, frames, labels, patch_size, stride, swap_rb=False, ctx=None):
        """frames [N,H,W,3]: a uint8 or fp32 [0,1] stack, NumPy (uploaded on first use) or a device tensor, channels in the order the
        patches should have unless swap_rb; labels: one class id per frame."""
        if len(frames.shape) != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise ValueError("the frame stack must be [N,H,W,3] with N >= 1")
        if str(frames.dtype).replace("torch.", "") not in ("uint8", "float32"):
            raise ValueError("the frame stack must be uint8 or float32")
        labels = np.asarray(labels)
        if labels.ndim != 1 or len(labels) != frames.shape[0] or not (np.issubdtype(labels.dtype, np.integer) or labels.dtype == bool):
            raise ValueError("labels: one integer class id per frame")
        table = window_table_defects(int(frames.shape[0]), frames.shape[1:3], patch_size, stride)
        return cls(_LabeledStore(frames, table, labels.astype(np.int64)[table[:, 0]], patch_size, swap_rb, ctx))

    @classmethod
    def from_dirs(cls, hr_root, patch_size=33, stride=14, class_map_path=None):
        """The dataset load_defects_dataset_as_patches(...) returns for the same arguments: the same validation and messages, the same file
        order, KeyError for a basename the class map lacks, PIL decode to uint8, one upload."""
        from SRModels import loading_methods as LM
        from PIL import Image
        if not os.path.exists(hr_root):
            raise ValueError("HR root directory must exist.")
        if not os.path.isdir(hr_root):
            raise ValueError("HR root path must be a directory.")
        if not isinstance(patch_size, int) or patch_size <= 0:
            raise ValueError("patch_size must be positive int.")
        if not isinstance(stride, int) or stride <= 0:
            raise ValueError("stride must be positive int.")
        class_map = LM._load_class_map(class_map_path)
        paths = LM.get_all_image_paths(hr_root)
        if not paths:
            raise ValueError("No images found under HR root directory.")
        paths = sorted(paths, key=os.path.basename)
        imgs, labels = [], []
        for path in paths:
            with Image.open(path) as im:
                a = np.asarray(im.convert("RGB"), dtype=np.uint8)
            base = os.path.basename(path)
            if base not in class_map:
                raise KeyError(f"Missing class id for image basename in class_labels_map: {base}")
            if imgs and a.shape != imgs[0].shape:
                raise ValueError(f"image {path} is {a.shape[0]} x {a.shape[1]}, the first ({paths[0]}) is {imgs[0].shape[0]} x "
                                 f"{imgs[0].shape[1]}: a LabeledPatches needs one frame size")
            imgs.append(a)
            labels.append(int(class_map[base]))
        return cls.from_stacks(np.stack(imgs), np.array(labels, np.int64), patch_size, stride)

    @classmethod
    def from_device(cls, frames_u8, labels, channel_order="bgr", patch_size=33, stride=14):
        """Device crops (data.common_methods.square_crop_batch: uint8 [N,S,S,3], BGR) and their class ids as a dataset, without a PNG in
        between.  channel_order "bgr" is swapped to the loader's RGB in the gather."""
        if channel_order not in ("bgr", "rgb"):
            raise ValueError("channel_order must be 'bgr' or 'rgb'")
        return cls.from_stacks(frames_u8, labels, patch_size, stride, swap_rb=channel_order == "bgr")

    # ---- the loader's surface
    def __len__(self):
        return len(self._s.table) if self.index is None else len(self.index)

    def __repr__(self):
        return f"LabeledPatches({len(self)} patches, patch={self._s.patch_size})"

    patch_size = property(lambda self: self._s.patch_size)
    frame_size = property(lambda self: (int(self._s.frames.shape[1]), int(self._s.frames.shape[2])))

    @property
    def y(self):
        """int64 [len]: the class id of every patch's frame -- the loader's y."""
        return self._s.labels.copy() if self.index is None else self._s.labels[self.index]

    @property
    def windows(self):
        """int32 [len,3]: (image, y, x) of this dataset's patches."""
        return self._s.table if self.index is None else self._s.table[self.index]

    def rows(self, indices):
        """Patch numbers of THIS dataset -> rows of the shared window table."""
        idx = _check_indices(indices, len(self), "patch indices")
        return idx if self.index is None else self.index[idx]

    def subset(self, indices):
        """The dataset of patches `indices` (in that order), sharing the stack and the table."""
        return LabeledPatches(self._s, self.rows(indices))

    def host_bytes(self):
        """Bytes this dataset holds on the host: the window table, the labels, the subset's index, and the stack while it is not uploaded."""
        s = self._s
        return s.table.nbytes + s.labels.nbytes + (0 if self.index is None else self.index.nbytes) + (s.frames.nbytes if isinstance(s.frames, np.ndarray) else 0)

    def device_bytes(self):
        """Bytes this dataset holds (or, before its first batch, will hold) on the device: the stack and the window table."""
        f = self._s.frames
        return int(np.prod([int(v) for v in f.shape])) * (1 if str(f.dtype).replace("torch.", "") == "uint8" else 4) + self._s.table.nbytes

    # ---- batches
    def set_order(self, host_permutation):
        """An order over this dataset's patches (an epoch's permutation), validated on the host -> int32 device tensor of table rows."""
        s = self._s.on_device()
        return s.ctx.to_device(self.rows(host_permutation).astype(np.int32))

    def batch(self, order_dev, offset, B):
        """Patches order_dev[offset : offset + B] (order_dev from set_order) -> fp32 device [B,p,p,3], the loader's values."""
        s = self._s.on_device()
        return s.ctx.gather_patch_pairs(dict(stack=s.frames, swap=s.swap), None, s.table_dev, order_dev, offset, B, s.patch_size)[0]

    def warped_batch(self, order_dev, offset, B, params):
        """The same patches through the augmentation warp (params fp32 [B,16]: Context.warp_params) -> fp32 device [B,p,p,3]: bit for bit
        ctx.affine_warp of the loader's array at those patches, without the array."""
        s = self._s.on_device()
        return s.ctx.gather_warp_patches(s.frames, s.table_dev, order_dev, offset, B, s.patch_size, params, swap=s.swap)


def _resized_unit(ctx, lr_u8, H, W, codes, swap):
    """uint8 device stack -> the loader's np.clip(resize(lr / 255, (W, H), code), 0, 1) per image, fp32 device [N,H,W,3]."""
    import torch
    from . import _lib as L
    unit = ctx.u8_to_unit(lr_u8, swap=swap)
    out = ctx.empty((unit.shape[0], H, W, 3), torch.float32)
    for i, code in enumerate(codes):
        out[i:i + 1] = ctx.eltwise(L.ELT_CLIP01, ctx.resize(unit[i:i + 1], H, W, code))
    return out
