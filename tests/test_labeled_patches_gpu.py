"""The classifier's device patch dataset on the device (sr355.patches.LabeledPatches, sr_gather_warp_patches): plain and augmented batches
against load_defects_dataset_as_patches' array and ctx.affine_warp of it, and FineTunedVGG16.fit / evaluate / predict on views against the
same calls on the arrays.  The bar everywhere is bit equality: the view path does the array path's arithmetic operation for operation.

Geometries (tests/labeled_patches_ref.py): (37, 53) / 11 / 5 -- odd sizes, 363 values per patch (no multiple of 4: sr_affine_warp's scalar
kernel is the reference), the frame's last rows and columns in no window; (32, 32) / 32 / 16 -- the patch is the frame, the origin clamp
range a single point; (150, 130) / 96 / 48 -- the reference's patch and stride; (40, 36) / 8 / 4 -- many small windows, most of them in the
frame's interior, where a warp clamped to the frame instead of the patch would read the real neighbouring pixels."""
import numpy as np
import pytest
import torch

import labeled_patches_ref as R
from sr355.patches import LabeledPatches
from SRModels.loading_methods import load_defects_dataset_as_patches

pytestmark = pytest.mark.gpu

_cases = {}


@pytest.fixture(scope="module")
def case(ctx, tmp_path_factory):
    """geometry -> the PNG tree, the loader's (X, y) (computed once, never written to), X on the device and the directory dataset."""
    def get(geom):
        if geom not in _cases:
            hw, patch, stride = geom
            hr_root, cmap, frames, labels = R.write_tree(tmp_path_factory.mktemp("tree"), 3, hw, seed=sum(hw))
            X, y = load_defects_dataset_as_patches(hr_root, patch, stride, cmap)
            Xd = ctx.to_device(X)
            X.setflags(write=False)
            _cases[geom] = dict(hr_root=hr_root, cmap=cmap, frames=frames, labels=labels, X=X, y=y, Xd=Xd,
                                ds=LabeledPatches.from_dirs(hr_root, patch, stride, cmap))
        return _cases[geom]
    yield get
    _cases.clear()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _sources(ctx, c, geom):
    _, patch, stride = geom
    yield "dirs", c["ds"]
    yield "bgr", LabeledPatches.from_device(ctx.to_device(np.ascontiguousarray(c["frames"][..., ::-1])), c["labels"], "bgr", patch, stride)
    yield "fp32", LabeledPatches.from_stacks(c["frames"].astype(np.float32) / 255.0, c["labels"], patch, stride)


# ---------------------------------------------------------------------------------------------------------------- plain batches
@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_plain_batches_equal_the_loader(ctx, case, geom):
    c = case(geom)
    X, n = c["X"], len(c["X"])
    k = 5 if n <= 10 else 25
    assert n % k != 0                                                    # the walk ends in a partial batch
    for name, ds in _sources(ctx, c, geom):
        assert len(ds) == n and np.array_equal(ds.y, c["y"])
        perm = np.random.default_rng(n).permutation(n)
        order = ds.set_order(perm)
        got = np.empty_like(X)
        for i in range(0, n, k):
            b = ds.batch(order, i, min(k, n - i))
            assert b.dtype == torch.float32 and tuple(b.shape) == (min(k, n - i),) + X.shape[1:]
            got[perm[i:i + k]] = b.cpu().numpy()
        assert np.array_equal(bits(got), bits(X)), name
        one = ds.batch(order, n // 2, 1).cpu().numpy()
        assert np.array_equal(bits(one), bits(X[perm[n // 2:n // 2 + 1]])), name
    assert np.array_equal(bits(c["ds"].X.numpy(chunk=7)), bits(X))
    sub = np.random.default_rng(1).permutation(n)[:max(1, n // 2)]
    assert np.array_equal(bits(c["ds"].X[sub].numpy(chunk=7)), bits(X[sub]))


# ---------------------------------------------------------------------------------------------------------------- warped batches
def _picks(n, seed):
    """An order of 40 patch numbers (a permutation, repeated where the dataset is smaller): batches of up to 33 at offset 3."""
    return np.resize(np.random.default_rng(seed).permutation(n), max(n, 40))


@pytest.mark.parametrize("B", [1, 7, 33])
@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_warped_batches_equal_affine_warp_of_the_loaders_array(ctx, case, geom, B):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    c = case(geom)
    hw, patch, _ = geom
    n = len(c["X"])
    picks = _picks(n, 100 + B)
    off = 3
    rows = picks[off:off + B]
    rot, offset, flip = FineTunedVGG16._augment_params(np.random.default_rng(7 * B + patch), B, patch, patch)
    params = ctx.warp_params(rot, offset, flip)
    ref = ctx.affine_warp(c["Xd"], rows, params).cpu().numpy()
    # the draws do what the case is for: samples fall outside the patch on every side (both clamps act)
    oy, ox = np.meshgrid(np.arange(patch), np.arange(patch), indexing="ij")
    sy = rot[:, 0, 0, None, None] * oy + rot[:, 0, 1, None, None] * ox + offset[:, 0, None, None]
    sx = rot[:, 1, 0, None, None] * oy + rot[:, 1, 1, None, None] * ox + offset[:, 1, None, None]
    if B > 1:
        assert sy.min() < 0 and sx.min() < 0 and sy.max() > patch - 1 and sx.max() > patch - 1
    win = c["ds"].windows[rows]
    if geom in (R.GEOMETRIES[0], R.GEOMETRIES[3]) and B > 1:             # interior windows: real pixels on every side of the patch
        assert np.any((win[:, 1] > 0) & (win[:, 2] > 0) & (win[:, 1] + patch < hw[0]) & (win[:, 2] + patch < hw[1]))
    for name, ds in _sources(ctx, c, geom):
        y = ds.warped_batch(ds.set_order(picks), off, B, ctx.to_device(params))
        assert y.dtype == torch.float32 and tuple(y.shape) == (B, patch, patch, 3)
        assert np.array_equal(bits(y.cpu().numpy()), bits(ref)), (name, float(np.abs(y.cpu().numpy() - ref).max()))


@pytest.mark.parametrize("geom", R.GEOMETRIES)
def test_warped_batches_exact_cases(ctx, case, geom):
    c = case(geom)
    _, patch, _ = geom
    X, n = c["X"], len(c["X"])
    picks = _picks(n, 5)
    B, off = 9, 2
    rows = picks[off:off + B]
    eye, zero, no = np.broadcast_to(np.eye(2), (B, 2, 2)), np.zeros((B, 2)), np.zeros(B, bool)
    for name, ds in _sources(ctx, c, geom):
        order = ds.set_order(picks)
        plain = ds.batch(order, off, B).cpu().numpy()
        assert np.array_equal(bits(plain), bits(X[rows]))
        ident = ds.warped_batch(order, off, B, ctx.warp_params(eye, zero, no)).cpu().numpy()
        assert np.array_equal(bits(ident), bits(plain)), name                                  # identity: batch()'s bits
        flip = np.arange(B) % 2 == 0
        fl = ds.warped_batch(order, off, B, ctx.warp_params(eye, zero, flip)).cpu().numpy()
        assert np.array_equal(bits(fl), bits(np.where(flip[:, None, None, None], plain[:, :, ::-1], plain))), name   # the column mirror
        # integer shifts, some past the border: the patch's own edge rows / columns replicated, never the frame's pixels beyond them
        shifts = np.array([[3, -7], [-4, 11], [patch + 5, 0], [0, -(patch + 9)], [2, 2], [-1, 0], [0, 1], [-patch, patch], [1, -1]], np.float64)
        sh = ds.warped_batch(order, off, B, ctx.warp_params(eye, shifts, no)).cpu().numpy()
        oy, ox = np.meshgrid(np.arange(patch), np.arange(patch), indexing="ij")
        for b in range(B):
            yy, xx = np.clip(oy + int(shifts[b, 0]), 0, patch - 1), np.clip(ox + int(shifts[b, 1]), 0, patch - 1)
            assert np.array_equal(bits(sh[b]), bits(X[rows[b]][yy, xx])), (name, b)


# ---------------------------------------------------------------------------------------------------------------- bad arguments
def test_gather_warp_patches_rejects_bad_arguments(ctx):
    """Everything here is refused on the host or by the ABI before a launch; no kernel is handed an out-of-range table."""
    from sr355.patches import window_table_defects
    stack = ctx.to_device(np.zeros((2, 12, 14, 3), np.uint8))
    win = ctx.to_device(window_table_defects(2, (12, 14), 8, 4))
    order = ctx.to_device(np.arange(4, dtype=np.int32))
    p = ctx.to_device(ctx.warp_params(np.broadcast_to(np.eye(2), (3, 2, 2)), np.zeros((3, 2)), np.zeros(3, bool)))
    assert tuple(ctx.gather_warp_patches(stack, win, order, 1, 3, 8, p).shape) == (3, 8, 8, 3)      # the good call
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack.to(torch.int16), win, order, 0, 3, 8, p)                      # stack dtype
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack.double(), win, order, 0, 3, 8, p)
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 0, 3, 8, p.double())                              # params dtype
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win.long(), order, 0, 3, 8, p)                                # int64 tables
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order.long(), 0, 3, 8, p)
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 0, 2, 8, p)                                       # params for another B
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 0, 3, 8, p[:, :12].contiguous())
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 2, 3, 8, p)                                       # the batch reaches past order
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, -1, 3, 8, p)
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 0, 3, 13, p)                                      # a patch larger than the frame
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack, win, order, 0, 3, (8, 15), p)
    with pytest.raises(ValueError):
        ctx.gather_warp_patches(stack[0], win, order, 0, 3, 8, p)                                    # not a stack
    # the ABI's own refusals, behind the host's: SR_ERR_INVALID and no launch
    from sr355 import _lib as L
    out = ctx.empty((3, 8, 8, 3))
    args = lambda **k: [k.get(a, d) for a, d in (("src", stack.data_ptr()), ("dtype", L.DTYPE_U8), ("N", 2), ("H", 12), ("W", 14), ("win", win.data_ptr()),
                                                 ("n_win", int(win.shape[0])), ("order", order.data_ptr()), ("n_order", 4), ("offset", 0), ("B", 3), ("ph", 8),
                                                 ("pw", 8), ("swap", 0), ("params", p.data_ptr()), ("y", out.data_ptr()))]
    call = lambda **k: ctx.lib.sr_gather_warp_patches(ctx.h, *args(**k), ctx.stream())
    assert call() == L.SR_OK
    for bad in (dict(src=None), dict(win=None), dict(order=None), dict(params=None), dict(y=None), dict(dtype=L.DTYPE_BF16), dict(N=0), dict(H=0),
                dict(W=0), dict(B=0), dict(ph=0), dict(pw=0), dict(ph=13), dict(pw=15), dict(offset=-1), dict(offset=2), dict(n_order=2), dict(n_win=0),
                dict(B=65536, n_order=1 << 20), dict(B=40000, ph=200, pw=200, H=200, W=200, n_order=1 << 20)):
        assert call(**bad) == L.SR_ERR_INVALID, bad
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- fits
@pytest.fixture(scope="module")
def fit_data():
    """Five 48 x 64 frames, patch 32, stride 16: 30 patches, split 22 / 8 by index.  -> the dataset, the loader's array form and the split."""
    frames = np.random.default_rng(21).integers(0, 256, (5, 48, 64, 3), dtype=np.uint8)
    ds = LabeledPatches.from_stacks(frames, np.array([0, 1, 1, 0, 1]), 32, 16)
    assert len(ds) == 30
    X = np.stack([frames[n, i:i + 32, j:j + 32] for n, i, j in ds.windows]).astype(np.float32) / 255.0        # the loader's X, element for element
    perm = np.random.default_rng(2).permutation(30)
    itr, iva = perm[:22], perm[22:]
    assert len(set(ds.y[itr])) == 2 and len(set(ds.y[iva])) == 2
    return ds, X, ds.y, itr, iva


def _model(**kw):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    m = FineTunedVGG16()
    m.setup_model(input_shape=(32, 32, 3), num_classes=2, dropout_rate=0.2, **kw)
    return m


def _same_fit(a, b):
    (ma, ha), (mb, hb) = a, b
    assert ha.history == hb.history, (ha.history, hb.history)
    for n in ("dense", "predictions"):
        for s in (0, 1):
            assert np.array_equal(bits(ma.weights[n][s]), bits(mb.weights[n][s])), (n, s)


@pytest.fixture(scope="module")
def array_fits(ctx, fit_data):
    """The two array fits the view fits are compared with, run once."""
    ds, X, y, itr, iva = fit_data
    out = {}
    for key, kw in (("aug", dict(epochs=2, use_augmentation=True, seed=9)), ("plain", dict(epochs=2, use_augmentation=False, batch_size=8, seed=9))):
        m = _model()
        out[key] = (m, m.fit(X[itr], y[itr], X[iva], y[iva], **kw))
    return out


def test_loader_array_form_of_the_fit_data(ctx, fit_data):
    ds, X, y, itr, iva = fit_data
    assert np.array_equal(bits(ds.X.numpy()), bits(X)) and np.array_equal(bits(ds.X[itr].numpy()), bits(X[itr]))


def test_fit_on_views_equals_fit_on_arrays_with_augmentation_and_dropout(ctx, fit_data, array_fits):
    ds, X, y, itr, iva = fit_data
    train, val = ds.subset(itr), ds.subset(iva)
    m = _model()
    h = m.fit(train.X, y[itr], val.X, y[iva], epochs=2, use_augmentation=True, seed=9)
    assert len(h.history["loss"]) == 2 and np.isfinite(h.history["loss"]).all()
    _same_fit((m, h), array_fits["aug"])


def test_fit_on_views_equals_fit_on_arrays_without_augmentation(ctx, fit_data, array_fits):
    ds, X, y, itr, iva = fit_data
    m = _model()
    h = m.fit(ds.X[itr], y[itr], ds.X[iva], y[iva], batch_size=8, epochs=2, use_augmentation=False, seed=9)      # 22 = 8 + 8 + 6
    _same_fit((m, h), array_fits["plain"])


def test_fit_with_a_view_for_training_and_an_array_for_validation(ctx, fit_data, array_fits):
    ds, X, y, itr, iva = fit_data
    m = _model()
    h = m.fit(ds.X[itr], y[itr], X[iva], y[iva], epochs=2, use_augmentation=True, seed=9)
    _same_fit((m, h), array_fits["aug"])
    m2 = _model()
    h2 = m2.fit(X[itr], y[itr], ds.X[iva], y[iva], batch_size=8, epochs=2, use_augmentation=False, seed=9)
    _same_fit((m2, h2), array_fits["plain"])


def test_view_fit_builds_no_patch_array(ctx, fit_data, monkeypatch):
    """A view fit never asks for the patches as an array, and never warps an fp32 patch set."""
    from sr355.patches import LabeledView
    from sr355.runtime import Context

    def boom(*a, **k):
        raise AssertionError("the array path was used")

    monkeypatch.setattr(LabeledView, "numpy", boom)
    monkeypatch.setattr(Context, "affine_warp", boom)
    ds, X, y, itr, iva = fit_data
    m = _model()
    h = m.fit(ds.X[itr], y[itr], ds.X[iva], y[iva], epochs=1, use_augmentation=True, seed=1)
    assert len(h.history["loss"]) == 1 and np.isfinite(h.history["val_loss"]).all()


def test_evaluate_and_predict_on_a_view_equal_the_array(ctx, fit_data, array_fits, capsys):
    ds, X, y, itr, iva = fit_data
    m = array_fits["aug"][0]
    for bs in (32, 7):                                                   # 30 patches: a partial forward batch either way
        pa, pv = m.predict(X, batch_size=bs), m.predict(ds.X, batch_size=bs)
        assert isinstance(pv, np.ndarray) and pv.dtype == pa.dtype and pv.shape == pa.shape == (30, 2)
        assert np.array_equal(bits(pv), bits(pa)), bs
    assert np.array_equal(bits(m.predict(ds.X[iva])), bits(m.predict(X[iva])))
    assert m.evaluate(ds.X[iva], y[iva]) == m.evaluate(X[iva], y[iva])
    assert m.evaluate(ds.X, y) == m.evaluate(X, y)
