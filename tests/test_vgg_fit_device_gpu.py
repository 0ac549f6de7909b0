"""FineTunedVGG16.fit on the device (VGG16_model.py:111-157): the augmentation warp (sr_affine_warp) against SciPy, the head step
(sr_dense_head_step) against the host reference head_forward / head_backward / sparse_cce, and whole fits against the host path composed
from _augment, _gap_features and fit_head on the same seeds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _ref_warp(img, rot, off, flip):
    """scipy.ndimage.affine_transform(order=1, mode='nearest') per channel in fp64, then the flip: what _augment computes per image."""
    from scipy import ndimage
    out = np.stack([ndimage.affine_transform(img[:, :, c].astype(np.float64), rot, offset=off, order=1, mode="nearest")
                    for c in range(img.shape[2])], -1)
    return out[:, ::-1] if flip else out


# ---------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("hw", [(32, 32), (128, 128), (37, 53)])
def test_affine_warp_matches_scipy(ctx, hw, C):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    H, W = hw
    rng = np.random.default_rng(H * 100 + W + C)
    X = rng.uniform(0, 1, (8, H, W, C)).astype(np.float32)
    idx = rng.integers(0, 8, 6)
    rot, off, flip = FineTunedVGG16._augment_params(np.random.default_rng(3), 6, H, W)
    y = ctx.affine_warp(ctx.to_device(X), idx, ctx.warp_params(rot, off, flip)).cpu().numpy()
    assert y.shape == (6, H, W, C) and y.dtype == np.float32
    err = max(float(np.abs(y[b] - _ref_warp(X[i], rot[b], off[b], flip[b])).max()) for b, i in enumerate(idx))
    assert err <= 2e-5, err


def test_affine_warp_is_augment(ctx):
    """_augment(x, rng) and the device warp on _augment_params drawn from the same seed."""
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    X = np.random.default_rng(5).uniform(0, 1, (10, 40, 36, 3)).astype(np.float32)
    ref = FineTunedVGG16._augment(X, np.random.default_rng(11))
    p = ctx.warp_params(*FineTunedVGG16._augment_params(np.random.default_rng(11), 10, 40, 36))
    y = ctx.affine_warp(ctx.to_device(X), np.arange(10), p).cpu().numpy()
    assert float(np.abs(y - ref).max()) <= 2e-5


def test_affine_warp_exact_cases(ctx):
    rng = np.random.default_rng(8)
    H, W = 21, 30
    X = rng.uniform(0, 1, (5, H, W, 3)).astype(np.float32)
    Xd = ctx.to_device(X)
    idx = np.array([4, 0, 0, 2, 3, 1, 4], np.int32)
    n = len(idx)
    eye = np.broadcast_to(np.eye(2), (n, 2, 2))
    ident = ctx.affine_warp(Xd, idx, ctx.warp_params(eye, np.zeros((n, 2)), np.zeros(n, bool))).cpu().numpy()
    assert np.array_equal(ident, X[idx])                                                   # an indexed gather, bit for bit
    flip = np.arange(n) % 2 == 0
    fl = ctx.affine_warp(Xd, idx, ctx.warp_params(eye, np.zeros((n, 2)), flip)).cpu().numpy()
    assert np.array_equal(fl, np.where(flip[:, None, None, None], X[idx][:, :, ::-1], X[idx]))
    # integer shifts, some past the border: every tap is an integer index, clamped -- the edge rows / columns replicated exactly
    shifts = np.array([[3, -7], [-4, 11], [H + 5, 0], [0, -(W + 9)], [2, 2], [-1, 0], [0, 1]], np.float64)
    sh = ctx.affine_warp(Xd, idx, ctx.warp_params(eye, shifts, np.zeros(n, bool))).cpu().numpy()
    oy, ox = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for b in range(n):
        yy, xx = np.clip(oy + int(shifts[b, 0]), 0, H - 1), np.clip(ox + int(shifts[b, 1]), 0, W - 1)
        assert np.array_equal(sh[b], X[idx[b]][yy, xx]), b
    assert np.array_equal(sh[2], np.broadcast_to(X[idx[2]][H - 1], (H, W, 3)))


def test_affine_warp_rejects_bad_arguments(ctx):
    X = ctx.to_device(np.zeros((3, 8, 8, 3), np.float32))
    p = ctx.warp_params(np.broadcast_to(np.eye(2), (2, 2, 2)), np.zeros((2, 2)), np.zeros(2, bool))
    with pytest.raises(ValueError):
        ctx.affine_warp(X, np.array([0, 3]), p)                                         # index out of range
    with pytest.raises(ValueError):
        ctx.affine_warp(X, np.array([-1, 0]), p)
    with pytest.raises(ValueError):
        ctx.affine_warp(X.double(), np.array([0, 1]), p)                                # wrong dtype
    with pytest.raises(ValueError):
        ctx.affine_warp(X, ctx.to_device(np.array([0, 1], np.int64)), p)               # int64 device indices
    with pytest.raises(ValueError):
        ctx.affine_warp(X, np.array([0, 1, 2]), p)                                      # params for another batch size


# ---------------------------------------------------------------------------------------------------------------- head step
def _head_case(n, C, seed):
    rng = np.random.default_rng(seed)
    g = rng.uniform(0, 2, (n, 512)).astype(np.float32)
    w = {"dense": ((rng.normal(size=(512, 256)) * np.sqrt(2 / 512)).astype(np.float32), (rng.normal(size=256) * 0.05).astype(np.float32)),
         "predictions": ((rng.normal(size=(256, C)) * np.sqrt(2 / 256)).astype(np.float32), (rng.normal(size=C) * 0.05).astype(np.float32))}
    y = rng.integers(0, C, n)
    return g, w, y


@pytest.mark.parametrize("n", [1, 7, 32, 100])
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("l2_reg", [0.0, 1e-3])
def test_dense_head_step_matches_host(ctx, n, C, l2_reg):
    from sr355.train import Adam, DeviceAdam, ParamBucket, head_backward, head_forward, sparse_cce
    g, w, y = _head_case(n, C, 1000 * n + 10 * C + int(l2_reg > 0))
    rate, keep = 0.2, 0.8
    # the host's masks come from head_forward's own draws; the device gets the same draws as uint8 keep masks
    w64 = {k: (a.astype(np.float64), b.astype(np.float64)) for k, (a, b) in w.items()}
    p, cache = head_forward(g.astype(np.float64), w64, True, rate, np.random.default_rng(77))
    mr = np.random.default_rng(77)
    m0, m1 = (mr.random((n, 512)) < keep).astype(np.uint8), (mr.random((n, 256)) < keep).astype(np.uint8)
    loss, acc = sparse_cce(p, y)
    ref = head_backward(p, y, cache, w64, l2_reg)

    bucket = ParamBucket(ctx, w)
    grads = torch.empty_like(bucket.flat)
    stats = ctx.empty((3,), torch.float64)
    work = ctx.dense_head_workspace(n, C)
    yd = ctx.to_device(y.astype(np.int32))
    ctx.dense_head_step(ctx.to_device(g), yd, bucket.flat, C, stats, work, grads, ctx.to_device(m0), ctx.to_device(m1), 1.0 / keep, l2_reg)
    st = stats.cpu().numpy()
    assert abs(st[0] / n - loss) <= 1e-5 * abs(loss) and st[1] / n == pytest.approx(acc)
    assert abs(st[2] - float(np.sum(w64["dense"][0] ** 2))) <= 1e-9 * st[2]
    gd = bucket.split(grads.cpu().numpy())
    for layer in ("dense", "predictions"):
        for s in (0, 1):
            assert rel_l2(gd[layer][s], ref[layer][s]) <= 1e-5, (layer, s, rel_l2(gd[layer][s], ref[layer][s]))
    # one Adam step through DeviceAdam against the host Adam on the device's gradients: the moments bit for bit; the weights within one
    # fp32 ulp of the weight plus four of the step (sr_adam's step lr_t m / (sqrt(v) + eps) can differ from NumPy's in its last bits)
    ha = Adam(w, 1e-3, epsilon=1e-7)
    host = ha.apply(w, {k: (a.copy(), b.copy()) for k, (a, b) in gd.items()})
    da = DeviceAdam(ctx, bucket.flat, 1e-3, epsilon=1e-7)
    da.apply(bucket.flat, grads)
    assert np.array_equal(da.m.cpu().numpy(), np.concatenate([a.ravel() for k in ("dense", "predictions") for a in ha.m[k]]))
    assert np.array_equal(da.v.cpu().numpy(), np.concatenate([a.ravel() for k in ("dense", "predictions") for a in ha.v[k]]))
    bucket.stale = True
    for layer in ("dense", "predictions"):
        for s in (0, 1):
            a, b = bucket.host()[layer][s], host[layer][s]
            assert np.all(np.abs(a - b) <= np.spacing(np.abs(b)) + 4 * np.spacing(np.abs(w[layer][s] - b))), layer
    # inference mode: no dropout, no gradients -- the validation pass of fit
    pi, _ = head_forward(g.astype(np.float64), w64)
    li, ai = sparse_cce(pi, y)
    bucket.load(w)
    ctx.dense_head_step(ctx.to_device(g), yd, bucket.flat, C, stats, work)
    st = stats.cpu().numpy()
    assert abs(st[0] / n - li) <= 1e-5 * abs(li) and st[1] / n == pytest.approx(ai)


def test_dense_head_step_rejects_bad_arguments(ctx):
    g, w, y = _head_case(4, 3, 1)
    from sr355.train import ParamBucket
    b = ParamBucket(ctx, w)
    grads, stats, work = torch.empty_like(b.flat), ctx.empty((3,), torch.float64), ctx.dense_head_workspace(4, 3)
    gd, yd = ctx.to_device(g), ctx.to_device(y.astype(np.int32))
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, ctx.to_device(y), b.flat, 3, stats, work, grads)          # int64 labels
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 4, stats, work, grads)                         # bucket of another class count
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd[:, :256].contiguous(), yd, b.flat, 3, stats, work, grads)   # not 512 features
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, ctx.dense_head_workspace(2, 3), grads)   # workspace too small
    m = ctx.to_device(np.ones((4, 512), np.uint8))
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, work, grads, keep0=m)              # one mask without the other


# ---------------------------------------------------------------------------------------------------------------- fit
def _data(seed=21, n=20, nv=8, hw=32):
    rng = np.random.default_rng(seed)
    X, y = rng.uniform(0, 1, (n, hw, hw, 3)).astype(np.float32), rng.integers(0, 2, n)
    Xv, yv = rng.uniform(0, 1, (nv, hw, hw, 3)).astype(np.float32), rng.integers(0, 2, nv)
    return X, y, Xv, yv


def _model(dtype="f32", **kw):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    m = FineTunedVGG16(compute_dtype=dtype)
    m.setup_model(input_shape=(32, 32, 3), num_classes=2, **kw)
    return m


def _host_fit(m, X, y, Xv, yv, epochs, seed, use_augmentation=True, batch_size=32):
    """The pre-device fit, composed from its host parts: _augment, _gap_features and fit_head, on the same seeds."""
    from sr355.train import fit_head
    rng = np.random.default_rng(seed)
    bs = 32 if use_augmentation else batch_size

    def batches(epoch):
        order = rng.permutation(len(X))
        for i in range(0, len(order), bs):
            idx = order[i:i + bs]
            yield (m._augment(X[idx], rng) if use_augmentation else X[idx]), y[idx]

    return fit_head(m._gap_features, m.weights, batches, y, Xv, yv, learning_rate=m.learning_rate, batch_size=bs, epochs=epochs,
                    dropout_rate=m.dropout_rate, l2_reg=m.l2_reg, seed=seed)


def test_fit_device_matches_host_reference_with_augmentation_and_dropout(ctx):
    X, y, Xv, yv = _data()
    m = _model(dropout_rate=0.2)
    w0 = {n: (k.copy(), b.copy()) for n, (k, b) in m.weights.items()}
    head_h, hist_h = _host_fit(m, X, y, Xv, yv, 3, 9)
    hist = m.fit(X, y, Xv, yv, epochs=3, use_augmentation=True, seed=9)
    for k in ("loss", "accuracy", "val_loss", "val_accuracy", "lr"):
        assert np.allclose(hist.history[k], hist_h.history[k], rtol=1e-3, atol=0), (k, hist.history[k], hist_h.history[k])
    for n in ("dense", "predictions"):
        assert rel_l2(m.weights[n][0] - w0[n][0], head_h[n][0] - w0[n][0]) <= 5e-3, n
    assert all(np.array_equal(m.weights[n][0], w0[n][0]) and np.array_equal(m.weights[n][1], w0[n][1]) for n in w0 if n.startswith("block"))
    m2 = _model(dropout_rate=0.2)
    hist2 = m2.fit(X, y, Xv, yv, epochs=3, use_augmentation=True, seed=9)
    assert hist2.history == hist.history
    assert all(np.array_equal(m2.weights[n][s], m.weights[n][s]) for n in ("dense", "predictions") for s in (0, 1))


def test_fit_device_callbacks_match_host(ctx):
    """A learning rate of 0.05 without augmentation or dropout: ReduceLROnPlateau halves lr and EarlyStopping stops and restores the best
    epoch's head, on both paths at the same epochs.  Seed 3 was chosen so that every val_loss step is far, compared with the paths' rounding
    difference, from the callbacks' thresholds (lr_best - 1e-4 and best): the test checks that margin before it compares the decisions."""
    X, y, Xv, yv = _data()
    m = _model(dropout_rate=0.0, learning_rate=0.05)
    head_h, hist_h = _host_fit(m, X, y, Xv, yv, 30, 3, use_augmentation=False, batch_size=8)
    w0 = {n: (k.copy(), b.copy()) for n, (k, b) in m.weights.items()}
    hist = m.fit(X, y, Xv, yv, batch_size=8, epochs=30, use_augmentation=False, seed=3)
    vh, vd = np.array(hist_h.history["val_loss"]), np.array(hist.history["val_loss"])
    k = min(len(vh), len(vd))
    diff = float(np.abs(vh[:k] - vd[:k]).max())
    lr_best, best, margins = np.inf, np.inf, []
    for e in range(k):                                                        # the callbacks' two comparisons, replayed on the host history
        if e:
            margins += [abs(vh[e] - (lr_best - 1e-4)), abs(vh[e] - best)]
        if vh[e] < lr_best - 1e-4:
            lr_best = vh[e]
        best = min(best, vh[e])
    assert min(margins) > 20 * diff, (min(margins), diff)
    assert len(vh) == len(vd) < 30                                            # EarlyStopping fired, at the same epoch
    assert hist.history["lr"] == hist_h.history["lr"] and hist.history["lr"][-1] < 0.05     # ReduceLROnPlateau fired, at the same epochs
    for n in ("dense", "predictions"):
        assert rel_l2(m.weights[n][0] - w0[n][0], head_h[n][0] - w0[n][0]) <= 5e-3, n


def test_fit_runs_on_the_device(ctx, monkeypatch):
    """With the host parts of the old path disabled, fit still trains, with and without augmentation."""
    import sr355.train as T
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16

    def boom(*a, **k):
        raise AssertionError("host path used")

    monkeypatch.setattr(FineTunedVGG16, "_augment", staticmethod(boom))
    monkeypatch.setattr(FineTunedVGG16, "_gap_features", boom)
    monkeypatch.setattr(T, "fit_head", boom)
    X, y, Xv, yv = _data()
    for aug in (True, False):
        m = _model(dropout_rate=0.2)
        w0 = m.weights["dense"][0].copy()
        h = m.fit(X, y, Xv, yv, batch_size=8, epochs=2, use_augmentation=aug, seed=4)
        assert len(h.history["loss"]) == 2 and np.isfinite(h.history["loss"]).all() and not np.array_equal(m.weights["dense"][0], w0)


def test_fit_bf16_is_reproducible_and_trains_only_the_head(ctx):
    X, y, Xv, yv = _data()
    runs = []
    for _ in range(2):
        m = _model("bf16", dropout_rate=0.2)
        w0 = {n: (k.copy(), b.copy()) for n, (k, b) in m.weights.items()}
        h = m.fit(X, y, Xv, yv, epochs=2, use_augmentation=True, seed=9)
        assert np.isfinite(h.history["loss"]).all() and np.isfinite(h.history["val_loss"]).all()
        assert all(np.array_equal(m.weights[n][0], w0[n][0]) for n in w0 if n.startswith("block"))
        assert not np.array_equal(m.weights["dense"][0], w0["dense"][0])
        runs.append((h.history, {n: m.weights[n] for n in ("dense", "predictions")}))
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(runs[0][1][n][s], runs[1][1][n][s]) for n in ("dense", "predictions") for s in (0, 1))
