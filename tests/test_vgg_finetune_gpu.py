"""FineTunedVGG16.setup_model(fine_tune_base=True) on the device: the head step with its input gradient (sr_dense_head_step_dx), the fused
GAP / max-pool / ReLU backward (sr_pool_gap_bwd), the packed-tile weight gradient of small maps (sr_conv2d_wgrad_maps), one training step
of sr355.vgg_train.VGGFineTuner against the fp64 autograd reference (tests/vgg_finetune_ref.py) and whole fits through the public class.

Bounds: 1e-5 rel-L2 is the fp32 conv route bound of test_conv_routes_gpu.py and the head test's bound, 2e-6 the wgrad bound of
test_backward_kernels_gpu.py; the reference's own fp32-vs-fp64 distance at these seeds is 4-9e-7 per gradient and 2e-7 over the fit's
history (tests/test_vgg_finetune_cpu.py)."""
import numpy as np
import pytest
import torch

import vgg_finetune_ref as R
from vgg_finetune_ref import rel_l2

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------- sr_dense_head_step_dx
def _head_case(n, C, seed):
    """Features in [0, 0.25): the logits stay within about +-1, so no row's p[y] comes near 1.  Every gradient of a row is a multiple of
    p - onehot, whose fp32 relative error is eps * p[y] / (1 - p[y]): a row with 1 - p[y] = 1e-3 (features in [0, 2) produce them) carries
    2e-5 whatever the kernel does, in sr_dense_head_step's own gradients too, and with n = 1 that row is the whole batch."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(0, 0.25, (n, 512)).astype(np.float32)
    w = {"dense": ((rng.normal(size=(512, 256)) * np.sqrt(2 / 512)).astype(np.float32), (rng.normal(size=256) * 0.05).astype(np.float32)),
         "predictions": ((rng.normal(size=(256, C)) * np.sqrt(2 / 256)).astype(np.float32), (rng.normal(size=C) * 0.05).astype(np.float32))}
    return g, w, rng.integers(0, C, n)


@pytest.mark.parametrize("l2_reg", [0.0, 1e-3])
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("n", [1, 5, 32])
def test_head_step_dx_keeps_the_step_and_adds_the_input_gradient(ctx, n, C, dropout, l2_reg):
    from sr355.train import ParamBucket, head_backward, head_forward
    g, w, y = _head_case(n, C, 100 * n + 10 * C + 2 * dropout + int(l2_reg > 0))
    rate, keep = 0.2, 0.8
    w64 = {k: (a.astype(np.float64), b.astype(np.float64)) for k, (a, b) in w.items()}
    p, cache = head_forward(g.astype(np.float64), w64, dropout, rate, np.random.default_rng(77))
    mr = np.random.default_rng(77)
    m0, m1 = ((mr.random((n, 512)) < keep), (mr.random((n, 256)) < keep)) if dropout else (None, None)
    # head_backward, extended by one product: d loss / d feats = (dz1 k1^T) * m0 / keep.  dz1 is recomputed as head_backward computes it and
    # tied to its output through the dense kernel's gradient.
    assert np.min(1.0 - p[np.arange(n), y]) >= 0.05                                                   # the conditioning _head_case promises
    ref = head_backward(p, y, cache, w64, l2_reg)
    x0, z1, x1, m1s = cache
    dz2 = p.copy()
    dz2[np.arange(n), y] -= 1.0
    dz2 /= n
    dx1 = dz2 @ w64["predictions"][0].T
    dz1 = (dx1 * m1s if m1s is not None else dx1) * (z1 > 0)
    assert np.allclose(x0.T @ dz1 + 2.0 * l2_reg * w64["dense"][0], ref["dense"][0], rtol=1e-12, atol=1e-15)
    dfeats_ref = dz1 @ w64["dense"][0].T * (m0 / keep if dropout else 1.0)

    bucket = ParamBucket(ctx, w)
    work = ctx.dense_head_workspace(n, C)
    gd, yd = ctx.to_device(g), ctx.to_device(y.astype(np.int32))
    k0, k1 = (ctx.to_device(m0.astype(np.uint8)), ctx.to_device(m1.astype(np.uint8))) if dropout else (None, None)
    grads_a, stats_a = torch.full_like(bucket.flat, 7.0), ctx.empty((3,), torch.float64)
    ctx.dense_head_step(gd, yd, bucket.flat, C, stats_a, work, grads_a, k0, k1, 1.0 / keep, l2_reg)
    grads_b, stats_b, dfeats = torch.full_like(bucket.flat, -7.0), ctx.empty((3,), torch.float64), torch.full((n, 512), 9.0, device=gd.device)
    ctx.dense_head_step(gd, yd, bucket.flat, C, stats_b, work, grads_b, k0, k1, 1.0 / keep, l2_reg, dfeats=dfeats)
    assert torch.equal(grads_a, grads_b) and torch.equal(stats_a, stats_b)
    err = rel_l2(dfeats.cpu().numpy(), dfeats_ref)
    assert err <= 1e-5, err
    if dropout:
        assert np.all(dfeats.cpu().numpy()[~m0] == 0.0)


def test_head_step_dx_rejects_bad_arguments(ctx):
    from sr355 import _lib as L
    from sr355.train import ParamBucket
    g, w, y = _head_case(4, 3, 1)
    b = ParamBucket(ctx, w)
    grads, stats, work = torch.empty_like(b.flat), ctx.empty((3,), torch.float64), ctx.dense_head_workspace(4, 3)
    gd, yd, df = ctx.to_device(g), ctx.to_device(y.astype(np.int32)), ctx.empty((4, 512))
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, work, None, dfeats=df)                       # an input gradient without a training step
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, work, grads, dfeats=ctx.empty((4, 256)))     # not [n,512]
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, ctx.to_device(y), b.flat, 3, stats, work, grads, dfeats=df)        # int64 labels
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 4, stats, work, grads, dfeats=df)                      # bucket of another class count
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, ctx.dense_head_workspace(2, 3), grads, dfeats=df)   # workspace too small
    m = ctx.to_device(np.ones((4, 512), np.uint8))
    with pytest.raises(ValueError):
        ctx.dense_head_step(gd, yd, b.flat, 3, stats, work, grads, keep0=m, dfeats=df)             # one mask without the other
    # the C entry itself: null tensors, another head, one mask
    args = lambda **kw: [kw.get(k, v) for k, v in (("feats", gd.data_ptr()), ("n", 4), ("in_dim", 512), ("hidden", 256), ("nc", 3), ("labels", yd.data_ptr()),
                                                   ("k0", None), ("k1", None), ("scale", 1.0), ("params", b.flat.data_ptr()), ("l2", 0.0),
                                                   ("grads", grads.data_ptr()), ("dfeats", df.data_ptr()), ("stats", stats.data_ptr()),
                                                   ("work", work.data_ptr()), ("bytes", work.numel()), ("stream", ctx.stream()))]
    call = lambda **kw: ctx.lib.sr_dense_head_step_dx(ctx.h, *args(**kw))
    assert call() == L.SR_OK
    for bad in (dict(dfeats=None), dict(grads=None), dict(feats=None), dict(labels=None), dict(params=None), dict(stats=None), dict(work=None),
                dict(in_dim=256), dict(hidden=512), dict(nc=1), dict(n=0), dict(k0=m.data_ptr())):
        assert call(**bad) == L.SR_ERR_INVALID, bad
    assert call(bytes=16) == L.SR_ERR_CAPACITY


# ---------------------------------------------------------------------------------------------------------------- sr_pool_gap_bwd
def _pool_gap_composition(ctx, a, dfeats):
    """The three launches sr_pool_gap_bwd replaces: the GAP spread, sr_maxpool2_bwd, SR_ELT_RELU_BWD."""
    from sr355 import _lib as L
    B, H, W, C = a.shape
    spread = (dfeats / torch.full_like(dfeats, float((H // 2) * (W // 2))))[:, None, None, :].expand(B, H // 2, W // 2, C).contiguous()
    return ctx.eltwise(L.ELT_RELU_BWD, ctx.maxpool2_bwd(a, spread), a)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [512, 20])
@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (4, 4), (6, 6), (8, 8)])
def test_pool_gap_bwd_is_the_three_launch_composition(ctx, hw, C, B):
    H, W = hw
    rng = np.random.default_rng(H * 1000 + W * 100 + C + B)
    a = ctx.to_device(np.maximum(rng.normal(size=(B, H, W, C)), 0).astype(np.float32))              # a ReLU output: half of it zero
    df = ctx.to_device(rng.normal(size=(B, C)).astype(np.float32))
    out = ctx.pool_gap_bwd(a, df)
    assert torch.equal(out, _pool_gap_composition(ctx, a, df))
    o = out.cpu().numpy()
    assert np.all(o[:, 2 * (H // 2):] == 0) and np.all(o[:, :, 2 * (W // 2):] == 0)                 # floor: an odd last row / column gets nothing
    assert np.count_nonzero(o) <= B * (H // 2) * (W // 2) * C                                       # at most one element per window


def test_pool_gap_bwd_ties(ctx):
    """All-zero windows give nothing (a > 0 fails); equal positive maxima at positions 1 and 2 send the gradient to position 1."""
    B, H, W, C = 2, 4, 4, 8
    a = np.zeros((B, H, W, C), np.float32)
    a[:, 0, 1, :] = 3.0                                       # window (0,0): positions (0,1) and (1,0) tie at 3, (1,1) is smaller
    a[:, 1, 0, :] = 3.0
    a[:, 1, 1, :] = 1.0
    a[:, 2, 2, :] = 2.0                                       # window (1,1): all four equal and positive -> position 0
    a[:, 2, 3, :] = a[:, 3, 2, :] = a[:, 3, 3, :] = 2.0
    df = np.arange(1, B * C + 1, dtype=np.float32).reshape(B, C)
    ad, dfd = ctx.to_device(a), ctx.to_device(df)
    out = ctx.pool_gap_bwd(ad, dfd)
    assert torch.equal(out, _pool_gap_composition(ctx, ad, dfd))
    exp = np.zeros_like(a)
    exp[:, 0, 1, :] = df / 4.0
    exp[:, 2, 2, :] = df / 4.0
    assert np.array_equal(out.cpu().numpy(), exp)


def test_pool_gap_bwd_rejects_bad_arguments(ctx):
    from sr355 import _lib as L
    a, df = ctx.empty((2, 4, 4, 8)), ctx.empty((2, 8))
    with pytest.raises(ValueError):
        ctx.pool_gap_bwd(a, ctx.empty((2, 4)))
    with pytest.raises(ValueError):
        ctx.pool_gap_bwd(a.double(), df)
    with pytest.raises(ValueError):
        ctx.pool_gap_bwd(ctx.empty((2, 1, 4, 8)), df)                                               # nothing to pool
    assert ctx.lib.sr_pool_gap_bwd(ctx.h, None, df.data_ptr(), 2, 4, 4, 8, a.data_ptr(), ctx.stream()) == L.SR_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- sr_conv2d_wgrad_maps
@pytest.mark.parametrize("chan", [(512, 512), (32, 64), (48, 40)])
@pytest.mark.parametrize("hw", [(8, 8), (4, 4), (2, 2), (8, 5)])
@pytest.mark.parametrize("B", [1, 2, 3, 4, 7])
def test_wgrad_maps_against_the_fp64_tap_sum(ctx, B, hw, chan):
    """B = 1, 2, 4, 7 leave the last packed tile partly filled at every width (3, 5, 9 and 4 images per tile at W = 8, 4, 2, 5)."""
    from test_backward_kernels_gpu import wgrad_ref
    (H, W), (cin, cout) = hw, chan
    rng = np.random.default_rng(B * 10000 + H * 1000 + W * 100 + cin)
    x, dy = rng.normal(size=(B, H, W, cin)).astype(np.float32), rng.normal(size=(B, H, W, cout)).astype(np.float32)
    xd, dyd = ctx.to_device(x), ctx.to_device(dy)
    dw, db = ctx.conv2d_wgrad_maps(xd, dyd)
    rw, rb = wgrad_ref(x, dy, 3)
    ew, eb = rel_l2(dw.cpu().numpy(), rw), rel_l2(db.cpu().numpy(), rb)
    assert ew <= 2e-6 and eb <= 2e-6, (ew, eb)
    dw2, db2 = ctx.conv2d_wgrad_maps(xd, dyd)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)


def test_wgrad_maps_exact_integers_and_out_views(ctx):
    """Small integers: every sum is exact, the result is bitwise the fp64 tap sum; written into views of a flat bucket."""
    from test_backward_kernels_gpu import wgrad_ref
    rng = np.random.default_rng(3)
    x, dy = rng.integers(-2, 3, (5, 8, 8, 40)).astype(np.float32), rng.integers(-2, 3, (5, 8, 8, 36)).astype(np.float32)
    flat = torch.zeros(9 * 40 * 36 + 36 + 4, device=ctx.torch_device)
    dw, db = flat[:9 * 40 * 36].reshape(3, 3, 40, 36), flat[9 * 40 * 36:9 * 40 * 36 + 36]
    ctx.conv2d_wgrad_maps(ctx.to_device(x), ctx.to_device(dy), out=(dw, db))
    rw, rb = wgrad_ref(x, dy, 3)
    assert np.array_equal(dw.cpu().numpy().astype(np.float64), rw) and np.array_equal(db.cpu().numpy().astype(np.float64), rb)
    assert torch.all(flat[-4:] == 0)


@pytest.mark.parametrize("W", [8, 5, 2])
def test_wgrad_maps_nothing_crosses_the_seam(ctx, W):
    """Image 0 has one non-zero dy pixel in its last column, its tile neighbour image 1 one non-zero x pixel in its first (and the other way
    round in a second run): within every image x or dy is zero, so the kernel gradient must be exactly zero."""
    H, C = 8, 32
    for first, second in ((0, 1), (1, 0)):
        x, dy = np.zeros((2, H, W, C), np.float32), np.zeros((2, H, W, C), np.float32)
        dy[first, 3, W - 1 if first == 0 else 0, :] = 1.5
        x[second, 3, 0 if first == 0 else W - 1, :] = 2.5
        dw, db = ctx.conv2d_wgrad_maps(ctx.to_device(x), ctx.to_device(dy))
        assert torch.count_nonzero(dw).item() == 0
        assert np.array_equal(db.cpu().numpy(), np.full(C, 1.5, np.float32))


def test_wgrad_maps_rejects_larger_maps(ctx):
    from sr355 import _lib as L
    with pytest.raises(ValueError):
        ctx.conv2d_wgrad_maps(ctx.empty((1, 9, 8, 32)), ctx.empty((1, 9, 8, 32)))
    x, dw, db = ctx.empty((1, 8, 9, 32)), ctx.empty((3, 3, 32, 32)), ctx.empty((32,))
    assert ctx.lib.sr_conv2d_wgrad_maps(ctx.h, x.data_ptr(), x.data_ptr(), 1, 8, 9, 32, 32, dw.data_ptr(), db.data_ptr(), ctx.stream()) == L.SR_ERR_INVALID
    assert ctx.lib.sr_conv2d_wgrad_maps(ctx.h, None, x.data_ptr(), 1, 8, 8, 32, 32, dw.data_ptr(), db.data_ptr(), ctx.stream()) == L.SR_ERR_INVALID


# ---------------------------------------------------------------------------------------------------------------- one training step
def _model(hw, n_last, **kw):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    m = FineTunedVGG16(compute_dtype="f32")
    m.setup_model(input_shape=(hw, hw, 3), num_classes=2, train_last_n_layers=n_last, fine_tune_base=True, **kw)
    return m


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_one_step_against_the_reference(ctx, case):
    from sr355.train import Adam
    from sr355.vgg_train import VGGFineTuner
    n_last, hw = case
    first, lr, l2 = R.FIRST_CONV[n_last], 1e-3, 1e-3
    layers, convs = R.tail_of(first), [n for n in R.tail_of(first) if "_conv" in n]
    m = _model(hw, n_last, dropout_rate=0.2, l2_reg=l2, learning_rate=lr)
    assert m._tail_convs() == convs
    X, y, k0, k1 = R.step_inputs(n_last, hw)
    x = m._prefix_device(ctx.to_device(X), first)
    side = hw // (16 if n_last == 4 else 8)
    assert tuple(x.shape) == (2, side, side, 512)
    tr = VGGFineTuner(ctx, m.weights, convs, lr)
    tr.collect_masks = True
    w0 = {n: (k.copy(), b.copy()) for n, (k, b) in tr.bucket.host().items()}
    stats, work = ctx.empty((3,), torch.float64), ctx.dense_head_workspace(2, 2)
    tr.step(x, ctx.to_device(y.astype(np.int32)), stats, work, ctx.to_device(k0), ctx.to_device(k1), 1.25, l2)
    acts = {n: a.cpu().numpy() for n, a in tr.last_acts.items()}
    assert list(acts) == convs
    xh = x.cpu().numpy()
    kw = dict(keep0=k0, keep1=k1, keep_scale=1.25, l2_reg=l2)
    own = R.tail_head(xh, layers, m.weights, y, **kw)
    # forward: the k-th trained conv within k x 1e-5 of the reference's own forward; branch differences capped
    for k, n in enumerate(convs, 1):
        e = rel_l2(acts[n], own["acts"][n])
        print(case, n, "forward rel-L2", e)
        assert e <= k * 1e-5, (n, e)
    relu_dev = {n: acts[n] > 0 for n in convs}
    pools = {p: layers[i - 1] for i, p in enumerate(layers) if p.endswith("_pool")}                # pool -> the conv in front of it
    sel_dev = {p: R.pool_selection(acts[c])[0] for p, c in pools.items()}
    relu_diff = sum(int(np.sum(relu_dev[n] != own["relu"][n])) for n in convs) / sum(a.size for a in acts.values())
    live = sum(int(np.sum(own["sel"][p][1])) for p in pools)
    sel_diff = sum(int(np.sum((sel_dev[p] != own["sel"][p][0]) & own["sel"][p][1])) for p in pools) / max(live, 1)
    print(case, "relu branch differences", relu_diff, "pool selection differences", sel_diff, "of", live)
    assert relu_diff <= 1e-4 and sel_diff <= 1e-3
    # loss and gradients against the reference on the device's branches
    ref = R.tail_head(xh, layers, m.weights, y, pin={"relu": relu_dev, "sel": sel_dev}, **kw)
    st = stats.cpu().numpy()
    loss = st[0] / 2 + l2 * st[2]
    print(case, "loss", loss, ref["loss"], own["loss"])
    assert abs(loss - ref["loss"]) <= 1e-5 * abs(ref["loss"]) and abs(loss - own["loss"]) <= 1e-5 * abs(own["loss"])
    gd = tr.bucket.split(tr.grads.cpu().numpy())
    # a conv's gradient has passed L convs' dgrad / wgrad kernels from the loss down to it (each held to 1e-5 / 2e-6 on its own; at worst they
    # add); the Dense layers' come from features that have passed all K convs forward (k x 1e-5 above) and the head step (1e-5)
    depth = {n: len(convs) - i for i, n in enumerate(convs)}
    depth["dense"] = depth["predictions"] = len(convs) + 1
    for n in convs + ["dense", "predictions"]:
        for s in (0, 1):
            e = rel_l2(gd[n][s], ref["grads"][n][s])
            print(case, n, "kernel" if s == 0 else "bias", "gradient rel-L2", e, "bound", depth[n] * 1e-5)
            assert e <= depth[n] * 1e-5, (n, s, e)
    # the update: DeviceAdam on the flat bucket is the host Adam on the device's own gradients, bit for bit
    host = Adam(w0, lr, epsilon=1e-7).apply(w0, {n: (a.copy(), b.copy()) for n, (a, b) in gd.items()})
    new = tr.bucket.host()
    for n in convs + ["dense", "predictions"]:
        for s in (0, 1):
            bad = int(np.sum(new[n][s] != host[n][s]))
            print(case, n, s, "Adam mismatches", bad, "of", host[n][s].size)
            assert bad == 0, (n, s, bad)
            assert not np.array_equal(new[n][s], w0[n][s])


# ---------------------------------------------------------------------------------------------------------------- fits
def _fit_model(n_last=4, lr=R.FIT["learning_rate"], dropout=0.0, **kw):
    return _model(32, n_last, dropout_rate=dropout, l2_reg=R.FIT["l2_reg"], learning_rate=lr, **kw)


def _run_fit(m, epochs=R.FIT["epochs"], **kw):
    X, y, Xv, yv = R.fit_inputs()
    return m.fit(X, y, Xv, yv, batch_size=R.FIT["batch_size"], epochs=epochs, use_augmentation=False, seed=R.FIT["seed"], **kw)


@pytest.fixture(scope="module")
def fitted(ctx):
    m = _fit_model()
    w0 = {n: (k.copy(), b.copy()) for n, (k, b) in m.weights.items()}
    return m, w0, _run_fit(m)


def test_two_epoch_fit_matches_the_reference_fit(ctx, fitted):
    m, w0, hist = fitted
    X, y, Xv, yv = R.fit_inputs()
    h64, _ = R.fit(X, y, Xv, yv, w0, dtype=torch.float64, **R.FIT)
    for k in ("loss", "accuracy", "val_loss", "val_accuracy", "lr"):
        print(k, hist.history[k], h64[k])
        assert len(hist.history[k]) == 2 and np.allclose(hist.history[k], h64[k], rtol=1e-3, atol=0), (k, hist.history[k], h64[k])


def test_fit_trains_the_tail_and_leaves_the_frozen_layers_alone(ctx, fitted):
    m, w0, hist = fitted
    trained = ["block5_conv1", "block5_conv2", "block5_conv3", "dense", "predictions"]
    assert m.trainable_layers() == trained and m.trained
    for n in w0:
        for s in (0, 1):
            if n in trained:
                assert not np.array_equal(m.weights[n][s], w0[n][s]), (n, s)
            else:
                assert np.array_equal(m.weights[n][s], w0[n][s]), (n, s)
    # the inference model has the updated convs: evaluate on the validation set reproduces the last epoch's val_loss (no early stop in 2 epochs)
    X, y, Xv, yv = R.fit_inputs()
    loss, acc = m.evaluate(Xv, yv)
    assert abs(loss - hist.history["val_loss"][-1]) <= 1e-4 * hist.history["val_loss"][-1], (loss, hist.history["val_loss"])
    assert acc == hist.history["val_accuracy"][-1]


def test_a_second_identical_fit_gives_the_same_bits(ctx, fitted):
    m, _, hist = fitted
    m2 = _fit_model()
    hist2 = _run_fit(m2)
    assert hist2.history == hist.history
    assert all(np.array_equal(m2.weights[n][s], m.weights[n][s]) for n in m.weights for s in (0, 1))


def test_fit_with_augmentation_trains_the_tail(ctx):
    """The augmented route (sr_affine_warp per batch, batches of 32) feeds the same trainer."""
    m = _fit_model()
    w0 = m.weights["block5_conv2"][0].copy()
    X, y, Xv, yv = R.fit_inputs()
    h = m.fit(X, y, Xv, yv, batch_size=4, epochs=1, use_augmentation=True, seed=1)                # the augmented route, batches of 32
    assert len(h.history["loss"]) == 1 and np.isfinite(h.history["loss"][0]) and not np.array_equal(m.weights["block5_conv2"][0], w0)


def test_one_trainable_layer_is_head_only_training(ctx):
    """train_last_n_layers=1 is block5_pool alone: no conv to train, and the fit is today's, bit for bit."""
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    X, y, Xv, yv = R.fit_inputs()
    out = []
    for fine in (True, False):
        m = FineTunedVGG16(compute_dtype="f32")
        m.setup_model(input_shape=(32, 32, 3), train_last_n_layers=1, dropout_rate=0.2, l2_reg=1e-3, fine_tune_base=fine)
        assert m.trainable_layers() == ["dense", "predictions"] and m.count_params(trainable_only=True) == 131842
        out.append((m.fit(X, y, Xv, yv, epochs=2, use_augmentation=True, seed=9), m))
    (h1, m1), (h2, m2) = out
    assert h1.history == h2.history
    assert all(np.array_equal(m1.weights[n][s], m2.weights[n][s]) for n in m1.weights for s in (0, 1))


def test_count_params_and_trainable_layers_follow_the_mode(ctx):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    b5 = ["block5_conv1", "block5_conv2", "block5_conv3"]
    head = ["dense", "predictions"]
    m = _model(32, 4)
    assert m.trainable_layers() == b5 + head and m.count_params(trainable_only=True) == 7211266 and m.count_params() == 14846530
    m = _model(32, 6, base_trainable=False)                                 # base_trainable is not consulted
    assert m.trainable_layers() == ["block4_conv3"] + b5 + head and m.count_params(trainable_only=True) == 9571074
    m = _model(32, 5)
    assert m.trainable_layers() == b5 + head
    m = _model(32, 18)
    assert m.trainable_layers() == [n for n in R.BASE if "_conv" in n] + head and m.count_params(trainable_only=True) == 14846530
    m = FineTunedVGG16()
    m.setup_model(input_shape=(32, 32, 3), train_last_n_layers=6, base_trainable=True)              # the reference's call: head-only
    assert m.trainable_layers() == head and m.count_params(trainable_only=True) == 131842


def test_early_stopping_restores_convs_and_head_of_the_best_epoch(ctx, monkeypatch):
    """lr 3e-4: the reference fit's val_loss is 6.69, 1.21, 1.85, 1.73, 1.78 -- the best epoch is the second, the three after it are worse by
    0.5, and EarlyStopping(patience 3) ends the fit after the fifth.  The test snapshots the weights the callbacks see at every epoch."""
    import sr355.train as T
    seen = []
    end_epoch = T.PlateauCallbacks.end_epoch

    def spy(self, ep, val_loss, weights):
        seen.append({n: (a.copy(), b.copy()) for n, (a, b) in weights.items()})
        return end_epoch(self, ep, val_loss, weights)

    monkeypatch.setattr(T.PlateauCallbacks, "end_epoch", spy)
    m = _fit_model(lr=3e-4)
    hist = _run_fit(m, epochs=12)
    vl = hist.history["val_loss"]
    best = int(np.argmin(vl))
    print("val_loss", vl, "lr", hist.history["lr"])
    assert len(vl) == len(seen) < 12 and len(vl) == best + 4                 # stopped, three epochs after the best one
    assert hist.history["lr"][-1] < 3e-4                                     # ReduceLROnPlateau acted on the one optimiser
    assert set(seen[best]) == set(m.trainable_layers())
    for n, (k, b) in seen[best].items():
        assert np.array_equal(m.weights[n][0], k) and np.array_equal(m.weights[n][1], b), n
        assert not np.array_equal(m.weights[n][0], seen[-1][n][0]), n        # and not the last epoch's
