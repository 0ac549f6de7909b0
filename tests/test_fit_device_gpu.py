"""The fits fed from device patch datasets and updated on the device (sr355/train.py fit, SRCNN / EDSR `update="device"`, ESRGAN.fit with
PatchPairs views) against the same fits from the loader's arrays with the host update, and sr_clip_by_norm_bucket against Adam.apply's clip."""
import os
import pickle

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import models as M
from sr355 import train as T
from sr355.weights import init_weights
from SRModels.loading_methods import load_dataset_as_patches

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def ulps(a, b):
    """Distance in fp32 steps between same-sign finite values."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


def weights_equal(a, b):
    return set(a) == set(b) and all(np.array_equal(bits(a[n][s]), bits(b[n][s])) for n in a for s in (0, 1))


def rel_l2_weights(a, b):
    fa = np.concatenate([np.asarray(a[n][s], np.float64).ravel() for n in b for s in (0, 1)])
    fb = np.concatenate([np.asarray(b[n][s], np.float64).ravel() for n in b for s in (0, 1)])
    return float(np.linalg.norm(fa - fb) / np.linalg.norm(fb))


# ---------------------------------------------------------------------------------------------------------------- the clip kernel
def test_clip_by_norm_bucket_against_the_host_clip(ctx):
    """Five variables of 1, 3, 1000, 4097 and 36 864 elements with norms near 0.3, 0 (all zero), 0.999, 1.001 and 50, clipnorm 1, with unused floats
    between them.  Variables at or under the bound keep their bits; a clipped variable's factor is within 1 fp32 ulp of np.float32(clipnorm / nrm64)
    and its values within 1 ulp of the host product (two fp64 sums of n <= 2^21 non-negative exact squares differ by at most n 2^-53 relative, far
    below fp32's half-ulp, so the rounded ratio moves by at most one ulp); two runs give the same bits."""
    rng = np.random.default_rng(11)
    lengths, targets, gap = (1, 3, 1000, 4097, 36864), (0.3, 0.0, 0.999, 1.001, 50.0), 5
    host = np.full(sum(lengths) + gap * (len(lengths) + 1), 7.25, np.float32)
    rows, o = [], gap
    for n, tgt in zip(lengths, targets):
        g = rng.standard_normal(n)
        host[o:o + n] = (g * (tgt / np.sqrt(np.sum(g ** 2)))).astype(np.float32) if tgt else 0.0
        rows.append((o, n))
        o += n + gap
    table = ctx.to_device(np.asarray(rows, np.int64))
    nrm = [float(np.sqrt(np.sum(host[o:o + n].astype(np.float64) ** 2))) for o, n in rows]
    assert nrm[0] < 1 and nrm[1] == 0 and 0.998 < nrm[2] < 1 < nrm[3] < 1.002 and nrm[4] > 49
    outs = []
    for _ in range(2):
        g = ctx.to_device(host.copy())
        scales = ctx.clip_by_norm_bucket(g, table, 1.0)
        outs.append((g.cpu().numpy(), scales.cpu().numpy()))
    (got, sc), (got2, sc2) = outs
    assert np.array_equal(bits(got), bits(got2)) and np.array_equal(bits(sc), bits(sc2))
    mask = np.ones(len(host), bool)
    for v, (o, n) in enumerate(rows):
        mask[o:o + n] = False
        if nrm[v] > 1.0:
            want = np.float32(1.0 / nrm[v])
            prod = host[o:o + n] * want
            ds, dv = int(ulps(sc[v:v + 1], np.array([want]))[0]), int(ulps(got[o:o + n], prod).max())
            print(f"variable {v} (n={n}, norm {nrm[v]:.6f}): factor {sc[v]!r} vs host {want!r}: {ds} ulp; values: max {dv} ulp")
            assert ds <= 1 and dv <= 1
        else:
            assert sc[v] == 1.0 and np.array_equal(bits(got[o:o + n]), bits(host[o:o + n]))
    assert np.all(got[mask] == 7.25)                                   # nothing outside the table's ranges is touched
    with pytest.raises(ValueError):
        ctx.clip_by_norm_bucket(ctx.to_device(host.copy()), table, 0.0)


# ---------------------------------------------------------------------------------------------------------------- data
@pytest.fixture(scope="module")
def srcnn_data(ctx, tmp_path_factory):
    """3 images of 40 x 52 (LR 20 x 26, resized by the loader), patch 11 / stride 7: 126 patches; 29 train (batch 4: an odd last batch), 6 val."""
    root = tmp_path_factory.mktemp("srcnn_set")
    rng = np.random.default_rng(40)
    hr_root, lr_root = str(root / "hr"), str(root / "lr")
    os.makedirs(hr_root), os.makedirs(lr_root)
    for i in range(3):
        base = rng.uniform(0, 255, (10, 13, 3))
        hr = np.clip(np.kron(base, np.ones((4, 4, 1))) + rng.normal(0, 12, (40, 52, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(hr_root, f"p{i}.png"))
        Image.fromarray(hr[::2, ::2]).save(os.path.join(lr_root, f"p{i}.png"))
    imap = str(root / "map.pkl")
    with open(imap, "wb") as fh:
        pickle.dump({"p0.png": "INTER_LINEAR", "p2.png": "INTER_AREA"}, fh)
    args = dict(mode="srcnn", patch_size=11, stride=7, interpolation_map_path=imap)
    X, Y, _, _ = load_dataset_as_patches(hr_root, lr_root, **args)
    Xd, Yd, _, _ = load_dataset_as_patches(hr_root, lr_root, on_device=True, **args)
    assert len(X) == 126 == len(Xd)
    perm = np.random.default_rng(0).permutation(len(X))
    return X, Y, Xd.ds, perm[:29], perm[29:35]


@pytest.fixture(scope="module")
def scale_data(ctx, tmp_path_factory):
    """3 pairs of 24 x 24 -> 48 x 48, patch 12 / stride 12: the 12 -> 24 patches tests/test_train_gpu.py trains EDSR and ESRGAN on; 10 train
    (batch 4: a last batch of 2), 2 val."""
    root = tmp_path_factory.mktemp("scale_set")
    rng = np.random.default_rng(41)
    hr_root, lr_root = str(root / "hr"), str(root / "lr")
    os.makedirs(hr_root), os.makedirs(lr_root)
    for i in range(3):
        base = rng.uniform(0, 255, (12, 12, 3))
        hr = np.clip(np.kron(base, np.ones((4, 4, 1))) + rng.normal(0, 10, (48, 48, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(hr).save(os.path.join(hr_root, f"q{i}.png"))
        Image.fromarray(hr[::2, ::2]).save(os.path.join(lr_root, f"q{i}.png"))
    args = dict(mode="scale", patch_size=12, stride=12, scale_factor=2)
    X, Y = load_dataset_as_patches(hr_root, lr_root, **args)
    Xd, Yd = load_dataset_as_patches(hr_root, lr_root, on_device=True, **args)
    assert X.shape == (12, 12, 12, 3) and Y.shape == (12, 24, 24, 3) and len(Xd) == 12
    perm = np.random.default_rng(1).permutation(12)
    return X, Y, Xd.ds, perm[:10], perm[10:]


def fit_args(data, on_device):
    X, Y, ds, tr, va = data
    if on_device:
        a, b = ds.subset(tr), ds.subset(va)
        return a.X, a.Y, b.X, b.Y
    return X[tr], Y[tr], X[va], Y[va]


def srcnn_fit(data, on_device, update, epochs=2):
    from SRModels.deep_learning_models.SRCNN_model import SRCNNModel
    m = SRCNNModel(update=update)
    m.setup_model(input_shape=(11, 11, 3), learning_rate=2e-3)
    hist, _, _ = m.fit(*fit_args(data, on_device), batch_size=4, epochs=epochs, shuffle=True, verbose=False)
    return m.weights, hist


def edsr_fit(data, on_device, update, epochs=2, clipnorm=None):
    from SRModels.deep_learning_models.EDSR_model import EDSR
    m = EDSR(update=update)
    if clipnorm is not None:
        m.clipnorm = clipnorm
    m.setup_model(scale_factor=2, num_res_blocks=2, learning_rate=1e-3)
    m.clip_scales_log = []
    hist, _, _ = m.fit(*fit_args(data, on_device), batch_size=4, epochs=epochs, shuffle=True, verbose=False)
    log = [s.cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s) for s in m.clip_scales_log]
    return m.weights, hist, np.stack(log)


@pytest.fixture(scope="module")
def srcnn_host_arrays(ctx, srcnn_data):
    return srcnn_fit(srcnn_data, False, "host")


@pytest.fixture(scope="module")
def edsr_host_arrays(ctx, scale_data):
    return edsr_fit(scale_data, False, "host")


# ---------------------------------------------------------------------------------------------------------------- dataset against arrays
def test_srcnn_fit_from_views_is_the_fit_from_arrays(ctx, srcnn_data, srcnn_host_arrays):
    w0, h0 = srcnn_host_arrays
    w1, h1 = srcnn_fit(srcnn_data, True, "host")
    assert len(h0.history["loss"]) == 2 and h1.history == h0.history and h1.epoch == h0.epoch and weights_equal(w1, w0)
    X, Y, ds, tr, va = srcnn_data
    from SRModels.deep_learning_models.SRCNN_model import SRCNNModel
    m = SRCNNModel()
    m.setup_model(input_shape=(11, 11, 3))
    for args in ((ds.X, Y[tr], X[va], Y[va]), (ds.subset(tr).X, ds.subset(tr).Y, X[va], Y[va]), (X[tr], Y[tr], ds.X, ds.subset(va).Y)):
        with pytest.raises(ValueError, match="view"):                    # a view with an array; two subsets of one dataset are two datasets
            m.fit(*args, epochs=1, verbose=False)


def test_srcnn_device_update_is_the_host_update_bit_for_bit(ctx, srcnn_data, srcnn_host_arrays):
    """The same kernels on the same numbers, DeviceAdam bit-equal to Adam by its own contract, the epoch sums in the same host arithmetic: final
    weights and History are the same bits, from arrays and from views."""
    w0, h0 = srcnn_host_arrays
    for on_device in (False, True):
        w1, h1 = srcnn_fit(srcnn_data, on_device, "device")
        assert h1.history == h0.history and h1.epoch == h0.epoch, on_device
        assert weights_equal(w1, w0), on_device


def test_edsr_fit_from_views_is_the_fit_from_arrays(ctx, scale_data, edsr_host_arrays):
    w0, h0, s0 = edsr_host_arrays
    w1, h1, s1 = edsr_fit(scale_data, True, "host")
    assert h1.history == h0.history and weights_equal(w1, w0) and np.array_equal(bits(s0), bits(s1))


# EDSR device against host, measured once on an MI355X at this test's sizes (2 epochs x 3 steps, 16 variables): every clip factor agreed with the
# host's bit for bit -- none of 96 clipping at clipnorm 1, 96 of 96 at clipnorm 1e-3 -- and weights rel-L2 and history difference were 0 in all four
# runs.  No disagreeing run exists to take ten times of, so the bars of the fallback branch are the ceiling.
EDSR_DEVICE_WEIGHTS_REL_L2_BAR = 1e-5
EDSR_DEVICE_HISTORY_REL_BAR = 1e-5


def test_edsr_device_update_against_the_host_update(ctx, scale_data, edsr_host_arrays):
    """Both modes log every step's clip factors.  Where all of them agree bit for bit the weights and the history must be the same bits (the
    reasoning of the SRCNN test).  Otherwise -- a device factor one fp32 ulp from the host's, because the fp64 norm is summed in another order --
    the final weights are compared by rel-L2 and the history by relative difference against host mode, at 10 x the value measured once on the
    GPU and at most 1e-5.  At the reference's clipnorm of 1 these small fits may clip nothing, so the comparison runs a second time at
    clipnorm 1e-3, where the clip certainly acts."""
    for clipnorm, host in ((1.0, edsr_host_arrays), (1e-3, edsr_fit(scale_data, False, "host", clipnorm=1e-3))):
        w0, h0, s0 = host
        for on_device in (False, True):
            w1, h1, s1 = edsr_fit(scale_data, on_device, "device", clipnorm=clipnorm)
            assert s1.shape == s0.shape and s0.shape[0] == 6
            n_clipped, worst = int(np.sum(s0 < 1)), int(ulps(s1, s0).max())
            rel_w = rel_l2_weights(w1, w0)
            rel_h = max(abs(a - b) / max(abs(b), 1e-30) for k in h0.history for a, b in zip(h1.history[k], h0.history[k]))
            print(f"clipnorm={clipnorm} views={on_device}: {n_clipped} of {s0.size} factors clip; worst factor distance {worst} ulp; "
                  f"weights rel-L2 {rel_w:.3e}; history rel {rel_h:.3e}")
            assert worst <= 1
            if clipnorm < 1:
                assert n_clipped > s0.size // 4                           # the clip is exercised
            if worst == 0:
                assert weights_equal(w1, w0) and h1.history == h0.history
            else:
                assert rel_w <= EDSR_DEVICE_WEIGHTS_REL_L2_BAR and rel_h <= EDSR_DEVICE_HISTORY_REL_BAR


def test_esrgan_fit_from_views_is_the_fit_from_arrays(ctx, scale_data):
    """x2, growth 8, one RRDB, 3 steps (10 patches in batches of 4) and a validation batch: the epoch record, the generator and the
    discriminator are the same bits whether the batches are indexed on the host and normalised by `norm`, or cut on the device with mul = 2,
    add = -1 and brought back to [0,1] by to01."""
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    dw = init_weights(M.discriminator_layers(), seed=5000)
    vw = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=6000)
    vw = {n: (k * 0.05 if n == "block1_conv1" else k, b) for n, (k, b) in vw.items()}
    runs = []
    for on_device in (False, True):
        m = ESRGAN(compute_dtype="f32")
        m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1, use_attention=True)
        m.set_loss_network_weights(discriminator=dw, vgg19=vw)
        Xt, Yt, Xv, Yv = fit_args(scale_data, on_device)
        losses, _, _ = m.fit(Xt, Yt, X_val=Xv, Y_val=Yv, epochs=1, batch_size=4, shuffle_seed=42)
        runs.append((losses, m.weights, m.d_weights))
    (l0, g0, d0), (l1, g1, d1) = runs
    assert len(l0["g_loss"]) == 3 and l1 == l0
    assert weights_equal(g1, g0) and weights_equal(d1, d0)
    X, Y, ds, tr, va = scale_data
    m = ESRGAN(compute_dtype="f32")
    m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1, use_attention=True)
    with pytest.raises(ValueError, match="view"):
        m.fit(ds.X, Y, epochs=1)


# ---------------------------------------------------------------------------------------------------------------- callbacks
def test_callbacks_behave_in_device_mode_as_in_host_mode(ctx, srcnn_data):
    """A contrived run: the validation prediction is pushed 10 further off at every epoch, so val_loss rises from the second epoch on.  With
    lr_patience 1 and es_patience 3, ReduceLROnPlateau halves the rate at the end of epochs 2, 3 and 4 and EarlyStopping stops after epoch 4,
    restoring the first epoch's weights -- in both modes: the same learning rates, the same stopped epoch, the same restored weights, which
    are those of a one-epoch fit."""
    from SRModels.deep_learning_models.SRCNN_model import SRCNNModel
    X, Y, ds, tr, va = srcnn_data
    tr = tr[:9]

    def run(update, epochs, views):
        m = SRCNNModel()
        m.setup_model(input_shape=(11, 11, 3))
        calls = [0]

        def predict(c, w, x):
            calls[0] += 1
            return m._predict_with(c, w, x) + 10.0 * (calls[0] - 1)     # one validation batch per epoch: val_loss ~ 100 k^2 at epoch k
        if update == "device":
            start = T.ParamBucket(ctx, m.weights)
            opt = T.DeviceAdam(ctx, start.flat, learning_rate=1e-3)
        else:
            start, opt = m.weights, T.Adam(m.weights, learning_rate=1e-3)
        dtr, dva = ds.subset(tr), ds.subset(va)
        data = (dtr.X, dtr.Y, dva.X, dva.Y) if views else (X[tr], Y[tr], X[va], Y[va])
        w, hist, _, _ = T.fit(ctx, start, T.srcnn_loss_and_grads, predict, opt, *data, batch_size=4, epochs=epochs, es_patience=3, lr_patience=1,
                              shuffle=True, verbose=False)
        return w, hist, opt.lr

    w_h, h_h, lr_h = run("host", 8, False)
    w_d, h_d, lr_d = run("device", 8, True)
    assert h_h.epoch == [0, 1, 2, 3] == h_d.epoch                                   # stopped after the fourth epoch
    assert h_h.history["lr"] == [1e-3, 1e-3, 5e-4, 2.5e-4] == h_d.history["lr"] and lr_h == lr_d == 1.25e-4
    assert h_d.history == h_h.history and weights_equal(w_d, w_h)
    w_1, _, _ = run("host", 1, False)
    assert weights_equal(w_h, w_1)                                                  # restore_best_weights: the first epoch's
