"""The classical study's back-projection, NL-means, edge-guided and frequency up-scalers (classic_algorithms.py:23-108) on the device
against the NumPy restatements of tests/classic_ref.py, on uint8 grayscale images from sr355.synth plus Gaussian noise."""
import numpy as np
import pytest
import torch

import classic_ref as CR

pytestmark = pytest.mark.gpu

# (H, W, h, w): the dataset's 478 / 239, an exact 2x, a 4x (a plain linear shrink in IBP), a non-integer ratio
SIZES = [(478, 478, 239, 239), (48, 48, 24, 24), (96, 96, 24, 24), (70, 50, 33, 24)]


def gray_pair(H, W, h, w, seed, noise=6.0):
    from sr355.synth import hr_tile
    rng = np.random.default_rng(seed)
    hr = hr_tile(rng, H, W)[:, :, 0].astype(np.float64) * 255.0
    hr = np.clip(hr + rng.normal(0, noise, hr.shape), 0, 255).astype(np.uint8)
    lr = np.clip(np.asarray(CR.O.cv_resize(hr.astype(np.float32)[:, :, None], h, w, CR.O.INTER_AREA))[:, :, 0] + rng.normal(0, noise, (h, w)),
                 0, 255).astype(np.uint8)
    return hr, lr


def dev(ctx, *arrs):
    return ctx.to_device(np.stack(arrs), torch.uint8)


def assert_u8_close(got, ref):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    assert d.max() <= 1 and np.mean(d == 0) >= 0.999, (d.max(), np.mean(d == 0))


@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_back_projection(ctx, H, W, h, w):
    hr, lr = gray_pair(H, W, h, w, seed=H + w)
    y, est = ctx.back_projection(dev(ctx, hr), dev(ctx, lr), 10, raw=True)
    ref_u8, ref_est = CR.back_projection(hr, lr, 10)
    assert np.max(np.abs(est[0].cpu().numpy() - ref_est)) <= 1e-3
    assert_u8_close(y[0].cpu().numpy(), ref_u8)


def test_back_projection_zero_iterations_is_the_first_argument(ctx):
    hr, lr = gray_pair(48, 48, 24, 24, seed=4)
    assert np.array_equal(ctx.back_projection(dev(ctx, hr), dev(ctx, lr), 0)[0].cpu().numpy(), hr)


@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_non_local_means(ctx, H, W, h, w):
    _, lr = gray_pair(H, W, h, w, seed=7 * H + w)
    up, den, sigma = ctx.non_local_means(dev(ctx, lr), H, W, raw=True)
    ref_up, ref_den, ref_sigma = CR.non_local_means((H, W), lr)
    assert abs(float(sigma[0]) - ref_sigma) <= 1e-12 * ref_sigma
    assert np.max(np.abs(den[0].cpu().numpy() - ref_den)) <= 1e-5
    assert np.max(np.abs(up[0].cpu().numpy() - ref_up)) <= 2e-5


def test_noise_sigma_odd_and_even_counts(ctx):
    imgs = [gray_pair(48, 50, 24, 25, seed=s)[1] for s in range(3)] + [gray_pair(52, 54, 26, 27, seed=9)[1][:24, :25]]
    sig = ctx.noise_sigma(dev(ctx, *imgs)).cpu().numpy()
    for s, im in zip(sig, imgs):
        assert abs(s - CR.noise_sigma(im)) <= 1e-12 * CR.noise_sigma(im)


def test_non_local_means_flat_image_raises(ctx):
    flat = np.full((24, 24), 93, np.uint8)
    assert np.isnan(float(ctx.noise_sigma(dev(ctx, flat))[0]))
    with pytest.raises(ValueError):
        ctx.non_local_means(dev(ctx, flat), 48, 48)


@pytest.mark.parametrize("H,W,h,w", SIZES)
def test_edge_guided(ctx, H, W, h, w):
    _, lr = gray_pair(H, W, h, w, seed=3 * H + w)
    y, up_e = ctx.edge_guided(dev(ctx, lr), H, W, raw=True)
    ref_u8, ref_up_e = CR.edge_guided(lr, H, W)
    assert np.max(np.abs(up_e[0].cpu().numpy() - ref_up_e)) <= 1e-4
    assert_u8_close(y[0].cpu().numpy(), ref_u8)


@pytest.mark.parametrize("H,W,h,w", SIZES + [(50, 61, 25, 30), (48, 49, 24, 25)])
def test_freq_extrapolate(ctx, H, W, h, w):
    _, lr = gray_pair(H, W, h, w, seed=H * W)
    got = ctx.freq_extrapolate(dev(ctx, lr), H, W)[0].cpu().numpy()
    ref = CR.freq_extrapolate(lr, H, W)
    assert got.dtype == np.float64 and np.max(np.abs(got - ref)) <= 1e-9 * np.max(ref)


def test_batch_equals_single_calls(ctx):
    pairs = [gray_pair(70, 50, 33, 24, seed=s) for s in range(4)]
    hr = dev(ctx, *[p[0] for p in pairs])
    lr = dev(ctx, *[p[1] for p in pairs])
    batched = {
        "ibp": ctx.back_projection(hr, lr, 10),
        "nlm": ctx.non_local_means(lr, 70, 50),
        "egi": ctx.edge_guided(lr, 70, 50),
        "freq": ctx.freq_extrapolate(lr, 70, 50),
    }
    for i in range(4):
        hr1, lr1 = hr[i:i + 1].contiguous(), lr[i:i + 1].contiguous()
        single = {
            "ibp": ctx.back_projection(hr1, lr1, 10),
            "nlm": ctx.non_local_means(lr1, 70, 50),
            "egi": ctx.edge_guided(lr1, 70, 50),
            "freq": ctx.freq_extrapolate(lr1, 70, 50),
        }
        for k in batched:
            assert torch.equal(batched[k][i], single[k][0]), k


def test_invalid_shapes_are_refused(ctx):
    _, lr = gray_pair(48, 48, 24, 24, seed=1)
    x = dev(ctx, lr)
    with pytest.raises(ValueError):
        ctx.freq_extrapolate(x, 12, 48)
    with pytest.raises(ValueError):
        ctx.edge_guided(x, 48, 12)
    with pytest.raises(ValueError):
        ctx.back_projection(x, dev(ctx, np.zeros((48, 48), np.uint8)))
    with pytest.raises(ValueError):
        ctx.freq_extrapolate(x.float(), 48, 48)
    with pytest.raises(ValueError):
        ctx.non_local_means(x, 48, 48, patch_size=4)


def test_reference_shaped_wrappers(ctx):
    from SRModels.classic_super_resolution_algorithms import classic_algorithms as CA
    hr, lr = gray_pair(70, 50, 33, 24, seed=11)
    out = CA.back_projection(hr, lr)
    assert out.shape == hr.shape and out.dtype == np.uint8
    assert np.array_equal(out, CR.back_projection(hr, lr, 10)[0]) or np.max(np.abs(out.astype(int) - CR.back_projection(hr, lr, 10)[0])) <= 1
    out = CA.non_local_means(hr, lr)
    assert out.shape == hr.shape and out.dtype == np.float64
    assert np.max(np.abs(out - CR.non_local_means(hr.shape, lr)[0])) <= 2e-5
    out = CA.edge_guided_interpolation(hr, lr)
    assert out.shape == hr.shape and out.dtype == np.uint8
    out = CA.frequency_extrapolation(hr, lr)
    assert out.shape == hr.shape and out.dtype == np.float64
    assert np.max(np.abs(out - CR.freq_extrapolate_fft(lr, 70, 50))) <= 1e-9 * np.max(out)
    rgb = np.stack([lr] * 3, axis=-1)
    for fn in (CA.back_projection, CA.non_local_means, CA.edge_guided_interpolation, CA.frequency_extrapolation):
        with pytest.raises(NotImplementedError):
            fn(np.stack([hr] * 3, axis=-1), rgb)
