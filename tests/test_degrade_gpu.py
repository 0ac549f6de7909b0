"""The dataset-synthesis stages on the device (sr_degrade_gauss / _motion / _noise / _jpeg, Context.degrade_*, data/common_methods.py) against
the NumPy restatement of tests/degrade_ref.py and, for the JPEG round trip, the codec's own outputs in tests/golden/degrade_jpeg.npz.
Every comparison is bit for bit except the kernel's fp32 normal deviates against the fp64 restatement: 1e-5 absolute, derived -- |z| <=
5.8 since u1 >= 2^-24, so 1e-5 is about 30 fp32 ulp there, room for the device's logf / sincospif / sqrtf and the final product."""
import os

import numpy as np
import pytest
import torch

import degrade_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degrade_jpeg.npz")


def image(H, W, seed, runs=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if runs:                                           # runs of 0 and 255, also across the borders the blurs reflect at
        img[:, :4] = 0
        img[:, -5:] = 255
        img[H // 2, 4:W // 2] = 255
        img[H // 2 + 1, W // 2:-5] = 0
    return img


def table(ctx, records):
    return ctx.to_device(ctx.degrade_params(records))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------- Gaussian blur
@pytest.mark.parametrize("shape", [(16, 16), (23, 37)])
def test_gauss_every_ksize_and_sigma(ctx, shape):
    cases = [(k, s) for k in (3, 5, 7) for s in (0.8, 2.0)]
    img = image(*shape, seed=11, runs=True)
    x = ctx.to_device(np.stack([img] * len(cases)))
    got = ctx.degrade_gauss(x, table(ctx, [{"gauss_ksize": k, "gauss_sigma": s} for k, s in cases])).cpu().numpy()
    for i, (k, s) in enumerate(cases):
        assert np.array_equal(got[i], R.gaussian_blur(img, R.gauss_taps(k, s))), (k, s)


def test_gauss_rows_differ_per_image_and_flag_off_copies(ctx):
    imgs = np.stack([image(37, 70, seed=20 + i) for i in range(3)])         # more than one tile both ways, no tile multiple
    recs = [{"gauss_ksize": 7, "gauss_sigma": 1.1}, {}, {"gauss_ksize": 3, "gauss_sigma": 2.0}]
    got = ctx.degrade_gauss(ctx.to_device(imgs), table(ctx, recs)).cpu().numpy()
    assert np.array_equal(got[0], R.gaussian_blur(imgs[0], R.gauss_taps(7, 1.1)))
    assert np.array_equal(got[1], imgs[1])
    assert np.array_equal(got[2], R.gaussian_blur(imgs[2], R.gauss_taps(3, 2.0)))
    alone = ctx.degrade_gauss(ctx.to_device(imgs[2:3]), table(ctx, recs[2:3])).cpu().numpy()          # any B: the same bits
    assert np.array_equal(alone[0], got[2])


# ---------------------------------------------------------------------------------------------- motion blur
@pytest.mark.parametrize("shape", [(16, 16), (37, 23)])
def test_motion_every_size(ctx, shape):
    img = image(*shape, seed=31, runs=True)
    recs = [{"motion_size": s} for s in (5, 7, 9)] + [{}]
    got = ctx.degrade_motion(ctx.to_device(np.stack([img] * 4)), table(ctx, recs)).cpu().numpy()
    for i, s in enumerate((5, 7, 9)):
        assert np.array_equal(got[i], R.motion_blur(img, s)), s
    assert np.array_equal(got[3], img)


# ---------------------------------------------------------------------------------------------- noise
def test_noise_supplied_field(ctx):
    rng = np.random.default_rng(41)
    imgs = np.stack([image(17, 23, seed=42 + i) for i in range(3)])
    field = rng.normal(0, 8.0, imgs.shape).astype(np.float32)
    recs = [{"noise_std": 8.0}, {}, {"noise_std": 8.0}]
    got = ctx.degrade_noise(ctx.to_device(imgs), table(ctx, recs), field=ctx.to_device(field)).cpu().numpy()
    assert np.array_equal(got[0], R.noise_apply(imgs[0], field[0])) and np.array_equal(got[2], R.noise_apply(imgs[2], field[2]))
    assert np.array_equal(got[1], imgs[1])


def test_noise_field_on_the_clip_and_truncation_edges(ctx):
    p = np.array([0, 0, 5, 254, 255, 255, 1, 200], np.uint8)
    n = np.array([-0.5, 0.0, -5.0, 0.999, 0.5, 0.0, -0.5, 54.999], np.float32)             # p + n: -0.5, 0, 0, 254.999, 255.5, 255, 0.5, 254.999
    want = [0, 0, 0, 254, 255, 255, 0, 254]
    img = np.zeros((16, 16, 3), np.uint8)
    f = np.zeros((16, 16, 3), np.float32)
    img.reshape(-1)[:8] = p
    f.reshape(-1)[:8] = n
    img.reshape(-1)[-8:] = p                           # and in the last, partial group of four elements' neighbourhood
    f.reshape(-1)[-8:] = n
    got = ctx.degrade_noise(ctx.to_device(img[None]), table(ctx, [{"noise_std": 1.0}]), field=ctx.to_device(f[None]))[0].cpu().numpy()
    assert got.reshape(-1)[:8].tolist() == want and got.reshape(-1)[-8:].tolist() == want
    assert np.array_equal(got, R.noise_apply(img, f))


def test_kernel_noise_against_the_philox_restatement(ctx):
    seed = 0x1234567890ABCDEF
    shape = (17, 23, 3)                                # 1173 elements: the last Philox block is partial
    imgs = np.stack([image(17, 23, seed=50 + i) for i in range(2)])
    recs = [{"noise_std": 9.5}, {"noise_std": 2.25}]
    y, z = ctx.degrade_noise(ctx.to_device(imgs), table(ctx, recs), seed=seed, raw=True)
    y, z = y.cpu().numpy(), z.cpu().numpy()
    for b in range(2):
        ref = R.philox_normal(seed, b, shape)
        err = float(np.abs(z[b].astype(np.float64) - ref).max())
        print(f"image {b}: max |z - fp64 restatement| = {err:.3e}")
        assert err <= 1e-5
        assert np.array_equal(y[b], R.noise_from_z(imgs[b], z[b], recs[b]["noise_std"]))
    assert not np.array_equal(z[0], z[1])              # two images of one batch: different fields
    y2, z2 = ctx.degrade_noise(ctx.to_device(imgs), table(ctx, recs), seed=seed, raw=True)
    assert np.array_equal(y2.cpu().numpy(), y) and np.array_equal(z2.cpu().numpy(), z)                 # the same seed: the same bits
    y3 = ctx.degrade_noise(ctx.to_device(imgs), table(ctx, recs), seed=seed + 1).cpu().numpy()
    assert not np.array_equal(y3, y)
    alone = ctx.degrade_noise(ctx.to_device(imgs[:1]), table(ctx, recs[:1]), seed=seed).cpu().numpy()
    assert np.array_equal(alone[0], y[0])


# ---------------------------------------------------------------------------------------------- JPEG round trip
def test_jpeg_every_golden_case(ctx, golden):
    qs = [int(q) for q in golden["qualities"]]
    for H, W in golden["sizes"].tolist():
        img = golden[f"in_{H}x{W}"]
        got = ctx.degrade_jpeg(ctx.to_device(np.stack([img] * len(qs))), table(ctx, [{"jpeg_quality": q} for q in qs])).cpu().numpy()
        for i, q in enumerate(qs):
            assert np.array_equal(got[i], golden[f"out_{H}x{W}_q{q}"]), ("codec", H, W, q)
            assert np.array_equal(got[i], R.jpeg_roundtrip(img, q)), ("restatement", H, W, q)


def test_jpeg_raw_outputs(ctx, golden):
    img = golden["in_17x23"]
    y, raw = ctx.degrade_jpeg(ctx.to_device(img[None]), table(ctx, [{"jpeg_quality": 49}]), raw=True)
    ref_y, ref = R.jpeg_roundtrip(img, 49, raw=True)
    assert tuple(raw["coef_y"].shape) == (1, 32, 32) and tuple(raw["cb"].shape) == (1, 16, 16)
    for k in ("coef_y", "coef_cb", "coef_cr", "y", "cb", "cr"):
        h, w = ref[k].shape
        assert np.array_equal(raw[k][0, :h, :w].cpu().numpy().astype(np.int64), ref[k].astype(np.int64)), k
    assert np.array_equal(y[0].cpu().numpy(), ref_y)


def test_jpeg_four_qualities_in_one_call_equal_four_calls(ctx):
    imgs = np.stack([image(40, 56, seed=60 + i) for i in range(4)])
    imgs[:, 10:30, 20:50] = (np.arange(30) * 8)[None, None, :, None].astype(np.uint8)
    recs = [{"jpeg_quality": 20}, {"jpeg_quality": 0}, {"jpeg_quality": 59}, {"jpeg_quality": 100}]
    x = ctx.to_device(imgs)
    got = ctx.degrade_jpeg(x, table(ctx, recs)).cpu().numpy()
    for i, r in enumerate(recs):
        alone = ctx.degrade_jpeg(x[i:i + 1].contiguous(), table(ctx, [r])).cpu().numpy()[0]
        assert np.array_equal(got[i], alone), i
        assert np.array_equal(got[i], R.jpeg_roundtrip(imgs[i], r["jpeg_quality"]) if r["jpeg_quality"] else imgs[i]), i


# ---------------------------------------------------------------------------------------------- the module
E2E_SEEDS = (3, 12, 17, 18, 28)      # chosen on the CPU from draw_degradation's records for a 32 x 48 frame; the test asserts what they cover


def test_degrade_image_end_to_end(ctx):
    from data import common_methods as M
    hr = image(32, 48, seed=70)
    hr[8:24, 8:40] = (np.arange(32) * 7)[None, :, None].astype(np.uint8)
    seen = set()
    for seed in E2E_SEEDS:
        rec = M.draw_degradation(hr.shape, 0.5, np.random.RandomState(seed))
        seen |= {("gauss", bool(rec["gauss_ksize"])), ("motion", bool(rec["motion_size"])), ("noise", rec["noise_std"] is not None),
                 ("jpeg", bool(rec["jpeg_quality"])), rec["interp_name"]}
        np.random.seed(seed)
        lr, name = M.degrade_image(hr, 0.5)
        assert name == rec["interp_name"]
        assert isinstance(lr, np.ndarray) and lr.dtype == np.uint8 and lr.shape == (16, 24, 3)
        assert np.array_equal(lr, R.degrade_with_record(hr, rec)), (seed, rec["interp_name"])
    assert seen >= {("gauss", True), ("motion", True), ("noise", True), ("jpeg", True), *R.INTERP_NAMES}
    np.random.seed(E2E_SEEDS[0])                       # a device tensor in, a device tensor out
    lr_t, _ = M.degrade_image(ctx.to_device(hr), 0.5)
    np.random.seed(E2E_SEEDS[0])
    assert isinstance(lr_t, torch.Tensor) and np.array_equal(lr_t.cpu().numpy(), M.degrade_image(hr, 0.5)[0])


def test_degrade_batch(ctx):
    from data import common_methods as M
    hr = np.stack([image(32, 48, seed=80 + i) for i in range(8)])
    lr, names = M.degrade_batch(hr, 0.5, seed=5)
    assert isinstance(lr, torch.Tensor) and lr.is_cuda and lr.dtype == torch.uint8 and tuple(lr.shape) == (8, 16, 24, 3)
    gen = np.random.default_rng(5)
    recs = [M.draw_degradation_generator(gen, (32, 48, 3), 0.5) for _ in range(8)]
    assert names == [r["interp_name"] for r in recs] and len(set(names)) > 1
    lr2, names2 = M.degrade_batch(ctx.to_device(hr), 0.5, seed=5)
    assert names2 == names and torch.equal(lr, lr2)
    assert not torch.equal(lr, M.degrade_batch(hr, 0.5, seed=6)[0])
    quiet = [b for b, r in enumerate(recs) if r["noise_std"] is None]
    assert quiet and len(quiet) < 8                    # frames without noise are the restatement chained with the draws, bit for bit
    for b in quiet:
        assert np.array_equal(lr[b].cpu().numpy(), R.degrade_with_record(hr[b], recs[b])), b


# ---------------------------------------------------------------------------------------------- guards
def test_guards(ctx):
    from data import common_methods as M
    with pytest.raises(ValueError):
        M.degrade_image(np.zeros((15, 40, 3), np.uint8))
    with pytest.raises(NotImplementedError):
        M.degrade_image(np.zeros((32, 32, 3), np.float32))
    with pytest.raises(NotImplementedError):
        ctx.degrade_gauss(ctx.to_device(np.zeros((1, 32, 32, 3), np.float32)), np.zeros((1, 16), np.int32))
    small = ctx.to_device(np.zeros((1, 15, 40, 3), np.uint8))
    for fn in (ctx.degrade_gauss, ctx.degrade_motion, ctx.degrade_noise, ctx.degrade_jpeg):
        with pytest.raises(ValueError, match="16"):
            fn(small, np.zeros((1, 16), np.int32))
    img = image(16, 20, seed=90)
    x = ctx.to_device(np.stack([img, img]))
    bad = ctx.degrade_params([{"gauss_ksize": 3, "gauss_sigma": 1.0}, {"gauss_ksize": 3, "gauss_sigma": 1.0}])
    bad[1, 0] = 4                                      # a kernel size the ABI does not take: reported through sr_last_error, the image copied
    with pytest.raises(ValueError, match="degrade_gauss.*row 1.*holds 4"):
        ctx.degrade_gauss(x, bad)
    y = ctx.degrade_gauss(x, bad, check=False)
    with pytest.raises(ValueError, match="degrade_gauss"):
        ctx.degrade_status()
    ctx.degrade_status()                               # the record is cleared once reported
    assert np.array_equal(y[1].cpu().numpy(), img) and np.array_equal(y[0].cpu().numpy(), R.gaussian_blur(img, R.gauss_taps(3, 1.0)))
    bad = ctx.degrade_params([{"jpeg_quality": 50}, {"jpeg_quality": 50}])
    bad[0, 11] = 101
    with pytest.raises(ValueError, match="degrade_jpeg.*row 0.*holds 101"):
        ctx.degrade_jpeg(x, bad)
    with pytest.raises(ValueError, match="degrade_motion"):
        ctx.degrade_motion(x, np.array([[0] * 8 + [6] + [0] * 7, [0] * 16], np.int32))
