"""The classical study's scoring without a GPU: the NumPy restatement behind the device tests (tests/metrics_ref.py) against independent
forms of each score (np.fft, scipy.ndimage, np.histogram, a direct loop), the host helpers of SRModels' profiling_methods (bootstrap,
summary, ranking) against hand-computed values, and the C ABI export of the device scores."""
import math
import os

import numpy as np
import pytest

import metrics_ref as MR


def pm():
    from SRModels.classic_super_resolution_algorithms import profiling_methods
    return profiling_methods


def rand_u8(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


# ------------------------------------------------------------------ the restatement against independent forms
@pytest.mark.parametrize("H,W", [(478, 478), (48, 48), (70, 53), (7, 7), (9, 16)])
def test_hf_ratio_matches_fft2_fftshift(H, W):
    hr, sr = rand_u8((H, W), H), rand_u8((H, W), W + 1)
    for frac in (0.6, 0.3):
        F = [np.fft.fftshift(np.fft.fft2(x.astype(np.float64))) for x in (hr, sr)]
        Y, X = np.ogrid[:H, :W]
        r = np.sqrt((Y - H // 2) ** 2 + (X - W // 2) ** 2)
        mask = r > frac * (r.max() + 1e-9)
        want = (np.abs(F[1])[mask].sum() + 1e-9) / (np.abs(F[0])[mask].sum() + 1e-9)
        assert abs(MR.hf_ratio(hr, sr, frac) - want) <= 1e-11 * want


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_ssim_matches_uniform_filter(dtype):
    ndi = pytest.importorskip("scipy.ndimage")
    a, b = rand_u8((40, 33), 1), rand_u8((40, 33), 2)
    dr = 255.0
    if dtype == "f32":
        a, b, dr = a.astype(np.float32) / 255, b.astype(np.float32) / 255, 1.0
    x, y = a.astype(np.float64), b.astype(np.float64)
    f = lambda v: ndi.uniform_filter(v, size=7)
    ux, uy = f(x), f(y)
    cn = 49 / 48
    vx, vy, vxy = cn * (f(x * x) - ux * ux), cn * (f(y * y) - uy * uy), cn * (f(x * y) - ux * uy)
    C1, C2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    assert np.max(np.abs(MR.ssim_map(a, b, dr) - S[3:-3, 3:-3])) <= 1e-10
    assert abs(MR.ssim(a, b, dr) - S[3:-3, 3:-3].mean()) <= 1e-12


def test_ssim_rgb_is_the_mean_of_channel_means():
    a, b = rand_u8((20, 21, 3), 3), rand_u8((20, 21, 3), 4)
    want = np.mean([MR.ssim(a[..., c], b[..., c], 255.0) for c in range(3)])
    assert MR.ssim(a, b, 255.0) == pytest.approx(want, abs=1e-15)


def test_sobel_matches_scipy_mirror():
    ndi = pytest.importorskip("scipy.ndimage")
    x = rand_u8((17, 23), 5)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], np.float64)
    g = x.astype(np.float32) / np.float32(255)
    gx, gy = ndi.correlate(g.astype(np.float64), kx, mode="mirror"), ndi.correlate(g.astype(np.float64), kx.T, mode="mirror")
    assert np.max(np.abs(MR.sobel_mag(x) - np.hypot(gx, gy))) <= 1e-12


def test_max_rule_scales_each_image_by_its_own_max():
    """_ensure_gray_f32: divide by 255 only when the image's own max > 1.5 -- restated by a direct float64 loop."""
    def direct(img):
        g = img.astype(np.float32)
        m = -math.inf
        for v in g.reshape(-1):
            m = max(m, float(v))
        return (g / np.float32(255) if m > 1.5 else g).astype(np.float64)
    u8 = rand_u8((9, 9), 6)
    binary = (rand_u8((9, 9), 7) > 128).astype(np.uint8)           # uint8 with max 1: not rescaled
    unit = np.random.default_rng(8).random((9, 9)).astype(np.float32)
    two = np.full((9, 9), 1.5, np.float32)
    two[0, 0] = 1.5000001
    for img in (u8, binary, unit, two, np.full((9, 9), 1.5, np.float32)):
        assert np.array_equal(MR.ensure_gray(img), direct(img))
    assert MR.ensure_gray(binary).max() == 1.0 and MR.ensure_gray(unit).max() <= 1.0


def test_rgb2gray_fixed_point():
    x = np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 255, 0], [0, 0, 255], [10, 200, 30]]], np.uint8)
    y = MR.rgb2gray_u8(x)[0]
    assert y.tolist() == [255, 0, (4899 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14, (1868 * 255 + 8192) >> 14,
                          (4899 * 10 + 9617 * 200 + 1868 * 30 + 8192) >> 14]
    assert 4899 + 9617 + 1868 == 1 << 14
    with pytest.raises(NotImplementedError):
        MR.gray_of(x.astype(np.float32))


def test_uint8_bins():
    assert np.array_equal(MR.u8_bin_lut(256), np.arange(256))
    assert np.array_equal(MR.u8_bin_lut(64), np.arange(256) // 4)


@pytest.mark.parametrize("bins", [256, 64])
def test_hist_counts_match_np_histogram(bins):
    rng = np.random.default_rng(bins)
    edges = np.arange(bins + 1) * (255.0 / bins) / 255.0
    f = np.concatenate([rng.random(5000), edges, np.nextafter(edges, 2), np.nextafter(edges, -1), [-0.5, 1.5, 0.0, 1.0]]).astype(np.float32)
    u = rand_u8(3000, 9)
    for img in (f, u):
        want = np.histogram(MR.hist_values(img), bins=bins, range=(0, 255))[0]
        assert np.array_equal(MR.hist_counts(img, bins), want)


def test_kl_forms_match_np_histogram_density():
    def kl(p, q, bins):
        P = np.histogram(MR.hist_values(p), bins=bins, range=(0, 255), density=True)[0] + 1e-12
        Q = np.histogram(MR.hist_values(q), bins=bins, range=(0, 255), density=True)[0] + 1e-12
        return float(np.sum(P * np.log(P / Q)))
    hr = rand_u8((30, 31, 3), 10)
    sr = rand_u8((30, 31, 3), 11)
    srf = np.random.default_rng(12).random((30, 31)).astype(np.float32)
    g = MR.rgb2gray_u8(hr)
    assert MR.kl_luma(hr, sr) == pytest.approx(kl(g, MR.rgb2gray_u8(sr), 256), rel=1e-12)
    assert MR.kl_luma(g, srf) == pytest.approx(kl(g, srf, 256), rel=1e-12)
    want_c = sum(kl(hr[..., c], sr[..., c], 64) for c in range(3)) / 3
    assert MR.kl_color(hr, sr) == pytest.approx(want_c, rel=1e-12)
    assert math.isnan(MR.kl_color(g, g))
    assert MR.kl_luma(hr, hr) == 0.0


def test_scores_identical_and_constant_images():
    x = rand_u8((16, 18), 13)
    s = dict(zip(MR.NAMES, MR.scores(x, x)))
    assert s["psnr"] == math.inf and s["ssim"] == 1.0 and s["kl_luma"] == 0.0 and s["epi"] == 1.0 and s["grad_mse"] == 0.0
    c = np.full((16, 18), 77, np.uint8)
    assert dict(zip(MR.NAMES, MR.scores(c, x)))["epi"] > 1 and dict(zip(MR.NAMES, MR.scores(x, c)))["epi"] < 1
    assert dict(zip(MR.NAMES, MR.scores(c, c)))["epi"] == 1.0


# ------------------------------------------------------------------ profiling_methods' host helpers
def test_module_imports_without_a_device_and_refuses_unsupported_cases():
    P = pm()
    assert P.DEF_EPS == 1e-9
    assert P.MAXIMIZE_DEFAULT == ['psnr_mean', 'ssim_mean']
    assert P.MINIMIZE_DEFAULT == ['time_mean', 'memory_mean', 'mae_mean', 'rmse_mean']
    f = np.zeros((8, 8, 3), np.float32)
    for fn in (P.gradient_mse, P.epi):
        with pytest.raises(NotImplementedError, match="float RGB"):
            fn(f, f)
    with pytest.raises(NotImplementedError, match="float RGB"):
        P.sobel_mag(f)
    with pytest.raises(NotImplementedError):
        P.kl_divergence(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), bins=128)
    with pytest.raises(NotImplementedError):
        P.structural_similarity(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8), data_range=255, win_size=5)


def test_time_and_memory_algorithm():
    P = pm()
    out, t = P.time_algorithm(lambda a, b=0: a + b, 2, b=3)
    assert out == 5 and t >= 0.0
    out, peak = P.memory_algorithm(lambda n: bytearray(n), 1 << 20)
    assert len(out) == 1 << 20 and peak >= 1 << 20


def test_bootstrap_ci_matches_integers_resampling():
    P = pm()
    vals = [31.2, 29.8, 33.1, 30.4, 28.9, 32.2, 30.0]
    rng = np.random.default_rng(42)
    v = np.array(vals)
    means = [v[rng.integers(0, len(v), size=len(v))].mean() for _ in range(1000)]
    assert P.bootstrap_ci(vals) == (float(np.percentile(means, 2.5)), float(np.percentile(means, 97.5)))
    rng = np.random.default_rng(7)
    means = [v[rng.integers(0, len(v), size=len(v))].mean() for _ in range(200)]
    assert P.bootstrap_ci(vals, n_boot=200, ci=0.9, seed=7) == (float(np.percentile(means, 5.0)), float(np.percentile(means, 95.0)))
    lo, hi = P.bootstrap_ci([1.0])
    assert math.isnan(lo) and math.isnan(hi)


def test_compute_summary_stats():
    P = pm()
    s = P.compute_summary_stats([1.0, 2.0, 4.0])
    assert s == {'mean': 7 / 3, 'median': 2.0, 'max': 4.0, 'std': float(np.std([1, 2, 4], ddof=1)), 'var': float(np.var([1, 2, 4], ddof=1)),
                 'count': 3}
    assert P.compute_summary_stats([5.0]) == {'mean': 5.0, 'median': 5.0, 'max': 5.0, 'std': 0.0, 'var': 0.0, 'count': 1}
    n = P.compute_summary_stats([np.nan, np.nan])
    assert math.isnan(n['mean']) and math.isnan(n['max']) and math.isnan(n['var']) and n['count'] == 2


SUMMARY_KEYS = {'psnr_mean', 'psnr_var', 'psnr_max', 'psnr_ci_low', 'psnr_ci_high', 'ssim_mean', 'ssim_var', 'ssim_max', 'ssim_ci_low',
                'ssim_ci_high', 'time_mean', 'time_max', 'time_jitter', 'time_var', 'memory_mean', 'memory_max', 'memory_var', 'mae_mean',
                'mae_max', 'rmse_mean', 'rmse_max', 'grad_mse_mean', 'epi_mean', 'hf_ratio_mean', 'kl_luma_mean', 'kl_color_mean'}


def test_build_metrics_summary():
    P = pm()
    algs = ('bilinear', 'nlm')
    t = {'bilinear': [0.5, 1.5], 'nlm': [2.0]}
    m = {'bilinear': [100, 300], 'nlm': [50]}
    psnr = {'bilinear': [30.0, 32.0], 'nlm': [28.0]}
    ssim = {'bilinear': [0.8, 0.9], 'nlm': [0.7]}
    one = lambda a, b: {'bilinear': [a, b], 'nlm': [a]}
    stats = dict(mae_stats=one(3.0, 5.0), rmse_stats=one(4.0, 6.0), gradient_mse_stats=one(0.1, 0.3), epi_stats=one(0.9, 1.1),
                 hf_energy_ratio_stats=one(0.5, 0.7), kl_luma_stats=one(0.01, 0.03), kl_color_stats={'bilinear': [0.2, 0.4], 'nlm': [np.nan]})
    before = {k: {a: list(v) for a, v in d.items()} for k, d in stats.items()}
    s = P.build_metrics_summary(t, m, psnr, ssim, **stats)
    assert {k: {a: list(v) for a, v in d.items()} for k, d in stats.items()} == before
    assert set(s) == set(algs) and all(set(s[a]) == SUMMARY_KEYS for a in algs)
    b = s['bilinear']
    assert b['psnr_mean'] == 31.0 and b['psnr_var'] == 2.0 and b['psnr_max'] == 32.0
    assert (b['psnr_ci_low'], b['psnr_ci_high']) == P.bootstrap_ci([30.0, 32.0])
    assert b['time_mean'] == 1.0 and b['time_max'] == 1.5 and b['time_var'] == 0.5
    assert b['time_jitter'] == pytest.approx(math.sqrt(0.5) / 1.0, rel=1e-15)
    assert b['memory_mean'] == 200.0 and b['memory_max'] == 300.0 and b['memory_var'] == 20000.0
    assert b['mae_mean'] == 4.0 and b['mae_max'] == 5.0 and b['rmse_mean'] == 5.0 and b['rmse_max'] == 6.0
    assert b['grad_mse_mean'] == pytest.approx(0.2) and b['epi_mean'] == 1.0 and b['hf_ratio_mean'] == pytest.approx(0.6)
    assert b['kl_luma_mean'] == pytest.approx(0.02) and b['kl_color_mean'] == pytest.approx(0.3)
    n = s['nlm']
    assert n['psnr_mean'] == 28.0 and n['psnr_var'] == 0.0 and n['ssim_max'] == 0.7
    for k in ('psnr_ci_low', 'psnr_ci_high', 'ssim_ci_low', 'ssim_ci_high', 'time_jitter', 'time_var', 'memory_var', 'kl_color_mean'):
        assert math.isnan(n[k]), k


def three_algs():
    return {
        'a': {'psnr_mean': 30.0, 'ssim_mean': 0.9, 'time_mean': 1.0, 'epi_mean': 1.0, 'hf_ratio_mean': 0.5},
        'b': {'psnr_mean': 20.0, 'ssim_mean': 0.8, 'time_mean': 3.0, 'epi_mean': 0.5, 'hf_ratio_mean': 1.0},
        'c': {'psnr_mean': 25.0, 'ssim_mean': np.nan, 'time_mean': 2.0, 'epi_mean': 1.25, 'hf_ratio_mean': np.nan},
    }


def test_rank_algorithms_explicit_lists():
    P = pm()
    ranked, scores, bounds = P.rank_algorithms(three_algs(), maximize=['psnr_mean', 'ssim_mean'], minimize=['time_mean'],
                                               weights={'psnr_mean': 0.5, 'ssim_mean': 0.25, 'time_mean': 0.25})
    # psnr: a 1, b 0, c 0.5;  ssim: a 1, b 0, c NaN -> 0;  time: a 1, b 0, c 0.5
    assert scores == {'a': 1.0, 'b': 0.0, 'c': 0.5 * 0.5 + 0.25 * 0.5}
    assert [k for k, _ in ranked] == ['a', 'c', 'b']
    assert bounds == {'psnr_mean': (20.0, 30.0), 'ssim_mean': (0.8, 0.9), 'time_mean': (1.0, 3.0)}
    _, eq, _ = P.rank_algorithms(three_algs(), maximize=['psnr_mean'], minimize=None)
    assert eq == {'a': 1.0, 'b': 0.0, 'c': 0.5}


def test_rank_algorithms_default_lists():
    P = pm()
    ranked, scores, bounds = P.rank_algorithms(three_algs())
    # metrics: psnr_mean, ssim_mean (max); time_mean, epi_dev, hf_ratio_dev (min); weight 1/5 each
    assert list(bounds) == ['psnr_mean', 'ssim_mean', 'time_mean', 'epi_dev', 'hf_ratio_dev']
    assert bounds['epi_dev'] == (0.0, 0.5) and bounds['hf_ratio_dev'] == (0.0, 0.5)
    w = 1 / 5
    assert scores['a'] == pytest.approx(w * (1 + 1 + 1 + 1 + 0))
    assert scores['b'] == pytest.approx(w * (0 + 0 + 0 + 0 + 1))
    assert scores['c'] == pytest.approx(w * (0.5 + 0 + 0.5 + 0.5 + 0))
    assert [k for k, _ in ranked] == ['a', 'c', 'b']


# ------------------------------------------------------------------ the C ABI
def test_library_exports_classic_scores():
    from sr355 import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = _lib.load()
    assert hasattr(lib, "sr_classic_scores")
    assert "sr_classic_scores" in _lib.SIGNATURES
    assert _lib.SCORE_NAMES == MR.NAMES
