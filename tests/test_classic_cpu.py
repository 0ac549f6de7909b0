"""The NumPy restatements behind the classical-baseline GPU tests (tests/classic_ref.py) agree with independent formulations of the same
algorithms, and the new C ABI entries refuse a missing context without touching anything (no GPU needed)."""
import numpy as np
import pytest

import classic_ref as CR


@pytest.mark.parametrize("h,w,H,W", [(24, 24, 48, 48), (24, 24, 96, 96), (25, 30, 50, 61), (33, 24, 70, 50), (7, 9, 7, 12), (31, 17, 62, 34)])
def test_freq_operator_matches_fft_zero_padding(h, w, H, W):
    x = np.random.default_rng(h * 100 + w).integers(0, 256, (h, w)).astype(np.uint8)
    ref = CR.freq_extrapolate_fft(x, H, W)
    got = CR.freq_extrapolate(x, H, W)
    assert np.max(np.abs(got - ref)) <= 1e-12 * np.max(ref)


def test_freq_operator_is_real_for_odd_sizes():
    assert np.max(np.abs(CR.dft_operator(478, 239).imag)) < 1e-12
    assert np.max(np.abs(CR.dft_operator(48, 24).imag)) > 1e-3


@pytest.mark.parametrize("h,w,seed", [(12, 15, 0), (20, 20, 1), (9, 14, 2)])
def test_nlm_gather_matches_the_pair_loop(h, w, seed):
    rng = np.random.default_rng(seed)
    x = np.clip(rng.normal(120, 40, (h, w)), 0, 255).astype(np.uint8)
    for hval in (0.05, 0.2, 3.0):            # cutoff active, partly active, every weight in
        a = CR.nl_means(x, hval)
        b = CR.nl_means_pairloop(x, hval)
        assert np.max(np.abs(a - b)) <= 1e-12, hval


def test_sobel_matches_scipy_mirror():
    ndi = pytest.importorskip("scipy.ndimage")
    x = np.random.default_rng(3).integers(0, 256, (17, 23)).astype(np.uint8)
    _, gx, gy = CR.sobel_mag(x)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    xi = x.astype(np.int64)
    assert np.array_equal(gx, ndi.correlate(xi, kx, mode="mirror"))
    assert np.array_equal(gy, ndi.correlate(xi, kx.T, mode="mirror"))


def _dwt_hi_direct(v, taps):
    """pywt's downsampling convolution of a 1-D signal: symmetric-pad, full convolution with the filter, keep every second sample
    starting at index 1 of the unpadded signal."""
    n, F = len(v), len(taps)
    ve = np.pad(v, F - 1, mode="symmetric")
    full = np.convolve(ve, taps)
    return full[np.arange((n + F - 1) // 2) * 2 + 1 + (F - 1)]


@pytest.mark.parametrize("h,w", [(24, 24), (25, 30), (239, 239), (7, 12)])
def test_db2_band_matches_direct_convolution(h, w):
    dec_hi = [-0.48296291314469025, 0.836516303737469, -0.22414386804185735, -0.12940952255092145]   # pywt.Wavelet('db2').dec_hi
    x = np.random.default_rng(h + w).integers(0, 256, (h, w)).astype(np.float64)
    t = np.stack([_dwt_hi_direct(x[:, c], dec_hi) for c in range(w)], axis=1)
    ref = np.stack([_dwt_hi_direct(t[r], dec_hi) for r in range(t.shape[0])], axis=0)
    got = CR.db2_hh(x)
    assert got.shape == ((h + 3) // 2, (w + 3) // 2)
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.max(np.abs(ref)))


def test_noise_sigma_median_rule_and_flat_image():
    x = np.random.default_rng(5).integers(0, 256, (24, 26)).astype(np.uint8)
    d = np.abs(CR.db2_hh(x)).ravel()
    d = d[d != 0]
    assert d.size % 2 == 0                                      # 13 x 14: the even-count branch (mean of the middle two)
    assert CR.noise_sigma(x) == pytest.approx(np.median(d) / 0.6744897501960817, rel=0, abs=0)
    assert np.isnan(CR.noise_sigma(np.full((20, 20), 77, np.uint8)))      # a flat image has no detail coefficient at all


def test_classic_entries_refuse_a_null_context():
    from sr355 import _lib
    lib = _lib.load()
    assert lib.sr_back_projection(None, None, None, 1, 8, 8, 4, 4, 1, None, None, None) == _lib.SR_ERR_INVALID
    assert lib.sr_noise_sigma(None, None, 1, 8, 8, None, None) == _lib.SR_ERR_INVALID
    assert lib.sr_nl_means(None, None, 1, 8, 8, 5, 6, None, 1.15, None, None) == _lib.SR_ERR_INVALID
    assert lib.sr_edge_guided(None, None, 1, 4, 4, 8, 8, 0.3, None, None, None) == _lib.SR_ERR_INVALID
    assert lib.sr_freq_extrapolate(None, None, 1, 4, 4, 8, 8, None, None) == _lib.SR_ERR_INVALID
