"""The host side of the classical study's device loop: the fp64 restatements of tests/classical_study_ref.py against independent forms
(metrics_ref.ssim_map, scipy.ndimage.uniform_filter, a hand-made ranking), the NumPy halves of visualization_methods.py, and what must
work without a GPU (imports, the plot stubs, classical_study's argument checks)."""
import subprocess
import sys

import numpy as np
import pytest

import classical_study_ref as SR
import metrics_ref as MR

# the GPU test's shapes (tests/test_classical_study_gpu.py)
SHAPES = [(7, 7), (9, 13), (33, 40), (64, 64)]


u8_pair = SR.u8_pair


@pytest.mark.parametrize("H,W", SHAPES)
def test_ssim_full_interior_is_the_cropped_map(H, W):
    a, b = u8_pair(H, W, H * 100 + W)
    for dr in (255.0, 200.0):
        S, m = SR.ssim_full(a, b, dr)
        assert S.shape == (H, W) and S.dtype == np.float64
        # uint8 values: both cumulative-sum forms are exact integers, so the interior is the cropped map bit for bit
        assert S[3:-3, 3:-3].tobytes() == MR.ssim_map(a, b, dr).tobytes()
        assert m == MR.ssim(a, b, dr)
    # float images: the two forms round their cumulative sums differently
    af, bf = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    S, m = SR.ssim_full(af, bf, 1.0)
    assert np.max(np.abs(S[3:-3, 3:-3] - MR.ssim_map(af, bf, 1.0))) <= 1e-12
    rgb_a, rgb_b = np.stack([a, b, a[::-1]], -1), np.stack([b, b, a], -1)
    S3, m3 = SR.ssim_full(rgb_a, rgb_b, 255.0)
    assert S3.shape == (H, W, 3) and m3 == MR.ssim(rgb_a, rgb_b, 255.0)
    assert S3[..., 2].tobytes() == SR.ssim_full(rgb_a[..., 2], rgb_b[..., 2], 255.0)[0].tobytes()


@pytest.mark.parametrize("H,W", SHAPES)
def test_ssim_full_matches_scipy_uniform_filter(H, W):
    """skimage's own formulation: uniform_filter(size=7) (mode='reflect') of x, y, x x, y y, x y.  Two fp64 formulations: 4e-13 per element."""
    ndi = pytest.importorskip("scipy.ndimage")
    a, b = u8_pair(H, W, H * 100 + W + 1)
    for x, y, dr in ((a.astype(np.float64), b.astype(np.float64), 255.0),
                     ((a.astype(np.float32) / np.float32(255)).astype(np.float64), b.astype(np.float64), 255.0)):
        f = lambda v: ndi.uniform_filter(v, size=7)
        ux, uy, uxx, uyy, uxy = f(x), f(y), f(x * x), f(y * y), f(x * y)
        cn = 49.0 / 48.0
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        C1, C2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
        ref = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        S, m = SR.ssim_full(x, y, dr)
        assert np.max(np.abs(S - ref)) <= 4e-13
        assert abs(m - ref[3:-3, 3:-3].mean()) <= 4e-13


def test_border_rule_shows_on_every_edge():
    """What the GPU test relies on: on such inputs REFLECT_101, clamp and zero borders move each of the four edge strips by more than 2e-3
    and leave the interior alone."""
    a, b = u8_pair(33, 40, 5)
    S, _ = SR.ssim_full(a, b, 255.0)
    for mode in ("reflect", "edge", "constant"):
        pa, pb = (np.pad(v.astype(np.float64), 3, mode=mode) for v in (a, b))
        ux, uy = MR._box7(pa) / 49.0, MR._box7(pb) / 49.0
        uxx, uyy, uxy = MR._box7(pa * pa) / 49.0, MR._box7(pb * pb) / 49.0, MR._box7(pa * pb) / 49.0
        cn = 49.0 / 48.0
        vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
        C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
        other = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
        d = np.abs(other - S)
        assert d[3:-3, 3:-3].max() == 0.0
        for strip in (d[:3], d[-3:], d[:, :3], d[:, -3:]):
            assert strip.max() > 2e-3, mode


def test_freq_to_u8_restatement():
    rng = np.random.default_rng(0)
    f = np.abs(rng.normal(0, 40, (9, 11)))
    y, m = SR.freq_to_u8(f)
    assert m == f.max() and y.dtype == np.uint8 and y.max() == 255 and y[np.unravel_index(np.argmax(f), f.shape)] == 255
    assert np.array_equal(y, np.floor(f / f.max() * 255.0).astype(np.uint8))
    z, mz = SR.freq_to_u8(np.zeros((4, 4)))
    assert mz == 0.0 and not z.any()
    c, mc = SR.freq_to_u8(np.full((3, 5), 0.3))
    assert mc == 0.3 and (c == 255).all()


def hand_summary():
    """Three algorithms: a NaN metric (kl_color of a gray method), a metric without spread (memory), derived metrics from the intervals."""
    return {
        "a": {"psnr_mean": 30.0, "ssim_mean": 0.9, "time_mean": 1.0, "memory_mean": 5.0, "kl_color_mean": 0.2, "epi_mean": 1.1,
              "psnr_ci_low": 29.0, "psnr_ci_high": 31.0},
        "b": {"psnr_mean": 20.0, "ssim_mean": 0.5, "time_mean": 3.0, "memory_mean": 5.0, "kl_color_mean": np.nan, "epi_mean": 0.7,
              "psnr_ci_low": 19.5, "psnr_ci_high": 20.0},
        "c": {"psnr_mean": 25.0, "ssim_mean": 0.8, "time_mean": 2.0, "memory_mean": 5.0, "kl_color_mean": 0.6, "epi_mean": 1.0,
              "psnr_ci_low": 24.0, "psnr_ci_high": 25.0},
    }


def test_ranking_contributions_by_hand():
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    from SRModels.classic_super_resolution_algorithms import visualization_methods as VM
    summary = hand_summary()
    ranked, scores, bounds, metrics, contrib = VM.ranking_contributions(summary)
    r0, s0, b0 = P.rank_algorithms(summary)
    assert ranked == r0 and scores == s0 and bounds == b0 and metrics == list(b0)
    assert metrics == ["psnr_mean", "ssim_mean", "time_mean", "memory_mean", "kl_color_mean", "psnr_ci_width", "epi_dev"]
    algs = [a for a, _ in ranked]
    assert algs == ["a", "c", "b"]
    w = 1.0 / 7.0
    by_hand = {                            # psnr, ssim, time, memory (no spread), kl_color (NaN for b), psnr_ci_width (2, .5, 1), epi_dev (.1, .3, 0)
        "a": [1.0, 1.0, 1.0, 0.0, 1.0, 0.0, 2.0 / 3.0],
        "b": [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0],
        "c": [0.5, 0.75, 0.5, 0.0, 0.0, 2.0 / 3.0, 1.0],
    }
    assert contrib.shape == (3, 7)
    for i, a in enumerate(algs):
        assert contrib[i] == pytest.approx(np.array(by_hand[a]) * w, abs=1e-15)
        assert contrib[i].sum() == pytest.approx(scores[a], abs=1e-15)
    assert np.array_equal(contrib, SR.ranking_contributions(summary, algs, metrics, maximize={"psnr_mean", "ssim_mean"}))
    # given lists and weights: used as they are, a metric missing from the weights weighs 0
    ranked2, scores2, _, metrics2, contrib2 = VM.ranking_contributions(summary, maximize=["ssim_mean"], minimize=["time_mean", "kl_color_mean"],
                                                                       weights={"ssim_mean": 0.5, "time_mean": 0.25})
    assert metrics2 == ["ssim_mean", "time_mean", "kl_color_mean"] and not contrib2[:, 2].any()
    algs2 = [a for a, _ in ranked2]
    assert np.array_equal(contrib2, SR.ranking_contributions(summary, algs2, metrics2, {"ssim_mean"}, {"ssim_mean": 0.5, "time_mean": 0.25}))
    assert contrib2[algs2.index("a")].tolist() == [0.5, 0.25, 0.0] and scores2["a"] == 0.75


def test_super_resolution_example_applies_to_display():
    from SRModels.classic_super_resolution_algorithms import visualization_methods as VM
    rng = np.random.default_rng(1)
    rgb = lambda: rng.integers(0, 256, (8, 9, 3)).astype(np.uint8)
    g = lambda: rng.integers(0, 256, (8, 9)).astype(np.uint8)
    nlm32 = rng.normal(0.5, 0.6, (8, 9)).astype(np.float32)
    vis = (rgb(), rgb()[:4, :4], rgb(), rgb(), rgb(), rgb())
    hr_g = g()
    out = VM.super_resolution_example(vis, (hr_g, g(), g()), (hr_g, nlm32), (hr_g, g(), g()), (hr_g, g()))
    assert [t for t, _ in out] == ["HR", "LR", "Bilinear", "Bicubic", "Area", "Lanczos", "IBP", "NLM", "EGI", "FREQ"]
    assert out[0][1] is vis[0] and out[1][1] is vis[1]
    assert np.array_equal(out[7][1], np.clip(nlm32, 0, 1)) and (nlm32 > 1).any()
    nlm64 = nlm32.astype(np.float64)                     # the reference clips float32 only
    assert VM.super_resolution_example(vis, (hr_g, g(), g()), (hr_g, nlm64), (hr_g, g(), g()), (hr_g, g()))[7][1] is nlm64


PLOTS = {"plot_time_memory_panels": "build_metrics_summary", "plot_psnr_ssim_panels": "build_metrics_summary",
         "plot_speed_quality_tradeoff_3d": "build_metrics_summary", "plot_error_metrics_grid": "build_metrics_summary",
         "plot_edge_metrics_grid": "build_metrics_summary", "plot_frequency_distribution_metrics_grid": "build_metrics_summary",
         "plot_and_save_super_resolution_example": "super_resolution_example", "plot_and_save_ssim_similarity_maps": "ssim_similarity_maps",
         "show_algorithm_ranking": "ranking_contributions"}


@pytest.mark.parametrize("name", sorted(PLOTS))
def test_plot_functions_name_their_numeric_halves(name):
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    from SRModels.classic_super_resolution_algorithms import visualization_methods as VM
    with pytest.raises(NotImplementedError, match=PLOTS[name]):
        getattr(VM, name)({}, [], {}, "title", "out.png")
    assert callable(getattr(VM, PLOTS[name], None) or getattr(P, PLOTS[name]))


def test_import_touches_no_device():
    """Importing the visualisation module and sr355.study creates no context and initialises no GPU runtime."""
    code = ("import sys, os\n"
            "root = sys.argv[1]\n"
            "sys.path[:0] = [root, os.path.join(root, 'super-resolution-images-for-3d-printing-defect-detection_amd')]\n"
            "import torch\n"
            "from SRModels.classic_super_resolution_algorithms import visualization_methods as VM\n"
            "import sr355.study as S\n"
            "from sr355 import Context\n"
            "assert not Context._instances and not torch.cuda.is_initialized()\n"
            "assert callable(VM.ssim_similarity_maps) and callable(S.classical_study)\n"
            "print('ok')\n")
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code, root], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_classical_study_checks_its_arguments_before_any_device_work():
    import torch
    from sr355.study import CLASSIC_ALGORITHMS, CLASSIC_STAT_KEYS, classical_study
    assert CLASSIC_ALGORITHMS == SR.ALGORITHMS and CLASSIC_STAT_KEYS == SR.STAT_KEYS
    hr, lr = np.zeros((2, 16, 16, 3), np.uint8), np.zeros((2, 8, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="float"):
        classical_study(hr.astype(np.float32), lr)
    with pytest.raises(ValueError, match="same size"):
        classical_study([hr[0], np.zeros((16, 17, 3), np.uint8)], lr)
    with pytest.raises(ValueError, match="2 HR images for 1 LR"):
        classical_study(hr, lr[:1])
    with pytest.raises(ValueError, match="example_index"):
        classical_study(hr, lr, example_index=2)
    with pytest.raises(ValueError, match="RGB stack"):
        classical_study(hr[..., 0], lr)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                 # valid arguments reach the device, and there is none: no CPU path
            classical_study(hr, lr)


def test_structural_similarity_keeps_refusing_other_keywords():
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    a = np.zeros((8, 8), np.uint8)
    with pytest.raises(NotImplementedError, match="gaussian_weights"):
        P.structural_similarity(a, a, data_range=255, full=True, gaussian_weights=True)
    with pytest.raises(NotImplementedError, match="win_size"):
        P.structural_similarity(a, a, data_range=255, win_size=11)
