"""The classical study's nine image-quality scores on the device (sr_classic_scores, Context.classic_scores, SRModels' profiling_methods)
against the fp64 NumPy restatement of tests/metrics_ref.py, on synthetic 3D-print tiles from sr355.synth."""
import math

import numpy as np
import pytest
import torch

import metrics_ref as MR

pytestmark = pytest.mark.gpu

NAMES = MR.NAMES
IDX = {k: i for i, k in enumerate(NAMES)}


def tile_pair(H, W, C, seed):
    """uint8 HR from sr355.synth plus noise, and an SR that is a blurred, noisier copy."""
    from sr355.synth import hr_tile
    rng = np.random.default_rng(seed)
    hr = np.clip(hr_tile(rng, H, W).astype(np.float64) * 255.0 + rng.normal(0, 5, (H, W, 3)), 0, 255)
    pad = np.pad(hr, ((1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    sr = np.clip(blur + rng.normal(0, 8, hr.shape), 0, 255)
    hr, sr = hr.astype(np.uint8), sr.astype(np.uint8)
    return (hr, sr) if C == 3 else (hr[..., 1], sr[..., 1])


def make_case(kind, H, W, C, seed):
    hr, sr = tile_pair(H, W, C, seed)
    if kind == "u8":
        return hr, sr, 255.0
    if kind == "u8_f32":                       # the notebook's NL-means row: uint8 HR against float SR in [0, 1]
        return hr, sr.astype(np.float32) / np.float32(255), "hr_span"
    return hr.astype(np.float32) / np.float32(255), sr.astype(np.float32) / np.float32(255), 1.0      # hr_f, sr_f


def assert_scores(got, ref, floaty):
    for k in NAMES:
        g, r = float(got[IDX[k]]), float(ref[IDX[k]])
        if math.isnan(r) or math.isinf(r):
            assert (math.isnan(g) and math.isnan(r)) or g == r, (k, g, r)
            continue
        if k == "ssim":
            tol = 1e-6 if floaty else 1e-9
            assert abs(g - r) <= tol, (k, g, r)
        else:
            rel = {"grad_mse": 1e-5, "epi": 1e-5, "hf_ratio": 1e-9}.get(k, 1e-6 if floaty else 1e-12)
            assert abs(g - r) <= rel * abs(r), (k, g, r, abs(g - r) / abs(r))


SHAPES = [(478, 478, 3), (478, 478, 1), (48, 48, 3), (48, 48, 1), (70, 53, 3), (70, 53, 1), (7, 7, 3), (7, 7, 1)]


# the notebook scores float SR output (NL-means) only in its gray branch
CASES = [(kind, H, W, C) for (H, W, C) in SHAPES for kind in ("u8", "u8_f32", "f32") if not (kind == "u8_f32" and C == 3)]


@pytest.mark.parametrize("kind,H,W,C", CASES)
def test_scores_match_restatement(ctx, kind, H, W, C):
    hr, sr, dr = make_case(kind, H, W, C, seed=H * 7 + W + C)
    got, raw = ctx.classic_scores(ctx.to_device(hr[None]), ctx.to_device(sr[None]), dr, raw=True)
    ref = MR.scores(hr, sr, dr)
    assert_scores(got[0].cpu().numpy(), ref, floaty=kind != "u8")
    if C == 1 or kind == "u8":
        for k, img in enumerate((hr, sr)):
            assert np.array_equal(raw["hist_luma"][0, k].cpu().numpy(), MR.hist_counts(MR.gray_of(img), 256))
            assert np.array_equal(raw["gray"][0, k].cpu().numpy(), MR.gray_of(img).astype(np.float32))
            assert np.max(np.abs(raw["sobel"][0, k].cpu().numpy() - MR.sobel_mag(img))) <= 1e-5 * max(1.0, MR.sobel_mag(img).max())
    if C == 3:
        for k, img in enumerate((hr, sr)):
            for c in range(3):
                assert np.array_equal(raw["hist_color"][0, k, c].cpu().numpy(), MR.hist_counts(img[..., c], 64))


def test_batch_of_eight_and_determinism(ctx):
    pairs = [tile_pair(70, 53, 3, seed=100 + i) for i in range(8)]
    hr = ctx.to_device(np.stack([p[0] for p in pairs]))
    sr = ctx.to_device(np.stack([p[1] for p in pairs]))
    dr = np.linspace(200.0, 255.0, 8)
    a = ctx.classic_scores(hr, sr, dr).cpu().numpy()
    b = ctx.classic_scores(hr, sr, dr).cpu().numpy()
    assert a.tobytes() == b.tobytes()
    for i in (0, 5, 7):
        one = ctx.classic_scores(hr[i:i + 1].contiguous(), sr[i:i + 1].contiguous(), dr[i:i + 1]).cpu().numpy()
        assert one.tobytes() == a[i:i + 1].tobytes(), i
        assert_scores(a[i], MR.scores(pairs[i][0], pairs[i][1], dr[i]), floaty=False)
    g = [tile_pair(478, 478, 1, seed=200 + i) for i in range(3)]
    hg, sg = ctx.to_device(np.stack([p[0] for p in g])), ctx.to_device(np.stack([p[1] for p in g]).astype(np.float32) / 255)
    full = ctx.classic_scores(hg, sg, "hr_span").cpu().numpy()
    assert ctx.classic_scores(hg[1:2].contiguous(), sg[1:2].contiguous(), "hr_span").cpu().numpy().tobytes() == full[1:2].tobytes()


def test_edge_cases(ctx):
    hr, _ = tile_pair(48, 48, 3, seed=1)
    s = ctx.classic_scores(ctx.to_device(hr[None]), ctx.to_device(hr[None])).cpu().numpy()[0]
    assert s[IDX["psnr"]] == math.inf and s[IDX["ssim"]] == 1.0 and s[IDX["kl_luma"]] == 0.0 and s[IDX["kl_color"]] == 0.0
    assert s[IDX["epi"]] == 1.0 and s[IDX["grad_mse"]] == 0.0 and s[IDX["mae"]] == 0.0
    c = np.full((1, 20, 24), 90, np.uint8)
    assert ctx.classic_scores(ctx.to_device(c), ctx.to_device(c)).cpu().numpy()[0, IDX["epi"]] == 1.0
    # a gray image whose max is 1 is not rescaled (its own rule); its uint8 partner with max 255 is
    rng = np.random.default_rng(3)
    binary = (rng.random((1, 30, 31)) > 0.5).astype(np.uint8)
    other = rng.integers(0, 256, (1, 30, 31)).astype(np.uint8)
    got, raw = ctx.classic_scores(ctx.to_device(binary), ctx.to_device(other), raw=True)
    assert np.max(np.abs(raw["sobel"][0, 0].cpu().numpy() - MR.sobel_mag(binary[0]))) <= 1e-6
    assert MR.sobel_mag(binary[0]).max() > 1.5
    assert_scores(got[0].cpu().numpy(), MR.scores(binary[0], other[0]), floaty=False)
    # 'hr_span': max(hr) - min(hr), 255 when that is 0
    h2 = np.stack([np.clip(other[0], 20, 220), np.full((30, 31), 5, np.uint8)])
    s2 = np.stack([other[0], other[0]])
    span = ctx.classic_scores(ctx.to_device(h2), ctx.to_device(s2), "hr_span").cpu().numpy()
    explicit = ctx.classic_scores(ctx.to_device(h2), ctx.to_device(s2), [200.0, 255.0]).cpu().numpy()
    assert span.tobytes() == explicit.tobytes()
    assert math.isnan(span[0, IDX["kl_color"]])
    # float RGB: the gray columns are NaN on the device and the gray metrics refuse it
    f = np.random.default_rng(4).random((1, 16, 16, 3)).astype(np.float32)
    s = ctx.classic_scores(ctx.to_device(f), ctx.to_device(f[:, ::-1].copy())).cpu().numpy()[0]
    assert all(math.isnan(s[IDX[k]]) for k in ("grad_mse", "epi", "hf_ratio", "kl_luma")) and not math.isnan(s[IDX["kl_color"]])
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    with pytest.raises(NotImplementedError, match="float RGB"):
        P.gradient_mse(f[0], f[0])
    with pytest.raises(ValueError):
        ctx.classic_scores(ctx.to_device(np.zeros((1, 6, 9), np.uint8)), ctx.to_device(np.zeros((1, 6, 9), np.uint8)))
    with pytest.raises(ValueError):
        P.mae(np.zeros((9, 6), np.uint8), np.zeros((9, 6), np.uint8))


def test_wrappers_match_restatement(ctx):
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    hr, sr = tile_pair(70, 53, 3, seed=9)
    ref = MR.scores(hr, sr)
    hg, sg = MR.rgb2gray_u8(hr), MR.rgb2gray_u8(sr)
    got = {"mae": P.mae(hr, sr), "rmse": P.rmse(hr, sr), "grad_mse": P.gradient_mse(hr, sr), "epi": P.epi(hr, sr),
           "hf_ratio": P.hf_energy_ratio(hg, sg, radius_frac=0.6), "kl_luma": P.kl_divergence(hg, sg), "kl_color": P.kl_divergence_color(hr, sr),
           "psnr": P.peak_signal_noise_ratio(hr, sr, data_range=255), "ssim": P.structural_similarity(hr, sr, data_range=255, channel_axis=2)}
    assert all(isinstance(v, float) for v in got.values())
    assert_scores(np.array([got[k] for k in NAMES]), ref, floaty=False)
    assert np.max(np.abs(P.sobel_mag(hr) - MR.sobel_mag(hr))) <= 1e-5 and P.sobel_mag(hr).dtype == np.float32
    # float32 RGB in [0, 1] with data_range 1 scores PSNR / SSIM as uint8 with 255 does, up to float32 rounding
    hf, sf = hr.astype(np.float32) / 255, sr.astype(np.float32) / 255
    assert P.peak_signal_noise_ratio(hf, sf, data_range=1.0) == pytest.approx(got["psnr"], rel=1e-6)
    assert P.structural_similarity(hf, sf, data_range=1.0, channel_axis=2) == pytest.approx(got["ssim"], abs=1e-6)
    # float64 goes in as float32
    assert P.mae(hg, sg.astype(np.float64) / 255) == P.mae(hg, (sg.astype(np.float32) / 255))


def test_device_upscalers_scored_in_place(ctx):
    """The four device up-scalers and a device resize, scored as device tensors through score_pairs, equal scoring their host copies."""
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    pairs = [tile_pair(96, 96, 1, seed=300 + i) for i in range(2)]
    hr = ctx.to_device(np.stack([p[0] for p in pairs]))
    lr = ctx.resize(hr.unsqueeze(-1), 48, 48, "INTER_AREA").squeeze(-1).contiguous()
    freq = ctx.freq_extrapolate(lr, 96, 96)
    mx = freq.reshape(2, -1).amax(1).reshape(2, 1, 1)
    outs = {
        "ibp": ctx.back_projection(hr, lr, 10),
        "nlm": ctx.non_local_means(lr, 96, 96),
        "egi": ctx.edge_guided(lr, 96, 96),
        "freq": (freq / mx * 255.0).to(torch.uint8),
        "bilinear": ctx.resize(lr.unsqueeze(-1), 96, 96, "INTER_LINEAR").squeeze(-1).contiguous(),
    }
    for name, sr in outs.items():
        dr = "hr_span" if name == "nlm" else 255.0
        dev = P.score_pairs(hr, sr.contiguous(), dr)
        host = P.score_pairs(hr.cpu().numpy(), sr.cpu().numpy(), dr)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
        for k in NAMES:
            assert dev[k].cpu().numpy().tobytes() == host[k].tobytes(), (name, k)
        for i in range(2):
            assert_scores(np.array([host[k][i] for k in NAMES]), MR.scores(hr[i].cpu().numpy(), sr[i].cpu().numpy(), dr), floaty=name == "nlm")


REFERENCE_SUMMARY_KEYS = {
    'psnr_mean', 'psnr_var', 'psnr_max', 'psnr_ci_low', 'psnr_ci_high', 'ssim_mean', 'ssim_var', 'ssim_max', 'ssim_ci_low', 'ssim_ci_high',
    'time_mean', 'time_max', 'time_jitter', 'time_var', 'memory_mean', 'memory_max', 'memory_var', 'mae_mean', 'mae_max', 'rmse_mean',
    'rmse_max', 'grad_mse_mean', 'epi_mean', 'hf_ratio_mean', 'kl_luma_mean', 'kl_color_mean'}


def test_notebook_loop(ctx):
    """The notebook's scoring loop and summary (its cells 8 and 9) on two synthetic RGB pairs: drop-in up-scalers, profiling_methods
    and the skimage-named functions, then build_metrics_summary and rank_algorithms.  Gray conversion comes from the restatement."""
    from SRModels.classic_super_resolution_algorithms import classic_algorithms as CA
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    from SRModels.classic_super_resolution_algorithms.profiling_methods import peak_signal_noise_ratio as psnr, structural_similarity as ssim
    from sr355.synth import make_pairs
    lr_f, hr_f = make_pairs(2, 48, 48, 2, seed=11)
    algorithms = ["bilinear", "bicubic", "area", "lanczos", "ibp", "nlm", "egi", "freq"]
    stats = {k: {a: [] for a in algorithms} for k in ("time", "memory", "psnr", "ssim", "mae", "rmse", "grad", "epi", "hf", "kl_luma", "kl_color")}
    for hr_img, lr_img in zip((hr_f * 255).astype(np.uint8), (lr_f * 255).astype(np.uint8)):
        h, w = hr_img.shape[:2]
        outs = {}
        for name, fn in (("bilinear", CA.interpolate_bilinear), ("bicubic", CA.interpolate_bicubic), ("area", CA.interpolate_area),
                         ("lanczos", CA.interpolate_lanczos)):
            outs[name], t = P.time_algorithm(fn, lr_img, (w, h))
            _, mem = P.memory_algorithm(fn, lr_img, (w, h))
            stats["time"][name].append(t)
            stats["memory"][name].append(mem)
        hrf = hr_img.astype(np.float32) / 255.0
        for name in ("bilinear", "bicubic", "area", "lanczos"):
            sr_img = outs[name]
            srf = sr_img.astype(np.float32) / 255.0
            stats["psnr"][name].append(psnr(hrf, srf, data_range=1.0))
            stats["ssim"][name].append(ssim(hrf, srf, channel_axis=2, data_range=1.0))
            stats["mae"][name].append(P.mae(hr_img, sr_img))
            stats["rmse"][name].append(P.rmse(hr_img, sr_img))
            stats["grad"][name].append(P.gradient_mse(hr_img, sr_img))
            stats["epi"][name].append(P.epi(hr_img, sr_img))
            stats["hf"][name].append(P.hf_energy_ratio(MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(sr_img), radius_frac=0.6))
            stats["kl_luma"][name].append(P.kl_divergence(MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(sr_img)))
            stats["kl_color"][name].append(P.kl_divergence_color(hr_img, sr_img))
            ref = MR.scores(hr_img, sr_img)
            assert stats["mae"][name][-1] == pytest.approx(ref[IDX["mae"]], rel=1e-12)
            assert stats["ssim"][name][-1] == pytest.approx(MR.ssim(hr_img, sr_img, 255.0), abs=1e-6)
        hr_g, lr_g = MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(lr_img)
        for name, fn in (("ibp", lambda: CA.back_projection(hr_g, lr_g, iterations=10)), ("nlm", lambda: CA.non_local_means(hr_g, lr_g)),
                         ("egi", lambda: CA.edge_guided_interpolation(hr_g, lr_g)), ("freq", lambda: CA.frequency_extrapolation(hr_g, lr_g))):
            outs[name], t = P.time_algorithm(fn)
            _, mem = P.memory_algorithm(fn)
            stats["time"][name].append(t)
            stats["memory"][name].append(mem)
        f = outs["freq"]
        outs["freq"] = (f / np.max(f) * 255.0).astype(np.uint8) if np.max(f) > 0 else f.astype(np.uint8)
        dr_nlm = hr_g.max() - hr_g.min() if hr_g.max() != hr_g.min() else 255.0
        for name in ("ibp", "nlm", "egi", "freq"):
            sr_g = outs[name]
            dr = dr_nlm if name == "nlm" else 255.0
            stats["psnr"][name].append(psnr(hr_g, sr_g, data_range=dr))
            stats["ssim"][name].append(ssim(hr_g, sr_g, data_range=dr))
            stats["mae"][name].append(P.mae(hr_g, sr_g))
            stats["rmse"][name].append(P.rmse(hr_g, sr_g))
            stats["grad"][name].append(P.gradient_mse(hr_g, sr_g))
            stats["epi"][name].append(P.epi(hr_g, sr_g))
            stats["hf"][name].append(P.hf_energy_ratio(hr_g, sr_g, radius_frac=0.6))
            stats["kl_luma"][name].append(P.kl_divergence(hr_g, sr_g))
            stats["kl_color"][name].append(np.nan)
            ref = MR.scores(hr_g, sr_g, dr)
            got = [stats[k][name][-1] for k in ("psnr", "ssim", "mae", "rmse", "grad", "epi", "hf", "kl_luma", "kl_color")]
            assert_scores(np.array(got), ref, floaty=name == "nlm")
    summary = P.build_metrics_summary(*(stats[k] for k in ("time", "memory", "psnr", "ssim", "mae", "rmse", "grad", "epi", "hf", "kl_luma",
                                                            "kl_color")))
    assert list(summary) == algorithms and all(set(v) == REFERENCE_SUMMARY_KEYS for v in summary.values())
    assert all(math.isfinite(summary[a]["psnr_ci_low"]) for a in algorithms)
    ranked, scores, bounds = P.rank_algorithms(summary)
    assert sorted(a for a, _ in ranked) == sorted(algorithms) and all(0.0 <= s <= 1.0 for s in scores.values())
    ranked2, _, _ = P.rank_algorithms(summary, maximize=P.MAXIMIZE_DEFAULT, minimize=P.MINIMIZE_DEFAULT)
    assert len(ranked2) == 8
