"""fp64 NumPy restatements behind the classical study's device loop (sr355.study.classical_study) and the numeric halves of
classic_super_resolution_algorithms/visualization_methods.py:

  ssim_full(a, b, dr)        skimage's structural_similarity(..., full=True) with its defaults: S over the WHOLE image, the window sums
                             taken on the image padded by 3 with np.pad(mode='symmetric') (scipy.ndimage.uniform_filter's default
                             'reflect': d c b a | a b c d), and mssim, the mean over the centres 3 pixels inside the border (RGB: the mean
                             of the per-channel means).  The interior of S is metrics_ref.ssim_map's.
  freq_to_u8(f)              the notebook's `(f / np.max(f) * 255.0).astype(np.uint8) if np.max(f) > 0 else f.astype(np.uint8)`, with the max.
  ranking_contributions      show_algorithm_ranking's weight x normalised-value matrix (visualization_methods.py:617-689), vectorised.
  per_image_route            the notebook's cell 8 one image at a time through the drop-ins, exactly as
                             test_classic_metrics_gpu.py::test_notebook_loop calls them (needs a GPU: the drop-ins run on it)."""
import numpy as np

import metrics_ref as MR

ALGORITHMS = ("bilinear", "bicubic", "area", "lanczos", "ibp", "nlm", "egi", "freq")
STAT_KEYS = ("time", "memory", "psnr", "ssim", "mae", "rmse", "gradient_mse", "epi", "hf_energy_ratio", "kl_luma", "kl_color")


def u8_pair(H, W, seed):
    """Uniformly random uint8 pair with a block where the two agree and a flat corner."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (H, W)).astype(np.uint8)
    b = rng.integers(0, 256, (H, W)).astype(np.uint8)
    b[H // 3:H // 3 + max(2, H // 4), W // 4:W // 4 + max(2, W // 3)] = a[H // 3:H // 3 + max(2, H // 4), W // 4:W // 4 + max(2, W // 3)]
    a[:3, :4] = 17
    b[:3, :4] = 17
    return a, b


def _ssim_channel(a, b, dr):
    pa = np.pad(np.asarray(a, np.float64), 3, mode="symmetric")
    pb = np.pad(np.asarray(b, np.float64), 3, mode="symmetric")
    ux, uy = MR._box7(pa) / 49.0, MR._box7(pb) / 49.0
    uxx, uyy, uxy = MR._box7(pa * pa) / 49.0, MR._box7(pb * pb) / 49.0, MR._box7(pa * pb) / 49.0
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim_full(a, b, dr):
    """(S, mssim) of one pair [H, W] or [H, W, C]; S float64 of the images' shape."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.shape[0] < 7 or a.shape[1] < 7:
        raise ValueError("images of different shapes, or smaller than the 7 x 7 window")
    if a.ndim == 2:
        S = _ssim_channel(a, b, float(dr))
        return S, float(S[3:-3, 3:-3].mean())
    S = np.stack([_ssim_channel(a[..., c], b[..., c], float(dr)) for c in range(a.shape[2])], axis=-1)
    return S, float(np.mean([S[3:-3, 3:-3, c].mean() for c in range(a.shape[2])]))


def freq_to_u8(f):
    """(uint8 image, max) of one fp64 image, the notebook's expression."""
    f = np.asarray(f, np.float64)
    m = np.max(f)
    return ((f / m * 255.0).astype(np.uint8) if m > 0 else f.astype(np.uint8)), m


_DERIVED = {"psnr_ci_width": ("psnr_ci_low", "psnr_ci_high"), "ssim_ci_width": ("ssim_ci_low", "ssim_ci_high")}
_DEV = {"epi_dev": "epi_mean", "hf_ratio_dev": "hf_ratio_mean"}


def metric_values(summary, algs, metric):
    """The metric's value per algorithm, float64 [len(algs)], derived metrics included; NaN where missing or not finite."""
    out = np.full(len(algs), np.nan)
    for i, a in enumerate(algs):
        st = summary[a]
        if metric in _DERIVED:
            lo, hi = (st.get(k, np.nan) for k in _DERIVED[metric])
            out[i] = hi - lo if np.isfinite(lo) and np.isfinite(hi) else np.nan
        elif metric in _DEV:
            v = st.get(_DEV[metric], np.nan)
            out[i] = abs(v - 1.0) if np.isfinite(v) else np.nan
        else:
            out[i] = st.get(metric, np.nan)
    return out


def ranking_contributions(summary, algs, metrics, maximize, weights=None):
    """contrib [len(algs), len(metrics)]: weight x min-max normalised value over the algorithms' finite values ((v - lo) / (hi - lo) for
    the metrics of `maximize`, (hi - v) / (hi - lo) for the others), 0 for a value that is not finite or a metric without spread."""
    w = {m: 1.0 / max(1, len(metrics)) for m in metrics} if weights is None else {m: float(weights.get(m, 0.0)) for m in metrics}
    contrib = np.zeros((len(algs), len(metrics)))
    for j, m in enumerate(metrics):
        v = metric_values(summary, algs, m)
        ok = np.isfinite(v)
        if not ok.any():
            continue
        lo, hi = v[ok].min(), v[ok].max()
        if hi == lo:
            continue
        norm = (v - lo) / (hi - lo) if m in maximize else (hi - v) / (hi - lo)
        contrib[:, j] = np.where(ok, np.clip(norm, 0.0, 1.0), 0.0) * w[m]
    return contrib


def per_image_route(hr_imgs, lr_imgs, iterations=10, radius_frac=0.6, profile=False):
    """Cell 8 for each (hr, lr) uint8 RGB pair through the drop-ins of classic_algorithms / profiling_methods, the gray images by
    metrics_ref.rgb2gray_u8.  -> (stats {key: {alg: list}}, outs: per image {alg: image} with freq already normalised, plus 'hr_g' and
    'lr_g').  profile=True also runs memory_algorithm's second pass of every algorithm, as the notebook does; time is wall clock."""
    from SRModels.classic_super_resolution_algorithms import classic_algorithms as CA
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    from SRModels.classic_super_resolution_algorithms.profiling_methods import peak_signal_noise_ratio as psnr, structural_similarity as ssim
    stats = {k: {a: [] for a in ALGORITHMS} for k in STAT_KEYS}
    all_outs = []

    def run(name, fn, *args):
        out, t = P.time_algorithm(fn, *args)
        mem = P.memory_algorithm(fn, *args)[1] if profile else 0
        stats["time"][name].append(t)
        stats["memory"][name].append(mem)
        return out

    for hr_img, lr_img in zip(hr_imgs, lr_imgs):
        h, w = hr_img.shape[:2]
        outs = {}
        for name, fn in (("bilinear", CA.interpolate_bilinear), ("bicubic", CA.interpolate_bicubic), ("area", CA.interpolate_area),
                         ("lanczos", CA.interpolate_lanczos)):
            outs[name] = run(name, fn, lr_img, (w, h))
        hrf = hr_img.astype(np.float32) / 255.0
        for name in ("bilinear", "bicubic", "area", "lanczos"):
            sr_img = outs[name]
            srf = sr_img.astype(np.float32) / 255.0
            stats["psnr"][name].append(psnr(hrf, srf, data_range=1.0))
            stats["ssim"][name].append(ssim(hrf, srf, channel_axis=2, data_range=1.0))
            stats["mae"][name].append(P.mae(hr_img, sr_img))
            stats["rmse"][name].append(P.rmse(hr_img, sr_img))
            stats["gradient_mse"][name].append(P.gradient_mse(hr_img, sr_img))
            stats["epi"][name].append(P.epi(hr_img, sr_img))
            stats["hf_energy_ratio"][name].append(P.hf_energy_ratio(MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(sr_img), radius_frac=radius_frac))
            stats["kl_luma"][name].append(P.kl_divergence(MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(sr_img)))
            stats["kl_color"][name].append(P.kl_divergence_color(hr_img, sr_img))
        hr_g, lr_g = MR.rgb2gray_u8(hr_img), MR.rgb2gray_u8(lr_img)
        outs["ibp"] = run("ibp", lambda: CA.back_projection(hr_g, lr_g, iterations=iterations))
        outs["nlm"] = run("nlm", lambda: CA.non_local_means(hr_g, lr_g))
        outs["egi"] = run("egi", lambda: CA.edge_guided_interpolation(hr_g, lr_g))
        f = run("freq", lambda: CA.frequency_extrapolation(hr_g, lr_g))
        outs["freq"] = (f / np.max(f) * 255.0).astype(np.uint8) if np.max(f) > 0 else f.astype(np.uint8)
        outs["freq_max"] = float(np.max(f))
        dr_nlm = hr_g.max() - hr_g.min() if hr_g.max() != hr_g.min() else 255.0
        for name in ("ibp", "nlm", "egi", "freq"):
            sr_g = outs[name]
            dr = dr_nlm if name == "nlm" else 255.0
            stats["psnr"][name].append(psnr(hr_g, sr_g, data_range=dr))
            stats["ssim"][name].append(ssim(hr_g, sr_g, data_range=dr))
            stats["mae"][name].append(P.mae(hr_g, sr_g))
            stats["rmse"][name].append(P.rmse(hr_g, sr_g))
            stats["gradient_mse"][name].append(P.gradient_mse(hr_g, sr_g))
            stats["epi"][name].append(P.epi(hr_g, sr_g))
            stats["hf_energy_ratio"][name].append(P.hf_energy_ratio(hr_g, sr_g, radius_frac=radius_frac))
            stats["kl_luma"][name].append(P.kl_divergence(hr_g, sr_g))
            stats["kl_color"][name].append(np.nan)
        outs["hr_g"], outs["lr_g"] = hr_g, lr_g
        all_outs.append(outs)
    return stats, all_outs
