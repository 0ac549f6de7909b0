"""The classical study's profiling and scoring helpers (reference: classic_super_resolution_algorithms/profiling_methods.py), with the
per-image metrics on the MI355X (csrc/metrics.hip, sr_classic_scores) and the summary / ranking helpers on the host in NumPy.

Per-image metrics take uint8 or float images, [H, W] or [H, W, 3] (float64 is cast to float32, lossless for the notebook's data), H and
W >= 7, and return Python floats:
  mae, rmse                  over every channel as passed (rmse = sqrt(mean(d^2) + 1e-9));
  sobel_mag -> float32 array, gradient_mse, epi
                             on the gray image, divided by 255 when its own max > 1.5 (each image decides for itself); the gray image of
                             uint8 RGB is OpenCV's fixed-point COLOR_RGB2GRAY, (4899 R + 9617 G + 1868 B + 8192) >> 14;
  hf_energy_ratio            on 2-D images, the unscaled values: masked |fftshift(fft2)| sums, r > radius_frac (r_max + 1e-9);
  kl_divergence              on 2-D images, 256-bin histograms; kl_divergence_color on RGB, 64 bins per channel.
A float RGB image passed to a gray-derived metric raises NotImplementedError (the notebook never passes one), as does any other bin count.
score_pairs scores stacked pairs in one batch (NumPy arrays or device tensors).  peak_signal_noise_ratio and structural_similarity are
drop-ins for skimage.metrics' functions with their default window (the notebook's skimage import can point here).

time_algorithm (wall clock) and memory_algorithm (tracemalloc peak of the host heap) keep the reference's semantics; the device metrics
return synchronized host values, so a wall clock around them covers the device work.  The GPU is touched only when a device metric runs:
importing this module and the host helpers need none."""
import time
import tracemalloc

import numpy as np

DEF_EPS = 1e-9

MAXIMIZE_DEFAULT = ['psnr_mean', 'ssim_mean']
MINIMIZE_DEFAULT = ['time_mean', 'memory_mean', 'mae_mean', 'rmse_mean']

SCORE_NAMES = ("psnr", "ssim", "mae", "rmse", "grad_mse", "epi", "hf_ratio", "kl_luma", "kl_color")


# ------------------------------------------------------------------ timing / memory (host)
def time_algorithm(func, *args, **kwargs):
    """(func(*args, **kwargs), wall-clock seconds of the call)."""
    t0 = time.perf_counter()
    out = func(*args, **kwargs)
    return out, time.perf_counter() - t0


def memory_algorithm(func, *args, **kwargs):
    """(func(*args, **kwargs), peak bytes tracemalloc saw on the host heap during the call)."""
    tracemalloc.start()
    out = func(*args, **kwargs)
    _, peak = tracemalloc.get_traced_memory()
    tracemalloc.stop()
    return out, peak


# ------------------------------------------------------------------ device scoring
def _context():
    from sr355 import Context                  # loaded on first use: the host helpers run without a GPU
    return Context.get()


def _image(a, name):
    a = np.asarray(a)
    if a.dtype == np.float64:
        a = a.astype(np.float32)
    if a.dtype not in (np.uint8, np.float32):
        raise NotImplementedError(f"{name}: dtype {a.dtype} is not scored here (uint8 or float images)")
    if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
        raise NotImplementedError(f"{name}: expected an [H, W] or [H, W, 3] image, got shape {a.shape}")
    return a


def _gray_capable(a, metric):
    if a.ndim == 3 and a.dtype != np.uint8:
        raise NotImplementedError(f"{metric}: a float RGB image has no gray image here (only uint8 RGB goes through COLOR_RGB2GRAY)")


def score_pairs(hr_imgs, sr_imgs, data_range=255.0, radius_frac=0.6):
    """Score stacked pairs [B, H, W] or [B, H, W, 3] in one device batch -> {column name: [B] scores}.  NumPy in, NumPy out; device
    tensors in, device fp64 tensors out (nothing leaves the device).  data_range: a number, a [B] array, or 'hr_span' (max(hr) - min(hr),
    255 when that is 0: the notebook's NL-means rule).  For float RGB pairs the gray-derived columns are NaN."""
    import torch
    ctx = _context()
    if isinstance(hr_imgs, torch.Tensor) and isinstance(sr_imgs, torch.Tensor):
        s = ctx.classic_scores(hr_imgs.contiguous(), sr_imgs.contiguous(), data_range, radius_frac)
        return {k: s[:, i] for i, k in enumerate(SCORE_NAMES)}
    hr = np.asarray(hr_imgs)
    sr = np.asarray(sr_imgs)
    hr = hr.astype(np.float32) if hr.dtype == np.float64 else hr
    sr = sr.astype(np.float32) if sr.dtype == np.float64 else sr
    if hr.dtype not in (np.uint8, np.float32) or sr.dtype not in (np.uint8, np.float32):
        raise NotImplementedError(f"score_pairs: dtypes {hr.dtype} / {sr.dtype} are not scored here (uint8 or float images)")
    if not isinstance(data_range, str) and np.ndim(data_range) > 0:
        data_range = np.asarray(data_range, dtype=np.float64)
    s = ctx.classic_scores(ctx.to_device(hr), ctx.to_device(sr), data_range, radius_frac).cpu().numpy()
    return {k: s[:, i] for i, k in enumerate(SCORE_NAMES)}


def _score(hr, sr, column, data_range=255.0, radius_frac=0.6, gray=False):
    a, b = _image(hr, column), _image(sr, column)
    if a.shape != b.shape:
        raise ValueError(f"{column}: images of shapes {a.shape} and {b.shape}")
    if gray:
        _gray_capable(a, column)
        _gray_capable(b, column)
    return float(score_pairs(a[None], b[None], data_range, radius_frac)[column][0])


def mae(a, b):
    """Mean absolute error over every channel, values as passed."""
    return _score(a, b, "mae")


def rmse(a, b):
    """sqrt(mean squared error + 1e-9) over every channel, values as passed."""
    return _score(a, b, "rmse")


def sobel_mag(img):
    """ksize-3 Sobel magnitude (BORDER_REFLECT_101) of the gray image, divided by 255 first when its max > 1.5 -> float32 [H, W]."""
    a = _image(img, "sobel_mag")
    _gray_capable(a, "sobel_mag")
    ctx = _context()
    x = ctx.to_device(a[None])
    _, raw = ctx.classic_scores(x, x, raw=True)
    return raw["sobel"][0, 0].cpu().numpy()


def gradient_mse(hr, sr):
    """Mean squared difference of the two images' Sobel magnitudes."""
    return _score(hr, sr, "grad_mse", gray=True)


def epi(hr, sr):
    """Edge preservation index: (sum of SR's Sobel magnitudes + 1e-9) / (HR's + 1e-9)."""
    return _score(hr, sr, "epi", gray=True)


def hf_energy_ratio(hr, sr, radius_frac=0.6):
    """High-frequency energy ratio of two gray images: masked |fftshift(fft2)| sum of SR over HR's."""
    if np.ndim(hr) != 2:
        raise NotImplementedError("hf_energy_ratio: 2-D (gray) images only, as the notebook passes them")
    return _score(hr, sr, "hf_ratio", radius_frac=radius_frac, gray=True)


def kl_divergence(p_img, q_img, bins=256):
    """KL divergence of the 256-bin gray histograms of p (HR) and q (SR)."""
    if bins != 256:
        raise NotImplementedError("kl_divergence: the device histograms have 256 bins")
    if np.ndim(p_img) != 2:
        raise NotImplementedError("kl_divergence: 2-D (gray) images only, as the notebook passes them")
    return _score(p_img, q_img, "kl_luma", gray=True)


def kl_divergence_color(p_rgb, q_rgb, bins=64):
    """Per-channel KL divergence of 64-bin histograms, averaged over the three channels."""
    if bins != 64:
        raise NotImplementedError("kl_divergence_color: the device histograms have 64 bins per channel")
    if np.ndim(p_rgb) != 3:
        raise NotImplementedError("kl_divergence_color: [H, W, 3] images only")
    return _score(p_rgb, q_rgb, "kl_color")


# ------------------------------------------------------------------ skimage.metrics drop-ins (default window only)
def _skimage_range(image, data_range, fn):
    if data_range is not None:
        return float(data_range)
    if np.asarray(image).dtype == np.uint8:
        return 255.0
    raise NotImplementedError(f"{fn}: pass data_range for float images")


def peak_signal_noise_ratio(image_true, image_test, *, data_range=None, **kwargs):
    """skimage.metrics.peak_signal_noise_ratio: 10 log10(data_range^2 / MSE)."""
    if kwargs:
        raise NotImplementedError(f"peak_signal_noise_ratio: {sorted(kwargs)} not supported")
    return _score(image_true, image_test, "psnr", _skimage_range(image_true, data_range, "peak_signal_noise_ratio"))


def structural_similarity(im1, im2, *, data_range=None, channel_axis=None, full=False, **kwargs):
    """skimage.metrics.structural_similarity with its default window (7 x 7 uniform, sample covariance, K1 0.01, K2 0.03): 2-D images,
    or [H, W, 3] with channel_axis 2 / -1 (the mean of the per-channel means).  full=True -> (mssim, S) as skimage returns them: S the
    float64 similarity map of the images' shape, the window means at the border by scipy's 'reflect' rule (sr_ssim_map)."""
    if kwargs:
        raise NotImplementedError(f"structural_similarity: {sorted(kwargs)} not supported (default window only)")
    nd = np.ndim(im1)
    if not ((channel_axis is None and nd == 2) or (channel_axis in (2, -1) and nd == 3)):
        raise NotImplementedError("structural_similarity: 2-D images, or [H, W, 3] with channel_axis=2")
    dr = _skimage_range(im1, data_range, "structural_similarity")
    if not full:
        return _score(im1, im2, "ssim", dr)
    a, b = _image(im1, "ssim"), _image(im2, "ssim")
    if a.shape != b.shape:
        raise ValueError(f"ssim: images of shapes {a.shape} and {b.shape}")
    ctx = _context()
    smap, mean = ctx.ssim_map(ctx.to_device(a[None]), ctx.to_device(b[None]), dr)
    return float(mean[0]), smap[0].cpu().numpy()


# ------------------------------------------------------------------ statistics, bootstrap and ranking (host)
def bootstrap_ci(values, n_boot=1000, ci=0.95, seed=42):
    """Percentile bootstrap interval of the mean: n_boot resamples with replacement (numpy default_rng(seed)); (NaN, NaN) below 2 values."""
    if len(values) < 2:
        return (np.nan, np.nan)
    v = np.asarray(values)
    rng = np.random.default_rng(seed)
    means = [rng.choice(v, size=len(v), replace=True).mean() for _ in range(n_boot)]
    return (float(np.percentile(means, (1.0 - ci) / 2.0 * 100.0)), float(np.percentile(means, (1.0 + ci) / 2.0 * 100.0)))


def compute_summary_stats(values):
    """mean, median, max, sample std / var (ddof 1; 0.0 for a single value) and count of a 1-D list of numbers."""
    n = len(values)
    return {
        'mean': float(np.mean(values)),
        'median': float(np.median(values)),
        'max': float(np.max(values)),
        'std': float(np.std(values, ddof=1)) if n > 1 else 0.0,
        'var': float(np.var(values, ddof=1)) if n > 1 else 0.0,
        'count': int(n),
    }


def build_metrics_summary(time_stats, memory_stats, psnr_stats, ssim_stats, mae_stats, rmse_stats, gradient_mse_stats, epi_stats,
                          hf_energy_ratio_stats, kl_luma_stats, kl_color_stats):
    """Per algorithm (the keys of time_stats): means / maxima / variances of the collected per-image lists, the time jitter
    (std / mean), and bootstrap intervals of the PSNR and SSIM means.  Pure: nothing passed in is modified."""
    summary = {}
    for alg in time_stats:
        t = time_stats.get(alg, [])
        m = memory_stats.get(alg, [])
        jitter = t_var = m_var = np.nan
        if len(t) > 1 and np.mean(t) > 0:
            jitter = float(np.std(t, ddof=1) / np.mean(t))
            t_var = float(np.var(t, ddof=1))
        if len(m) > 1:
            m_var = float(np.var(m, ddof=1))
        st = {name: compute_summary_stats(src.get(alg, [])) for name, src in (
            ('time', time_stats), ('memory', memory_stats), ('psnr', psnr_stats), ('ssim', ssim_stats), ('mae', mae_stats),
            ('rmse', rmse_stats), ('grad', gradient_mse_stats), ('epi', epi_stats), ('hf', hf_energy_ratio_stats),
            ('kl_luma', kl_luma_stats), ('kl_color', kl_color_stats))}
        p_lo, p_hi = bootstrap_ci(psnr_stats[alg])
        s_lo, s_hi = bootstrap_ci(ssim_stats[alg])
        summary[alg] = {
            'psnr_mean': st['psnr']['mean'], 'psnr_var': st['psnr']['var'], 'psnr_max': st['psnr']['max'],
            'psnr_ci_low': p_lo, 'psnr_ci_high': p_hi,
            'ssim_mean': st['ssim']['mean'], 'ssim_var': st['ssim']['var'], 'ssim_max': st['ssim']['max'],
            'ssim_ci_low': s_lo, 'ssim_ci_high': s_hi,
            'time_mean': st['time']['mean'], 'time_max': st['time']['max'], 'time_jitter': jitter, 'time_var': t_var,
            'memory_mean': st['memory']['mean'], 'memory_max': st['memory']['max'], 'memory_var': m_var,
            'mae_mean': st['mae']['mean'], 'mae_max': st['mae']['max'],
            'rmse_mean': st['rmse']['mean'], 'rmse_max': st['rmse']['max'],
            'grad_mse_mean': st['grad']['mean'], 'epi_mean': st['epi']['mean'], 'hf_ratio_mean': st['hf']['mean'],
            'kl_luma_mean': st['kl_luma']['mean'], 'kl_color_mean': st['kl_color']['mean'],
        }
    return summary


_DERIVED = {
    'psnr_ci_width': lambda s: _width(s, 'psnr'),
    'ssim_ci_width': lambda s: _width(s, 'ssim'),
    'epi_dev': lambda s: _dev_from_one(s.get('epi_mean', np.nan)),
    'hf_ratio_dev': lambda s: _dev_from_one(s.get('hf_ratio_mean', np.nan)),
}


def _width(stats, prefix):
    lo, hi = stats.get(prefix + '_ci_low', np.nan), stats.get(prefix + '_ci_high', np.nan)
    return float(hi - lo) if np.isfinite(lo) and np.isfinite(hi) else np.nan


def _dev_from_one(v):
    return float(abs(v - 1.0)) if np.isfinite(v) else np.nan


def _metric(stats, name):
    return _DERIVED[name](stats) if name in _DERIVED else stats.get(name, np.nan)


def rank_algorithms(summary, maximize=None, minimize=None, weights=None):
    """Weighted min-max score per algorithm -> (ranked [(alg, score)] best first, {alg: score}, {metric: (min, max)}).

    Each metric is normalised over the algorithms' finite values to [0, 1] (higher is better: (v - lo) / (hi - lo) for `maximize`,
    (hi - v) / (hi - lo) for `minimize`); NaN values and metrics without spread contribute 0.  Weights default to equal shares.
    With both lists None the metrics are picked from what the summary holds: PSNR / SSIM means and maxima to maximise; time, memory,
    error, variance and KL figures, the bootstrap interval widths (psnr_ci_width, ssim_ci_width) and |epi_mean - 1|, |hf_ratio_mean - 1|
    (epi_dev, hf_ratio_dev) to minimise.  Otherwise the given lists are used as they are."""
    if maximize is None and minimize is None:
        present = set().union(*(st.keys() for st in summary.values())) if summary else set()
        maximize = [m for m in ('psnr_mean', 'psnr_max', 'ssim_mean', 'ssim_max') if m in present]
        minimize = [m for m in ('time_mean', 'time_max', 'time_jitter', 'time_var', 'memory_mean', 'memory_max', 'memory_var',
                                'mae_mean', 'mae_max', 'rmse_mean', 'rmse_max', 'grad_mse_mean', 'kl_luma_mean', 'kl_color_mean',
                                'psnr_var', 'ssim_var') if m in present]
        for prefix in ('psnr', 'ssim'):
            if prefix + '_ci_low' in present and prefix + '_ci_high' in present:
                minimize.append(prefix + '_ci_width')
        if 'epi_mean' in present:
            minimize.append('epi_dev')
        if 'hf_ratio_mean' in present:
            minimize.append('hf_ratio_dev')
    else:
        maximize, minimize = list(maximize or []), list(minimize or [])
    metrics = list(dict.fromkeys(list(maximize) + list(minimize)))

    bounds = {}
    for m in metrics:
        v = np.array([_metric(st, m) for st in summary.values()], dtype=float)
        v = v[np.isfinite(v)]
        bounds[m] = (float(v.min()), float(v.max())) if v.size else (np.nan, np.nan)
    if weights is None:
        weights = dict.fromkeys(metrics, 1.0 / max(1, len(metrics)))

    scores = {}
    for alg, st in summary.items():
        total = 0.0
        for m in metrics:
            v = _metric(st, m)
            lo, hi = bounds[m]
            norm = 0.0
            if np.isfinite(v) and np.isfinite(lo) and np.isfinite(hi) and hi - lo != 0:
                norm = (v - lo) / (hi - lo) if m in maximize else (hi - v) / (hi - lo)
                norm = float(np.clip(norm, 0.0, 1.0))
            total += weights.get(m, 0.0) * norm
        scores[alg] = total
    ranked = sorted(scores.items(), key=lambda kv: kv[1], reverse=True)
    return ranked, scores, bounds
