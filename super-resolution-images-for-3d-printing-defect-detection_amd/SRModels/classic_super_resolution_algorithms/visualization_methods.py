"""The numeric halves of the reference's classic_super_resolution_algorithms/visualization_methods.py, the module that draws the classical
study's figures.

Built: `ssim_similarity_maps` (the `(ssim_map, val)` pairs plot_and_save_ssim_similarity_maps draws, :553-591, on the device: one batched
gray conversion and one sr_ssim_map launch over the eight pairs), `super_resolution_example` (the ten titled images of
plot_and_save_super_resolution_example, :517-551) and `ranking_contributions` (the ranking and the weight x normalised-value matrix
show_algorithm_ranking draws, :617-689, on the host in NumPy).
Not built: every matplotlib panel -- the `plot_*` functions and `show_algorithm_ranking` raise NotImplementedError and name the numeric
function.  Importing this module touches no device; only ssim_similarity_maps needs one.
"""
from collections import OrderedDict

import numpy as np

from .profiling_methods import rank_algorithms

SSIM_MAP_NAMES = ("Bilinear", "Bicubic", "Area", "Lanczos", "IBP", "NLM", "EGI", "FREQ")
EXAMPLE_TITLES = ("HR", "LR") + SSIM_MAP_NAMES


def _unpack(vis, ibp_example, nlm_example, egi_example, freq_example):
    hr_img_v, lr_img_v, bilinear_v, bicubic_v, area_v, lanczos_v = vis
    hr_g_v, _lr_g_v, ibp_v = ibp_example
    hr_v, nlm_v = nlm_example
    hr_egi_v, _lr_egi_v, egi_v = egi_example
    hr_freq_v, freq_v = freq_example
    return (hr_img_v, lr_img_v, bilinear_v, bicubic_v, area_v, lanczos_v), (hr_g_v, ibp_v), (hr_v, nlm_v), (hr_egi_v, egi_v), (hr_freq_v, freq_v)


def super_resolution_example(vis, ibp_example, nlm_example, egi_example, freq_example):
    """The ten (title, image) pairs plot_and_save_super_resolution_example shows (:517-551), its to_display applied: a 2-D float32 image is
    clipped to [0, 1], every other image is shown as it is."""
    (hr_img, lr_img, bilinear, bicubic, area, lanczos), (_, ibp), (_, nlm), (_, egi), (_, freq) = _unpack(vis, ibp_example, nlm_example, egi_example,
                                                                                                        freq_example)

    def to_display(img):
        img = np.asarray(img)
        if img.ndim == 2 and img.dtype == np.float32:
            return np.clip(img, 0, 1)
        return img

    return [(t, to_display(im)) for t, im in zip(EXAMPLE_TITLES, (hr_img, lr_img, bilinear, bicubic, area, lanczos, ibp, nlm, egi, freq))]


def ssim_maps_device(vis, ibp_example, nlm_example, egi_example, freq_example):
    """ssim_similarity_maps without its read: (S float64 [8,H,W], mssim float64 [8]) on the device, in SSIM_MAP_NAMES' order."""
    import torch
    from sr355 import Context
    ctx = Context.get()
    (hr_img, _, bilinear, bicubic, area, lanczos), (hr_g, ibp), (hr_n, nlm), (hr_e, egi), (hr_f, freq) = _unpack(vis, ibp_example, nlm_example,
                                                                                                              egi_example, freq_example)

    def dev(x, who):
        if not isinstance(x, torch.Tensor):
            x = np.asarray(x)
            x = torch.from_numpy(np.ascontiguousarray(x.astype(np.float32) if x.dtype == np.float64 else x))
        if x.dtype == torch.float64:
            x = x.to(torch.float32)
        if x.dtype not in (torch.uint8, torch.float32) or x.dim() not in (2, 3) or (x.dim() == 3 and x.shape[2] != 3):
            raise NotImplementedError(f"ssim_similarity_maps: {who} must be a uint8 or float [H,W] or [H,W,3] image")
        if x.dim() == 3 and x.dtype != torch.uint8:
            raise NotImplementedError(f"ssim_similarity_maps: {who} is a float RGB image, which has no gray image here (only uint8 RGB goes "
                                      "through COLOR_RGB2GRAY)")
        return x.to(ctx.torch_device).contiguous()

    rgb_names = ("HR", "Bilinear", "Bicubic", "Area", "Lanczos")
    firsts = [dev(x, n) for n, x in zip(rgb_names, (hr_img, bilinear, bicubic, area, lanczos))]
    if len({tuple(x.shape) for x in firsts}) != 1:
        raise ValueError("ssim_similarity_maps: the example's images differ in size")
    if firsts[0].dim() == 3:
        grays = list(ctx.rgb2gray(torch.stack(firsts)))                 # to_gray of the five RGB images: one launch
    else:
        grays = firsts
    hrs = [grays[0]] * 4 + [dev(x, "an HR image") for x in (hr_g, hr_n, hr_e, hr_f)]
    srs = grays[1:] + [dev(x, n) for n, x in zip(SSIM_MAP_NAMES[4:], (ibp, nlm, egi, freq))]
    if any(x.dim() != 2 for x in hrs[4:] + srs[4:]):
        raise NotImplementedError("ssim_similarity_maps: the gray examples must be 2-D images, as the notebook collects them")
    if len({tuple(x.shape) for x in hrs + srs}) != 1:
        raise ValueError("ssim_similarity_maps: the example's images differ in size")
    data_range = [1.0 if h.dtype == torch.float32 else 255.0 for h in hrs]

    def side(imgs):                                                     # one dtype per side of the launch: float(uint8) is exact, and so are its window sums
        if all(x.dtype == torch.uint8 for x in imgs):
            return torch.stack(imgs)
        return torch.stack([x.to(torch.float32) for x in imgs])

    return ctx.ssim_map(side(hrs), side(srs), np.asarray(data_range))


def ssim_similarity_maps(vis, ibp_example, nlm_example, egi_example, freq_example):
    """The similarity maps of plot_and_save_ssim_similarity_maps (:553-591): an ordered mapping name -> (ssim_map float64 [H,W], val) for
    Bilinear, Bicubic, Area, Lanczos, IBP, NLM, EGI, FREQ, each skimage's structural_similarity(hr, sr, data_range=..., full=True) with
    the reference's to_gray (uint8 RGB through COLOR_RGB2GRAY) and its data-range rule: 255 unless the HR image is float32, then 1.0 -- so
    the NLM pair is uint8 HR against a [0, 1] float SR at range 255, as the reference computes it.  NumPy arrays or device tensors; all
    eight pairs must have one size.  Two launches (the RGB images' gray conversion, the eight maps) and one read."""
    import torch
    smap, mean = ssim_maps_device(vis, ibp_example, nlm_example, egi_example, freq_example)
    host = torch.cat([smap.reshape(-1), mean]).cpu().numpy()            # the one read
    maps = host[:smap.numel()].reshape(tuple(smap.shape))
    vals = host[smap.numel():]
    return OrderedDict((n, (maps[i].copy(), float(vals[i]))) for i, n in enumerate(SSIM_MAP_NAMES))


def _metric_value(stats, metric):
    if metric in ("psnr_ci_width", "ssim_ci_width"):
        lo, hi = stats.get(metric[:4] + "_ci_low", np.nan), stats.get(metric[:4] + "_ci_high", np.nan)
        return float(hi - lo) if np.isfinite(lo) and np.isfinite(hi) else np.nan
    if metric in ("epi_dev", "hf_ratio_dev"):
        v = stats.get(metric[:-4] + "_mean", np.nan)
        return float(abs(v - 1.0)) if np.isfinite(v) else np.nan
    return stats.get(metric, np.nan)


def ranking_contributions(metric_summary, maximize=None, minimize=None, weights=None):
    """What show_algorithm_ranking draws (:617-689): (ranked, scores, bounds) of rank_algorithms, the metrics it used (the keys of bounds, in
    order) and contrib float64 [algorithm in ranked order, metric] = weight x the metric's normalised value -- (v - lo) / (hi - lo) for a
    metric to maximise, (hi - v) / (hi - lo) otherwise, clipped to [0, 1]; 0 for a value that is not finite and for a metric without spread.
    Weights default to equal shares, a metric missing from `weights` weighs 0.  Host NumPy; a row of contrib sums to the algorithm's score."""
    ranked, scores, bounds = rank_algorithms(metric_summary, maximize=maximize, minimize=minimize, weights=weights)
    alg_order = [alg for alg, _ in ranked]
    metrics = list(bounds.keys())
    if maximize is not None or minimize is not None:
        max_set, min_set = set(maximize or []), set(minimize or [])
    else:
        max_set = {m for m in metrics if m in ("psnr_mean", "psnr_max", "ssim_mean", "ssim_max")}
        min_set = {m for m in metrics if m not in max_set}
    if weights is None:
        weights_used = dict.fromkeys(metrics, 1.0 / max(1, len(metrics)))
    else:
        weights_used = {m: float(weights.get(m, 0.0)) for m in metrics}
    contrib = np.zeros((len(alg_order), len(metrics)), dtype=float)
    for j, m in enumerate(metrics):
        lo, hi = bounds[m]
        for i, alg in enumerate(alg_order):
            val = _metric_value(metric_summary[alg], m)
            norm = 0.0
            if np.isfinite(val) and np.isfinite(lo) and np.isfinite(hi) and hi - lo != 0:
                norm = (val - lo) / (hi - lo) if (m in max_set and m not in min_set) else (hi - val) / (hi - lo)
                norm = float(np.clip(norm, 0.0, 1.0))
            contrib[i, j] = weights_used[m] * norm
    return ranked, scores, bounds, metrics, contrib


def _not_built(name, numeric):
    def plot(*args, **kwargs):
        raise NotImplementedError(f"{name}: the matplotlib panel is not built; its numbers are {numeric}(...)")
    plot.__name__ = name
    plot.__doc__ = f"Not built (a matplotlib panel).  The numbers it draws: {numeric}."
    return plot


_SUMMARY = "profiling_methods.build_metrics_summary"
plot_time_memory_panels = _not_built("plot_time_memory_panels", _SUMMARY)
plot_psnr_ssim_panels = _not_built("plot_psnr_ssim_panels", _SUMMARY)
plot_speed_quality_tradeoff_3d = _not_built("plot_speed_quality_tradeoff_3d", _SUMMARY)
plot_error_metrics_grid = _not_built("plot_error_metrics_grid", _SUMMARY)
plot_edge_metrics_grid = _not_built("plot_edge_metrics_grid", _SUMMARY)
plot_frequency_distribution_metrics_grid = _not_built("plot_frequency_distribution_metrics_grid", _SUMMARY)
plot_and_save_super_resolution_example = _not_built("plot_and_save_super_resolution_example", "super_resolution_example")
plot_and_save_ssim_similarity_maps = _not_built("plot_and_save_ssim_similarity_maps", "ssim_similarity_maps")
show_algorithm_ranking = _not_built("show_algorithm_ranking", "ranking_contributions")
