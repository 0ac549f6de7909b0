"""The dataset EDA (reference: data/EDA.ipynb -- ImagePairLoader, ImageDatasetAnalyzer, ImagePairMetrics, MetricsAggregator,
StatsReporter, ImageDataVisualization, run_eda_pipeline), with every per-pair statistic, global accumulator and per-pair panel map on
the MI355X (csrc/eda.hip: sr_eda_pair_stats, sr_eda_accumulate, sr_eda_pair_panels) and the bookkeeping on the host in NumPy.  A notebook imports these names instead of defining the cells; cv2, scikit-image, scipy and
pandas are not needed.

Images are uint8 BGR [H, W, 3] as cv2.imread returns them (files are decoded through PIL and the channel order restored), gray images
uint8 [H, W].  The single-image methods take NumPy arrays and return Python floats / dicts.  The device derives the gray and HSV planes
from the BGR image itself, so the methods that the reference hands a precomputed plane (feature_distribution(img, hsv),
detect_artifacts(img, gray)) check that plane against the device's and raise ValueError on a mismatch; rms_noise, laplacian_variance
and glcm_features, which receive only a gray image, run on it as a BGR image with three equal channels (its COLOR_BGR2GRAY is itself).
The OpenCV 8-bit semantics (gray, Gaussian blurs, HSV, Canny, dilation) are the contract stated in include/sr355.h.
Each single-image method scores the pair (img, img) through the whole device pipeline (classic scores, Canny, GLCM, both DCTs) to
return its one number or dict: fine for a notebook cell, wasteful in a loop -- collect / collect_arrays make one pass per batch and are
the way to score a dataset.

LPIPS needs the user's two checkpoints (torchvision's AlexNet and the lpips package's alex.pth; they exist nowhere this project runs, as
VGG16's and VGG19's do not): after ImageDatasetAnalyzer.load_lpips(alexnet_path, lpips_path) the device scores it (csrc/lpips.hip,
Context.lpips) -- lpips_score returns the float, collect / collect_arrays fill the rows' lpips column in the same batch pass, loss_fn()
returns the scoring callable and StatsReporter.lpips_scenarios gives the pipeline's best / worst file names.  The loaded state is
process-wide and nothing loads it implicitly; until then, and after unload_lpips(), the lpips column is NaN and lpips_score and loss_fn
raise NotImplementedError.

ImageDataVisualization is the numeric half of the notebook's plots: visual_example / advanced_panel / advanced_panels return the maps
of one pair or a stack from the device (the spectra as np.log(mag + 1e-8) of the device's magnitudes, taken here), global_advanced_panel
and the *_data methods return the numbers under the global panel and the seven table plots in host NumPy on collect's global_data and
StatsReporter.dataframe's columns (no pandas, scipy, seaborn or matplotlib).  run_eda_panels returns (df, panels); run_eda_pipeline has
the reference's signature, returns df and writes each panel as an .npz where the reference writes the .png of the same stem.  Ranking
the examples by lpips needs load_lpips; rank_by names another column.  Out of scope: the drawing itself -- the plotting names
(save_visual_example, create_advanced_visualizations, basic_distributions, ...) raise NotImplementedError naming the numeric method --
PNG writing and OpenCV's JET colour map.  Importing this module and its host helpers (ImagePairLoader.iter_pairs, ImagePairMetrics,
StatsReporter, ImageDataVisualization's *_data methods and global_advanced_panel) needs no GPU."""
import math
import os

import numpy as np

ANGLES = (0.0, math.pi / 4, math.pi / 2, 3 * math.pi / 4)
SAT_BINS = np.linspace(0, 256, 51)
# OpenCV interpolation names the device resize does not offer for uint8 images
_INTERP_KNOWN_NOT_OFFERED = ("INTER_LINEAR_EXACT", "INTER_NEAREST_EXACT", "INTER_BITS", "INTER_BITS2", "INTER_MAX")


def _context():
    from sr355 import Context                  # loaded on first use: the host helpers run without a GPU
    return Context.get()


def _row_columns():
    from sr355 import _lib
    return _lib.EDA_ROW_COLUMNS


def _bgr(img, name):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise NotImplementedError(f"{name}: expected a uint8 BGR image [H, W, 3], got {a.dtype} {a.shape} (the EDA reads 8-bit BGR files only)")
    return np.ascontiguousarray(a)


def _gray(gray, name):
    a = np.asarray(gray)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise NotImplementedError(f"{name}: expected a uint8 gray image [H, W], got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _angle_indices(angles, multi_angle):
    if angles is None:
        return (0, 1, 2, 3) if multi_angle else (0,)
    out = []
    for a in angles:
        hit = [i for i, s in enumerate(ANGLES) if abs(float(a) - s) < 1e-9]
        if not hit:
            raise NotImplementedError(f"glcm_features: angle {a!r} is not one of 0, pi/4, pi/2, 3 pi/4")
        out.append(hit[0])
    if len(set(out)) != len(out):
        raise NotImplementedError("glcm_features: repeated angles are not offered")
    return tuple(out)


def _single(img, levels=64, angles=(0,), raw=False):
    """One image scored as the pair (img, img): -> ({stat name: float}, raw dict of NumPy planes or None)."""
    ctx = _context()
    x = ctx.to_device(img[None])
    res = ctx.eda_pair_stats(x, x, levels, angles, raw=raw)
    stats, inter = res if raw else (res, None)
    vals = dict(zip(ctx.EDA_STAT_NAMES, (float(v) for v in stats[0].cpu().numpy())))
    return vals, (None if inter is None else {k: v[0].cpu().numpy() for k, v in inter.items()})


class ImagePairLoader:
    """Iterating and aligning LR / HR pairs."""

    @staticmethod
    def iter_pairs(lr_base, hr_base):
        """Yields (lr_relpath, hr_relpath) for every .png / .jpg / .jpeg present under both trees, in lexicographic order."""
        exts = (".png", ".jpg", ".jpeg")

        def rel(base):
            return {os.path.relpath(os.path.join(root, f), base) for root, _, files in os.walk(base) for f in files if f.lower().endswith(exts)}

        common = sorted(rel(lr_base) & rel(hr_base))
        if not common:
            raise ValueError("No matching LR/HR image pairs were found under the provided directories.")
        for r in common:
            yield r, r

    @staticmethod
    def read_bgr(path):
        """cv2.imread's array for an 8-bit colour file: uint8 [H, W, 3], BGR (decoded through PIL, channel order restored)."""
        from PIL import Image
        try:
            with Image.open(path) as im:
                return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1])
        except OSError as e:
            raise ValueError(f"Failed reading {path}") from e

    @staticmethod
    def interpolation_for(lr_path, interp_map=None):
        """The interpolation name load_and_align uses for this file: the map's entry when it is one the reference knows, else INTER_LINEAR."""
        name = None if interp_map is None else interp_map.get(os.path.basename(lr_path))
        if name in _INTERP_KNOWN_NOT_OFFERED:
            raise NotImplementedError(f"interpolation {name} is not offered by the device resize for uint8 images")
        return name if name in ("INTER_LINEAR", "INTER_CUBIC", "INTER_AREA", "INTER_LANCZOS4") else "INTER_LINEAR"

    @staticmethod
    def load_and_align(lr_path, hr_path, interp_map=None):
        """Reads both images and resizes LR to HR's size on the device when they differ -> (lr, hr) uint8 BGR."""
        lr, hr = ImagePairLoader.read_bgr(lr_path), ImagePairLoader.read_bgr(hr_path)
        if lr.shape[:2] != hr.shape[:2]:
            ctx = _context()
            lr = ctx.resize(ctx.to_device(lr[None]), hr.shape[0], hr.shape[1], ImagePairLoader.interpolation_for(lr_path, interp_map))[0].cpu().numpy()
        return lr, hr


class ImageDatasetAnalyzer:
    """The reference's static per-image metrics."""

    _lpips_ctx = None      # the context whose LPIPS weights load_lpips set; None: not loaded

    @staticmethod
    def load_lpips(alexnet_path, lpips_path=None):
        """Reads torchvision's AlexNet checkpoint and the lpips package's alex.pth (or one .npz holding both: sr355.lpips.load_weights)
        and sets them on the device: from here on lpips_score, loss_fn and the rows' lpips column are served.  Process-wide."""
        from sr355.lpips import load_weights
        w = load_weights(alexnet_path, lpips_path)
        ctx = _context()
        ctx.lpips_set_weights(w)
        ImageDatasetAnalyzer._lpips_ctx = ctx

    @staticmethod
    def unload_lpips():
        ctx, ImageDatasetAnalyzer._lpips_ctx = ImageDatasetAnalyzer._lpips_ctx, None
        if ctx is not None:
            ctx.lpips_set_weights(None)

    @staticmethod
    def loss_fn():
        """The reference's name for the LPIPS model: a callable scoring two float tensors [B,3,H,W] in [-1, 1] (lpips_score's to_tensor
        form) -> float32 [B,1,1,1] on the device.  NotImplementedError until load_lpips."""
        ctx = ImageDatasetAnalyzer._lpips_ctx
        if ctx is None:
            raise NotImplementedError("loss_fn: LPIPS needs torchvision's AlexNet checkpoint and the lpips package's alex.pth: call "
                                      "ImageDatasetAnalyzer.load_lpips(alexnet_path, lpips_path) first")

        def score(a, b):
            import torch
            nhwc = lambda t: ctx.to_device(torch.as_tensor(t), torch.float32).permute(0, 2, 3, 1).contiguous()
            return ctx.lpips(nhwc(a), nhwc(b)).reshape(-1, 1, 1, 1)

        return score

    @staticmethod
    def lpips_score(lr_img, hr_img):
        ctx = ImageDatasetAnalyzer._lpips_ctx
        if ctx is not None:
            lr, hr = _bgr(lr_img, "lpips_score"), _bgr(hr_img, "lpips_score")
            return float(ctx.lpips(ctx.to_device(lr[None]), ctx.to_device(hr[None]))[0])
        # not loaded (load_lpips): the message this method has always raised
        raise NotImplementedError("lpips_score: LPIPS needs AlexNet and LPIPS weights that are not available here; it is out of this port's scope "
                                  "(the rows' lpips column is NaN)")

    @staticmethod
    def rms_noise(gray):
        g = _gray(gray, "rms_noise")
        return _single(np.repeat(g[..., None], 3, 2))[0]["rms_noise_lr"]

    @staticmethod
    def laplacian_variance(gray):
        g = _gray(gray, "laplacian_variance")
        return _single(np.repeat(g[..., None], 3, 2))[0]["lap_var_lr"]

    @staticmethod
    def psnr_metric(lr_img, hr_img):
        ctx = _context()
        lr, hr = _bgr(lr_img, "psnr_metric"), _bgr(hr_img, "psnr_metric")
        return float(ctx.classic_scores(ctx.to_device(hr[None]), ctx.to_device(lr[None]), 255.0)[0, 0])

    @staticmethod
    def ssim_metric(lr_img, hr_img):
        ctx = _context()
        lr, hr = _bgr(lr_img, "ssim_metric"), _bgr(hr_img, "ssim_metric")
        return float(ctx.classic_scores(ctx.to_device(hr[None]), ctx.to_device(lr[None]), 255.0)[0, 1])

    @staticmethod
    def glcm_features(gray, angles=None, levels=64, multi_angle=False):
        g = _gray(gray, "glcm_features")
        if levels not in (64, 256):
            raise NotImplementedError(f"glcm_features: levels {levels} is not offered (64 or 256)")
        v = _single(np.repeat(g[..., None], 3, 2), levels, _angle_indices(angles, multi_angle))[0]
        return {k: v[k] for k in ("glcm_contrast", "glcm_homogeneity", "glcm_correlation")}

    @staticmethod
    def feature_distribution(img, hsv):
        a = _bgr(img, "feature_distribution")
        v, raw = _single(a, raw=True)
        hsv = np.asarray(hsv)
        if hsv.shape != a.shape or not (np.array_equal(hsv[..., 1], raw["sat"][0]) and np.array_equal(hsv[..., 2], raw["val"][0])):
            raise ValueError("feature_distribution: hsv is not COLOR_BGR2HSV of img (its S / V planes differ from the device's)")
        out = {}
        for c in range(3):
            for k in ("mean", "std", "skew", "kurt"):
                out[f"ch{c}_{k}"] = v[f"ch{c}_{k}_lr"]
        out["saturation_mean"] = v["saturation_mean_lr"]
        out["brightness_mean"] = v["brightness_mean_lr"]
        return out

    @staticmethod
    def detect_artifacts(img, gray):
        a = _bgr(img, "detect_artifacts")
        v, raw = _single(a, raw=True)
        if not np.array_equal(np.asarray(gray), raw["gray"][0]):
            raise ValueError("detect_artifacts: gray is not COLOR_BGR2GRAY of img (it differs from the device's plane)")
        return {"blocking_score": v["blocking_lr"], "color_noise": v["color_noise_lr"], "ringing_artifact": v["ringing_lr"]}

    @staticmethod
    def color_planes(img):
        """(gray, hsv) of a BGR image as the notebook's cv2.cvtColor calls give them, from the device; hsv's H plane is zero (never used)."""
        a = _bgr(img, "color_planes")
        _, raw = _single(a, raw=True)
        return raw["gray"][0], np.stack([np.zeros_like(raw["sat"][0]), raw["sat"][0], raw["val"][0]], -1)


class ImagePairMetrics:
    """The metrics of one LR / HR pair."""
    FIELDS = ("filename", "lpips", "psnr", "ssim", "glcm_contrast", "glcm_homogeneity", "glcm_correlation", "rms_noise_lr", "rms_noise_hr",
              "lap_var_lr", "lap_var_hr", "blocking_lr", "blocking_hr", "color_noise_lr", "color_noise_hr", "ringing_lr", "ringing_hr",
              "saturation_mean_lr", "saturation_mean_hr", "brightness_mean_lr", "brightness_mean_hr", "edge_diff",
              "ch0_skew_lr", "ch0_skew_hr", "ch1_skew_lr", "ch1_skew_hr", "ch2_skew_lr", "ch2_skew_hr",
              "ch0_kurt_lr", "ch0_kurt_hr", "ch1_kurt_lr", "ch1_kurt_hr", "ch2_kurt_lr", "ch2_kurt_hr")

    def __init__(self, filename, lpips, psnr, ssim, glcm_contrast, glcm_homogeneity, glcm_correlation, rms_noise_lr, rms_noise_hr, lap_var_lr,
                 lap_var_hr, blocking_lr, blocking_hr, color_noise_lr, color_noise_hr, ringing_lr, ringing_hr, saturation_mean_lr,
                 saturation_mean_hr, brightness_mean_lr, brightness_mean_hr, edge_diff, ch0_skew_lr=None, ch0_skew_hr=None, ch1_skew_lr=None,
                 ch1_skew_hr=None, ch2_skew_lr=None, ch2_skew_hr=None, ch0_kurt_lr=None, ch0_kurt_hr=None, ch1_kurt_lr=None, ch1_kurt_hr=None,
                 ch2_kurt_lr=None, ch2_kurt_hr=None):
        args = locals()
        for k in self.FIELDS:
            setattr(self, k, args[k])

    def as_dict(self):
        return self.__dict__.copy()


class MetricsAggregator:
    """Metric extraction for all pairs."""
    BATCH = 32

    @staticmethod
    def new_global_data():
        return {"count": 0, "lr_fft_sum": None, "hr_fft_sum": None, "grad_hr_sum": None, "glcm_sum": None,
                "sat_lr_counts": np.zeros(50, np.float64), "sat_hr_counts": np.zeros(50, np.float64), "sat_bins": SAT_BINS.copy(), "noise_means_lr": []}

    @staticmethod
    def collect_arrays(lr_imgs, hr_imgs, glcm_multi_angle=False, glcm_levels=64, filenames=None, device_acc=None, finish=True):
        """collect on aligned stacks [B, H, W, 3] uint8 BGR (NumPy arrays or device tensors) -> (rows, global_data).  device_acc / finish
        let a caller run several batches of one image size into the same device accumulators: pass the returned global_data['_device']
        back in and finish=True on the last batch, which downloads the sums once."""
        import torch
        ctx = _context()
        to_dev = lambda a: a.contiguous() if isinstance(a, torch.Tensor) else ctx.to_device(np.ascontiguousarray(np.asarray(a)))
        lr, hr = to_dev(lr_imgs), to_dev(hr_imgs)
        B = int(lr.shape[0])
        names = list(filenames) if filenames is not None else [str(i) for i in range(B)]
        if len(names) != B:
            raise ValueError(f"collect_arrays: {len(names)} file names for {B} pairs")
        cols = _row_columns()
        stats = ctx.eda_pair_stats(lr, hr, glcm_levels, (0, 1, 2, 3) if glcm_multi_angle else (0,))
        acc = ctx.eda_accumulate(lr, hr, device_acc)
        lp = ImageDatasetAnalyzer._lpips_ctx.lpips(lr, hr).cpu().numpy() if ImageDatasetAnalyzer._lpips_ctx is not None else None   # same batch pass
        host = stats.cpu().numpy()
        rows = [ImagePairMetrics(filename=names[i].replace("\\", "/"), lpips=math.nan if lp is None else float(lp[i]), **{k: float(host[i, j]) for j, k in enumerate(cols)}) for i in range(B)]
        g = MetricsAggregator.new_global_data()
        g["count"] = B
        g["noise_means_lr"] = [r.color_noise_lr for r in rows]
        g["_device"] = acc
        if finish:
            MetricsAggregator._download(g)
        return rows, g

    @staticmethod
    def _download(g):
        acc = g.pop("_device")
        for k in ("lr_fft_sum", "hr_fft_sum", "grad_hr_sum"):
            g[k] = acc[k].cpu().numpy()
        g["glcm_sum"] = acc["glcm_sum"].cpu().numpy().reshape(256, 256, 1, 1)
        sat = acc["sat_counts"].cpu().numpy()
        g["sat_lr_counts"], g["sat_hr_counts"] = sat[0].astype(np.float64), sat[1].astype(np.float64)

    @staticmethod
    def collect(lr_dir, hr_dir, glcm_multi_angle=False, glcm_levels=64, interp_map=None):
        """Metrics of every pair under the two trees and the global accumulators -> (rows in pair order, global_data).  Pairs are read on
        the host, LR is aligned to HR on the device, and pairs of one (LR shape, HR shape, interpolation) go through the device in batches.
        The global sums need one image size, as in the reference (its += fails otherwise)."""
        pairs = list(ImagePairLoader.iter_pairs(lr_dir, hr_dir))
        ctx = _context()
        groups = {}
        for idx, (lf, hf) in enumerate(pairs):
            lr, hr = ImagePairLoader.read_bgr(os.path.join(lr_dir, lf)), ImagePairLoader.read_bgr(os.path.join(hr_dir, hf))
            interp = ImagePairLoader.interpolation_for(lf, interp_map) if lr.shape != hr.shape else None
            groups.setdefault((lr.shape, hr.shape, interp), []).append((idx, lf, lr, hr))
        sizes = {k[1] for k in groups}
        if len(sizes) != 1:
            raise ValueError(f"collect: the global accumulators need HR images of one size, found {sorted(sizes)}")
        rows = [None] * len(pairs)
        acc = None
        for (_, hr_shape, interp), items in groups.items():
            for s in range(0, len(items), MetricsAggregator.BATCH):
                part = items[s:s + MetricsAggregator.BATCH]
                lr = ctx.to_device(np.stack([p[2] for p in part]))
                hr = ctx.to_device(np.stack([p[3] for p in part]))
                if interp is not None:
                    lr = ctx.resize(lr, hr_shape[0], hr_shape[1], interp)
                r, g = MetricsAggregator.collect_arrays(lr, hr, glcm_multi_angle, glcm_levels, [p[1] for p in part], device_acc=acc, finish=False)
                acc = g["_device"]
                for p, row in zip(part, r):
                    rows[p[0]] = row
        g = MetricsAggregator.new_global_data()
        g["count"] = len(rows)
        g["noise_means_lr"] = [r.color_noise_lr for r in rows]
        g["_device"] = acc
        MetricsAggregator._download(g)
        return rows, g


class StatsReporter:
    """The rows as columns, and their descriptive statistics (pandas is not a dependency: dicts of NumPy arrays instead of DataFrames)."""

    @staticmethod
    def dataframe(rows):
        """{column: NumPy array, one entry per pair}, in the reference DataFrame's column order."""
        dicts = [r.as_dict() for r in rows]
        keys = list(dicts[0]) if dicts else list(ImagePairMetrics.FIELDS)
        out = {}
        for k in keys:
            vals = [d[k] for d in dicts]
            numeric = all(v is None or isinstance(v, (int, float, np.integer, np.floating)) for v in vals)
            out[k] = np.array([math.nan if v is None else float(v) for v in vals], np.float64) if numeric else np.array(vals, dtype=object)
        return out

    @staticmethod
    def lpips_scenarios(df, top_k=1):
        """run_eda_pipeline's df.sort_values("lpips") head and tail -> (best, worst) lists of file names, top_k each (fewer when there
        are fewer rows).  The sort is stable (ties keep row order) and NaN sorts last, as pandas' does; ValueError when every value is
        NaN (nothing was scored: load_lpips)."""
        vals = np.asarray(df["lpips"], dtype=np.float64)
        if vals.size == 0 or np.isnan(vals).all():
            raise ValueError("lpips_scenarios: the lpips column holds no score (ImageDatasetAnalyzer.load_lpips was not called)")
        order = np.argsort(vals, kind="stable")
        k = min(max(int(top_k), 0), vals.size)
        names = [str(f) for f in np.asarray(df["filename"], dtype=object)]
        return [names[i] for i in order[:k]], [names[i] for i in order[vals.size - k:]]

    @staticmethod
    def summary(df):
        """{column: {mean, std, 25%, 50%, 75%}} of the numeric columns as DataFrame.describe() computes them: NaN skipped, std with
        ddof 1, quartiles by linear interpolation."""
        out = {}
        for k, col in df.items():
            a = np.asarray(col)
            if a.dtype.kind not in "fiu":
                continue
            a = np.sort(a.astype(np.float64)[~np.isnan(a.astype(np.float64))])
            n = a.size
            if n == 0:
                out[k] = {s: math.nan for s in ("mean", "std", "25%", "50%", "75%")}
                continue
            mean = float(a.sum() / n)

            def quantile(q):
                pos = q * (n - 1)
                lo = int(math.floor(pos))
                hi = min(lo + 1, n - 1)
                return float(a[lo] + (a[hi] - a[lo]) * (pos - lo))

            std = math.sqrt(float(((a - mean) ** 2).sum()) / (n - 1)) if n > 1 else math.nan
            out[k] = {"mean": mean, "std": std, "25%": quantile(0.25), "50%": quantile(0.5), "75%": quantile(0.75)}
        return out


def _finite(col):
    a = np.asarray(col, dtype=np.float64).ravel()
    return a[np.isfinite(a)]


def _hist30(col):
    """(counts, edges) of plt.hist(col, bins=30): np.histogram over the finite values' own range (matplotlib takes the range with
    nanmin / nanmax and np.histogram then drops the NaNs); None for a column without a finite value, where the plot fails."""
    a = _finite(col)
    return np.histogram(a, bins=30) if a.size else None


def _sat_density(counts):
    """(density, edges) of plt.hist(S.ravel(), bins=50, density=True) from the 256 counts of S: np.histogram over the image's own
    [min, max]; integer weights give the bits of the unweighted call on the pixels."""
    counts = np.asarray(counts, dtype=np.int64)
    nz = np.nonzero(counts)[0]
    return np.histogram(np.arange(256), 50, range=(int(nz[0]), int(nz[-1])), weights=counts, density=True)


def _contrast(P):
    """graycoprops(P, 'contrast')[0, 0] of a normed [L, L] matrix."""
    L = P.shape[0]
    I, J = np.ogrid[0:L, 0:L]
    return float(np.sum(P * (I - J) ** 2))


class ImageDataVisualization:
    """The numeric half of the reference's plots (cell 769cc582): every array and number a panel draws, no drawing.  The plotting names
    raise NotImplementedError naming the method that returns their numbers."""
    OVERLAY_PAIRS = (("blocking_lr", "blocking_hr", "Blocking Score"), ("ringing_lr", "ringing_hr", "Ringing Artifact"),
                     ("saturation_mean_lr", "saturation_mean_hr", "Saturation Mean"), ("brightness_mean_lr", "brightness_mean_hr", "Brightness Mean"),
                     ("color_noise_lr", "color_noise_hr", "Color Noise"))
    BOX_GROUPS = (("blocking_lr", "blocking_hr", "Blocking"), ("ringing_lr", "ringing_hr", "Ringing"), ("saturation_mean_lr", "saturation_mean_hr", "Saturation"),
                  ("brightness_mean_lr", "brightness_mean_hr", "Brightness"), ("color_noise_lr", "color_noise_hr", "ColorNoise"))
    DISTRIBUTION_COLUMNS = ("lpips", "psnr", "ssim", "lap_var_hr", "rms_noise_hr", "blocking_hr", "glcm_contrast", "glcm_homogeneity", "glcm_correlation")
    CORRELATION_COLUMNS = ("lpips", "psnr", "ssim", "lap_var_hr", "rms_noise_hr", "blocking_hr", "ringing_hr", "saturation_mean_hr", "brightness_mean_hr",
                           "edge_diff")
    SCATTER_PAIRS = (("lpips", "psnr", "LPIPS vs PSNR"), ("lpips", "ssim", "LPIPS vs SSIM"), ("lap_var_hr", "psnr", "LaplacianVar HR vs PSNR"),
                     ("rms_noise_hr", "psnr", "Noise HR vs PSNR"), ("blocking_hr", "ringing_hr", "Blocking vs Ringing"),
                     ("saturation_mean_hr", "brightness_mean_hr", "Saturation vs Brightness"), ("edge_diff", "psnr", "Edge Diff vs PSNR"),
                     ("edge_diff", "ssim", "Edge Diff vs SSIM"))
    _PLOTS = {"save_visual_example": "visual_example", "create_advanced_visualizations": "advanced_panel",
              "create_global_advanced_visualizations": "global_advanced_panel", "basic_distributions": "basic_distributions_data",
              "artifact_color_histograms": "artifact_color_histograms_data", "artifact_boxplots": "artifact_boxplots_data",
              "channel_shape_bars": "channel_shape_bars_data", "correlation_matrix": "correlation_matrix_data", "scatter_relations": "scatter_relations_data"}

    # ---------------------------------------------------------------- per pair, on the device
    @staticmethod
    def _aligned(lr_img, hr_img, who):
        lr, hr = _bgr(lr_img, who), _bgr(hr_img, who)
        if lr.shape != hr.shape:                      # save_visual_example's cv2.resize(lr, hr's size, INTER_CUBIC); the identity on an aligned pair
            ctx = _context()
            lr = ctx.resize(ctx.to_device(lr[None]), hr.shape[0], hr.shape[1], "INTER_CUBIC")[0].cpu().numpy()
        return lr, hr

    @staticmethod
    def visual_example(lr_img, hr_img):
        """save_visual_example's three images -> {'lr_rgb', 'hr_rgb', 'diff_gray'} uint8: the two RGB views and the gray difference map
        cvtColor(absdiff(lr, hr), BGR2GRAY) from the device.  The JET colour map on top of it is the plot's half: OpenCV's table is not
        restated here."""
        lr, hr = ImageDataVisualization._aligned(lr_img, hr_img, "visual_example")
        ctx = _context()
        d = ctx.eda_pair_panels(ctx.to_device(lr[None]), ctx.to_device(hr[None]), which=("diff",))["diff"][0].cpu().numpy()
        return {"lr_rgb": np.ascontiguousarray(lr[..., ::-1]), "hr_rgb": np.ascontiguousarray(hr[..., ::-1]), "diff_gray": d}

    @staticmethod
    def _panel_of(host, i):
        return {"lr_log_spectrum": np.log(host["spec_lr"][i] + 1e-8), "hr_log_spectrum": np.log(host["spec_hr"][i] + 1e-8),
                "gradient_magnitude": host["grad_hr"][i], "lr_glcm": host["glcm_lr"][i], "lr_glcm_contrast": float(host["glcm_contrast"][i]),
                "noise_map": host["noise_lr"][i], "color_noise_mean": float(host["noise_mean"][i]),
                "sat_lr": _sat_density(host["sat_hist"][i, 0]), "sat_hr": _sat_density(host["sat_hist"][i, 1]), "diff_gray": host["diff"][i]}

    @staticmethod
    def advanced_panels(lr_imgs, hr_imgs):
        """advanced_panel for aligned stacks [B, H, W, 3] uint8 BGR (NumPy arrays or device tensors) -> list of B dicts (each also carries
        visual_example's 'diff_gray').  One device call and one read per chunk of MetricsAggregator.BATCH pairs."""
        import torch
        ctx = _context()
        to_dev = lambda a: a.contiguous() if isinstance(a, torch.Tensor) else ctx.to_device(np.ascontiguousarray(np.asarray(a)))
        out = []
        for s in range(0, int(lr_imgs.shape[0]), MetricsAggregator.BATCH):
            dev = ctx.eda_pair_panels(to_dev(lr_imgs[s:s + MetricsAggregator.BATCH]), to_dev(hr_imgs[s:s + MetricsAggregator.BATCH]))
            host = {k: v.cpu().numpy() for k, v in dev.items()}
            out.extend(ImageDataVisualization._panel_of(host, i) for i in range(host["diff"].shape[0]))
        return out

    @staticmethod
    def advanced_panel(lr_img, hr_img):
        """create_advanced_visualizations' numbers for one aligned BGR pair: 'lr_log_spectrum', 'hr_log_spectrum' (np.log(mag + 1e-8) of the
        device's magnitudes, taken here), 'gradient_magnitude', 'lr_glcm' [256, 256], 'lr_glcm_contrast', 'noise_map', 'color_noise_mean',
        'sat_lr', 'sat_hr' ((density, edges) of plt.hist(S.ravel(), bins=50, density=True))."""
        lr, hr = _bgr(lr_img, "advanced_panel"), _bgr(hr_img, "advanced_panel")
        if lr.shape != hr.shape:
            raise ValueError(f"advanced_panel: the pair is not aligned ({lr.shape} and {hr.shape}); ImagePairLoader.load_and_align does that")
        p = ImageDataVisualization.advanced_panels(lr[None], hr[None])[0]
        p.pop("diff_gray")
        return p

    # ---------------------------------------------------------------- host NumPy on collect's global_data and on the frame
    @staticmethod
    def global_advanced_panel(global_data):
        """create_global_advanced_visualizations' numbers from collect's global_data; None when it holds no pair (the reference prints and returns)."""
        if global_data is None or global_data.get("count", 0) == 0:
            return None
        n, eps = global_data["count"], 1e-8
        out = {k + "_avg": np.asarray(global_data[k + "_sum"]) / n for k in ("lr_fft", "hr_fft", "grad_hr")}
        out["lr_log_spectrum"], out["hr_log_spectrum"] = np.log(out["lr_fft_avg"] + eps), np.log(out["hr_fft_avg"] + eps)
        glcm_sum = np.asarray(global_data["glcm_sum"])
        glcm_avg = (glcm_sum / glcm_sum.sum()).reshape(glcm_sum.shape[0], glcm_sum.shape[1])
        out["glcm_avg"], out["glcm_contrast"] = glcm_avg, _contrast(glcm_avg)
        bins = np.asarray(global_data["sat_bins"])
        width = bins[1] - bins[0]
        for s in ("lr", "hr"):
            c = np.asarray(global_data[f"sat_{s}_counts"])
            out[f"sat_{s}_density"] = c / (c.sum() * width + eps)
        out["sat_centers"] = 0.5 * (bins[:-1] + bins[1:])
        noise = np.array(global_data["noise_means_lr"], dtype=np.float64)
        out["noise_means"], out["noise_mean"], out["noise_std"] = noise, float(noise.mean()), float(noise.std())
        out["noise_hist"] = np.histogram(noise, bins=30)
        return out

    @staticmethod
    def basic_distributions_data(df):
        """{column: (counts, edges)}: plt.hist(df[column], bins=30) of the nine columns of distributions.png."""
        return {m: _hist30(df[m]) for m in ImageDataVisualization.DISTRIBUTION_COLUMNS}

    @staticmethod
    def kde(values, gridsize=200, cut=3):
        """The curve seaborn.kdeplot draws by default, restated from seaborn's documented defaults (seaborn is not installed where this
        project runs, so it is not pinned against seaborn itself): a Gaussian kernel with Scott's factor n^(-1/5) on the sample standard
        deviation (ddof 1), evaluated at `gridsize` points from min - cut bw to max + cut bw -> (grid, density, bw)."""
        x = _finite(values)
        n = x.size
        if n < 2:
            return None
        bw = float(np.std(x, ddof=1)) * n ** (-0.2)
        if not bw > 0.0:
            return None
        grid = np.linspace(x.min() - cut * bw, x.max() + cut * bw, gridsize)
        z = (grid[:, None] - x[None, :]) / bw
        return grid, np.exp(-0.5 * z * z).sum(1) / (n * bw * math.sqrt(2.0 * math.pi)), bw

    @staticmethod
    def artifact_color_histograms_data(df):
        """artifact_color_histograms.png: per overlay title {'lr', 'hr'} each its own 30-bin histogram (two plt.hist calls), then
        'edge_diff' (histogram) and 'edge_diff_kde' (kde above)."""
        out = {title: {"lr": _hist30(df[l]), "hr": _hist30(df[h])} for l, h, title in ImageDataVisualization.OVERLAY_PAIRS}
        out["edge_diff"] = _hist30(df["edge_diff"])
        k = ImageDataVisualization.kde(df["edge_diff"])
        out["edge_diff_kde"] = None if k is None else {"grid": k[0], "density": k[1], "bw": k[2]}
        return out

    @staticmethod
    def boxplot_stats(values, whis=1.5):
        """matplotlib.cbook.boxplot_stats(x, whis) of the finite values: q1 / med / q3 by linear percentiles, the whiskers at the furthest
        data within whis IQR of the box (the quartile itself when there is none), fliers beyond them (low ones first), mean, iqr."""
        x = _finite(values)
        if not x.size:
            return None
        q1, med, q3 = (float(v) for v in np.percentile(x, [25, 50, 75]))
        iqr = q3 - q1
        hi, lo = x[x <= q3 + whis * iqr], x[x >= q1 - whis * iqr]
        whishi = q3 if hi.size == 0 or hi.max() < q3 else float(hi.max())
        whislo = q1 if lo.size == 0 or lo.min() > q1 else float(lo.min())
        return {"mean": float(np.mean(x)), "med": med, "q1": q1, "q3": q3, "iqr": iqr, "whislo": whislo, "whishi": whishi,
                "fliers": np.concatenate([x[x < whislo], x[x > whishi]])}

    @staticmethod
    def artifact_boxplots_data(df):
        """{label: boxplot_stats} under the reference's ten labels ('Blocking LR', 'Blocking HR', ...), in its order."""
        out = {}
        for l, h, name in ImageDataVisualization.BOX_GROUPS:
            out[f"{name} LR"] = ImageDataVisualization.boxplot_stats(df[l])
            out[f"{name} HR"] = ImageDataVisualization.boxplot_stats(df[h])
        return out

    @staticmethod
    def channel_shape_bars_data(df):
        """The four bar groups' heights, each [B, G, R]: the columns' means, NaN skipped as Series.mean does; None when a column is missing."""
        need = [f"ch{c}_{k}_{s}" for k in ("skew", "kurt") for c in range(3) for s in ("lr", "hr")]
        if not all(r in df for r in need):
            return None
        mean = lambda k: float(_finite(df[k]).mean()) if _finite(df[k]).size else math.nan
        return {f"{k}_means_{s}": [mean(f"ch{c}_{k}_{s}") for c in range(3)] for k in ("skew", "kurt") for s in ("lr", "hr")}

    @staticmethod
    def correlation_matrix_data(df):
        """{'columns', 'corr'}: Pearson's r between the available ones of the ten columns, each pair over the rows where both are finite,
        as DataFrame.corr does (NaN where fewer than two such rows or a constant column); None below three columns."""
        cols = [m for m in ImageDataVisualization.CORRELATION_COLUMNS if m in df]
        if len(cols) < 3:
            return None
        data = [np.asarray(df[m], dtype=np.float64) for m in cols]
        corr = np.full((len(cols), len(cols)), math.nan)
        for i, a in enumerate(data):
            for j, b in enumerate(data[:i + 1]):
                m = np.isfinite(a) & np.isfinite(b)
                if m.sum() < 2:
                    continue
                x, y = a[m] - a[m].mean(), b[m] - b[m].mean()
                den = math.sqrt(float((x * x).sum()) * float((y * y).sum()))
                if den > 0.0:
                    corr[i, j] = corr[j, i] = 1.0 if i == j else float((x * y).sum()) / den
        return {"columns": cols, "corr": corr}

    @staticmethod
    def scatter_relations_data(df):
        """The scatter panels present in the frame: list of {'x', 'y', 'title', 'x_values', 'y_values'}."""
        return [{"x": x, "y": y, "title": t, "x_values": np.asarray(df[x], dtype=np.float64), "y_values": np.asarray(df[y], dtype=np.float64)}
                for x, y, t in ImageDataVisualization.SCATTER_PAIRS if x in df and y in df]

    @staticmethod
    def flatten_panel(panel, prefix=""):
        """A panel as the flat {name: array} that its .npz holds: nested names joined with '.', tuples and lists of arrays by index,
        None left out."""
        out = {}
        if panel is None:
            return out
        if isinstance(panel, dict):
            items = panel.items()
        elif isinstance(panel, (tuple, list)) and any(isinstance(v, (dict, tuple, list, np.ndarray)) or v is None for v in panel):
            items = enumerate(panel)
        else:
            out[prefix or "value"] = np.asarray(panel)
            return out
        for k, v in items:
            out.update(ImageDataVisualization.flatten_panel(v, f"{prefix}.{k}" if prefix else str(k)))
        return out


def _plot_stub(name, numeric):
    def stub(*args, **kwargs):
        raise NotImplementedError(f"{name}: drawing is not offered (no matplotlib / seaborn here); ImageDataVisualization.{numeric} returns the numbers "
                                  f"this plot shows")
    stub.__name__ = name
    return staticmethod(stub)


for _name, _numeric in ImageDataVisualization._PLOTS.items():
    setattr(ImageDataVisualization, _name, _plot_stub(_name, _numeric))


def _load_interp_map(interp_map_path):
    """run_eda_pipeline's loading of the pickled {file name: interpolation name} map, with its two messages."""
    if interp_map_path and os.path.exists(interp_map_path):
        try:
            import pickle
            with open(interp_map_path, "rb") as f:
                return pickle.load(f)
        except Exception as e:
            print(f"Warning: could not load interpolation map: {e}")
            return None
    print("Interpolation map not found; default interpolation will be used.")
    return None


def run_eda_panels(lr_dir, hr_dir, top_k_examples=1, glcm_multi_angle=False, glcm_levels=64, interp_map_path="", rank_by="lpips"):
    """run_eda_pipeline without the files -> (df, panels).  panels: 'advanced_global_panel', 'distributions',
    'artifact_color_histograms', 'artifact_boxplots', 'channel_shape_bars', 'correlation_matrix', 'scatter_relations' (the numeric
    methods above on collect's rows) and 'examples': {'{label}_scenarios/{parent}/{label}_{rank}_{stem}': visual_example,
    '.../{label}_{rank}_advanced_{stem}': advanced_panel} for the best and worst top_k_examples rows by `rank_by` (ascending, stable,
    NaN last; the reference ranks by lpips).  Example pairs of one size go through the device as one batch."""
    if rank_by == "lpips" and ImageDatasetAnalyzer._lpips_ctx is None:
        raise NotImplementedError("run_eda_panels: ranking by lpips needs the LPIPS weights: call ImageDatasetAnalyzer.load_lpips(alexnet_path, "
                                  "lpips_path) first, or rank by another column (rank_by='psnr')")
    interp_map = _load_interp_map(interp_map_path)
    rows, global_data = MetricsAggregator.collect(lr_dir, hr_dir, glcm_multi_angle=glcm_multi_angle, glcm_levels=glcm_levels, interp_map=interp_map)
    df = StatsReporter.dataframe(rows)
    V = ImageDataVisualization
    panels = {"advanced_global_panel": V.global_advanced_panel(global_data), "distributions": V.basic_distributions_data(df),
              "artifact_color_histograms": V.artifact_color_histograms_data(df), "artifact_boxplots": V.artifact_boxplots_data(df),
              "channel_shape_bars": V.channel_shape_bars_data(df), "correlation_matrix": V.correlation_matrix_data(df),
              "scatter_relations": V.scatter_relations_data(df), "examples": {}}
    if rank_by not in df or np.asarray(df[rank_by]).dtype.kind != "f":
        raise ValueError(f"run_eda_panels: rank_by {rank_by!r} is not a numeric column of the frame")
    vals = np.asarray(df[rank_by], dtype=np.float64)
    order = np.argsort(vals, kind="stable")
    k = min(max(int(top_k_examples), 0), vals.size)
    names = [str(f) for f in df["filename"]]
    picked = []                                      # (visual key, advanced key, lr, hr)
    for label, idx in (("best", order[:k]), ("worst", order[vals.size - k:])):
        for rank, i in enumerate(idx, 1):
            rel = names[i]
            lr, hr = ImagePairLoader.load_and_align(os.path.join(lr_dir, rel), os.path.join(hr_dir, rel), interp_map=interp_map)
            rel_no_ext = os.path.splitext(rel.replace("\\", "/"))[0]
            parent, stem = os.path.dirname(rel_no_ext), os.path.basename(rel_no_ext)
            base = f"{label}_scenarios/{parent}/" if parent else f"{label}_scenarios/"
            picked.append((f"{base}{label}_{rank}_{stem}", f"{base}{label}_{rank}_advanced_{stem}", lr, hr))
    by_shape = {}
    for n, p in enumerate(picked):
        by_shape.setdefault(p[3].shape, []).append(n)
    adv = [None] * len(picked)
    for members in by_shape.values():
        res = V.advanced_panels(np.stack([picked[n][2] for n in members]), np.stack([picked[n][3] for n in members]))
        for n, r in zip(members, res):
            adv[n] = r
    for (vis_key, adv_key, lr, hr), a in zip(picked, adv):
        panels["examples"][vis_key] = {"lr_rgb": np.ascontiguousarray(lr[..., ::-1]), "hr_rgb": np.ascontiguousarray(hr[..., ::-1]), "diff_gray": a.pop("diff_gray")}
        panels["examples"][adv_key] = a
    return df, panels


PANEL_NAMES = ("advanced_global_panel", "distributions", "artifact_color_histograms", "artifact_boxplots", "channel_shape_bars", "correlation_matrix",
               "scatter_relations")


def run_eda_pipeline(lr_dir, hr_dir, output_dir="eda_results", top_k_examples=1, glcm_multi_angle=False, glcm_levels=64, interp_map_path="", rank_by="lpips"):
    """The notebook's last cell: the reference's signature (rank_by is this port's addition, for a run without the LPIPS weights) and its
    return value, df.  Where the reference saves a .png, the panel's numbers are written as an .npz of the same stem (flatten_panel's
    names): advanced_global_panel.npz, distributions.npz, artifact_color_histograms.npz, artifact_boxplots.npz, channel_shape_bars.npz,
    correlation_matrix.npz, scatter_relations.npz, LPIPS_Scenarios/{best,worst}_scenarios/<parent>/{label}_{rank}[_advanced]_{stem}.npz.
    A panel the reference skips (None) writes no file."""
    df, panels = run_eda_panels(lr_dir, hr_dir, top_k_examples, glcm_multi_angle, glcm_levels, interp_map_path, rank_by)
    examples_dir = os.path.join(output_dir, "LPIPS_Scenarios")
    for d in (output_dir, os.path.join(examples_dir, "best_scenarios"), os.path.join(examples_dir, "worst_scenarios")):
        os.makedirs(d, exist_ok=True)
    files = [(os.path.join(output_dir, key), panels[key]) for key in PANEL_NAMES]
    files += [(os.path.join(examples_dir, *key.split("/")), p) for key, p in panels["examples"].items()]
    for path, panel in files:
        flat = ImageDataVisualization.flatten_panel(panel)
        if not flat:
            continue
        os.makedirs(os.path.dirname(path), exist_ok=True)
        np.savez(path + ".npz", **flat)
    return df
