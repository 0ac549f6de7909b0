"""NumPy restatement of the dataset EDA's per-pair statistics and global accumulators (reference data/EDA.ipynb: ImageDatasetAnalyzer,
cell 87582ba8, and MetricsAggregator.collect, cell eb5cc926), the contract csrc/eda.hip implements.  Integer where the contract is
integer, fp64 elsewhere; written from the definitions below, not from the reference's text.

Inputs are aligned pairs (lr, hr) of uint8 BGR images [H, W, 3].  cv2 is not installed where these tests run, so the 8-bit OpenCV paths
are restated from OpenCV's documented behaviour and are NOT pinned against cv2 itself:
  gray     COLOR_BGR2GRAY: (1868 B + 9617 G + 4899 R + 8192) >> 14 (imgproc color_yuv: the 14-bit RGB2Gray coefficients).
  blur3/5  GaussianBlur (3,3) / (5,5), sigma 0: getGaussianKernel's fixed small-kernel taps (1 2 1) / 4 and (1 4 6 4 1) / 16, separable;
           for 8-bit images the fixed-point filter is exact, so the result is the exact integer sum rounded half up once,
           (s + 8) >> 4 and (s + 128) >> 8; BORDER_REFLECT_101.
  HSV      COLOR_BGR2HSV, 8 bit (imgproc color_hsv, RGB2HSV_b): V = max, S = ((V - min) sdiv[V] + 2^11) >> 12 with
           sdiv[v] = round(255 2^12 / v), sdiv[0] = 0.  H is never used and not computed.
  Canny    Canny(gray, 100, 200), aperture 3, L2gradient off (imgproc canny.cpp): 3 x 3 Sobel pair with replicated borders, magnitude
           m = |gx| + |gy|.  A pixel with m > 100 survives non-maximum suppression when, with x = |gx| and y = |gy| << 15:
             y < 13573 x              (horizontal gradient)  m > left and m >= right;
             y > 13573 x + (x << 16)  (vertical gradient)    m > above and m >= below;
             otherwise (diagonal), s = -1 where gx and gy differ in sign, else 1:  m > (above, col - s) and m > (below, col + s).
           A survivor is strong when m > 200.  An edge is a survivor that is strong or 8-connected through survivors to a strong one.
           The outermost rows and columns are never edges.  canny.cpp pads its magnitude and label buffers by one pixel, which can be
           read as letting the border pixels take part with zero magnitude outside; the project's contract fixes the other reading:
           border pixels are neither strong nor weak and carry no connection, their magnitudes still count in their neighbours'
           suppression.
  dilate   5 x 5 ones, centred anchor; pixels outside the image are ignored (morphology's default border never adds a set pixel).
  Laplacian  cv2.Laplacian(gray, CV_64F), aperture 1: 0 1 0 / 1 -4 1 / 0 1 0, BORDER_REFLECT_101.   Sobel ksize 5: (1 4 6 4 1) x (-1 -2 0 2 1).
  dct      the orthonormal 2-D DCT-II of the whole image, in fp64 (cv2.dct computes it in float32).
skimage / scipy pieces: graycomatrix's offset for angle a is (round(sin a), round(cos a)) in (row, col); graycoprops' correlation is 1
where either marginal standard deviation is below 1e-15; filters.sobel scales the image by 1 / 255, uses (1 2 1) x (1 0 -1) / 4 with
scipy 'reflect' borders (edge pixel repeated) and returns sqrt((h^2 + v^2) / 2); stats.skew is m3 / m2^1.5 (biased), kurtosis
m4 / m2^2 - 3 (Fisher), both NaN for a constant channel.  Central moments are formed exactly from Python integers
(N sum x^2 - (sum x)^2 and its third- and fourth-order kin, one division).

The CPU tests (test_eda_cpu.py) check each piece against an independent form: scipy.stats, scipy.fft, scipy.ndimage, np.histogram,
plain loops and a hand-made example."""
import math

import numpy as np

ROW_COLUMNS = (("psnr", "ssim", "glcm_contrast", "glcm_homogeneity", "glcm_correlation")
               + tuple(f"{k}_{s}" for k in ("rms_noise", "lap_var", "blocking", "color_noise", "ringing", "saturation_mean", "brightness_mean")
                       for s in ("lr", "hr"))
               + ("edge_diff",)
               + tuple(f"ch{c}_{k}_{s}" for k in ("skew", "kurt") for c in range(3) for s in ("lr", "hr")))
STAT_NAMES = (ROW_COLUMNS + ("sobel_mean_lr", "sobel_mean_hr")
              + tuple(f"ch{c}_{k}_{s}" for k in ("mean", "std") for c in range(3) for s in ("lr", "hr")))
ANGLE_OFFSETS = ((0, 1), (1, 1), (1, 0), (1, -1))        # 0, 45, 90, 135 degrees: (round(sin a), round(cos a))
SAT_BINS = np.linspace(0, 256, 51)


# ------------------------------------------------------------------ 8-bit planes
def gray_u8(img):
    x = np.asarray(img).astype(np.int64)
    return ((1868 * x[..., 0] + 9617 * x[..., 1] + 4899 * x[..., 2] + 8192) >> 14).astype(np.uint8)


def _pad(x, r, mode):
    return np.pad(x, [(r, r), (r, r)] + [(0, 0)] * (x.ndim - 2), mode=mode)


def _correlate_int(x, k, mode):
    """Integer correlation of [H, W(, C)] with the odd square kernel k; mode 'reflect' is BORDER_REFLECT_101, 'edge' replicates."""
    k = np.asarray(k, np.int64)
    r = k.shape[0] // 2
    p = _pad(np.asarray(x).astype(np.int64), r, mode)
    H, W = x.shape[:2]
    out = np.zeros(x.shape, np.int64)
    for i in range(k.shape[0]):
        for j in range(k.shape[1]):
            if k[i, j]:
                out += k[i, j] * p[i:i + H, j:j + W]
    return out


B3 = np.outer([1, 2, 1], [1, 2, 1])
B5 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
LAP = np.array([[0, 1, 0], [1, -4, 1], [0, 1, 0]])
SOBEL3_X = np.outer([1, 2, 1], [-1, 0, 1])               # d / dx: smooth down the rows, differentiate along the columns
SOBEL5_X = np.outer([1, 4, 6, 4, 1], [-1, -2, 0, 2, 1])


def blur3_u8(x):
    return ((_correlate_int(x, B3, "reflect") + 8) >> 4).astype(np.uint8)


def blur5_u8(x):
    return ((_correlate_int(x, B5, "reflect") + 128) >> 8).astype(np.uint8)


def laplacian(gray):
    return _correlate_int(gray, LAP, "reflect")


def sobel5(gray):
    return _correlate_int(gray, SOBEL5_X, "reflect"), _correlate_int(gray, SOBEL5_X.T, "reflect")


def hsv_sv(img):
    """(S, V) uint8 planes of 8-bit COLOR_BGR2HSV."""
    x = np.asarray(img).astype(np.int64)
    v = x.max(-1)
    d = v - x.min(-1)
    sdiv = np.zeros(256, np.int64)
    sdiv[1:] = [int(round(255 * 4096 / i)) for i in range(1, 256)]       # never a tie: 2 * 255 * 4096 has no odd multiple of i <= 255 times 2^13
    return ((d * sdiv[v] + 2048) >> 12).astype(np.uint8), v.astype(np.uint8)


def sat_counts(s):
    """np.histogram(S, linspace(0, 256, 51)) through integers: the edges are i * 5.12, so the bin of an integer S is S * 25 // 128."""
    return np.bincount(np.asarray(s).astype(np.int64).ravel() * 25 // 128, minlength=50).astype(np.int64)


# ------------------------------------------------------------------ Canny
def canny_labels(gray):
    """0 none / 1 weak survivor / 2 strong, after non-maximum suppression (before hysteresis); the outermost rows and columns are 0."""
    gx = _correlate_int(gray, SOBEL3_X, "edge")
    gy = _correlate_int(gray, SOBEL3_X.T, "edge")
    m = np.abs(gx) + np.abs(gy)
    H, W = m.shape
    mp = np.pad(m, 1)                                    # never read for an interior pixel's decision; keeps the slices simple
    nb = lambda dy, dx: mp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    x, y = np.abs(gx), np.abs(gy) << 15
    t22 = x * 13573
    t67 = t22 + (x << 16)
    horiz = y < t22
    vert = ~horiz & (y > t67)
    diag = ~horiz & ~vert
    s_neg = (gx ^ gy) < 0                                # s = -1
    keep = np.zeros((H, W), bool)
    keep |= horiz & (m > nb(0, -1)) & (m >= nb(0, 1))
    keep |= vert & (m > nb(-1, 0)) & (m >= nb(1, 0))
    keep |= diag & s_neg & (m > nb(-1, 1)) & (m > nb(1, -1))
    keep |= diag & ~s_neg & (m > nb(-1, -1)) & (m > nb(1, 1))
    keep &= m > 100
    keep[0, :] = keep[-1, :] = False
    keep[:, 0] = keep[:, -1] = False
    lab = np.zeros((H, W), np.uint8)
    lab[keep] = 1
    lab[keep & (m > 200)] = 2
    return lab


def _grow8(e):
    p = np.pad(e, 1)
    H, W = e.shape
    out = np.zeros_like(e)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def hysteresis(lab):
    """Edges (bool): strong pixels, and weak survivors 8-connected to one through survivors: grow until nothing changes."""
    edge = lab == 2
    weak = lab == 1
    while True:
        new = weak & _grow8(edge) & ~edge
        if not new.any():
            return edge
        edge = edge | new


def canny_u8(gray):
    return hysteresis(canny_labels(gray)).astype(np.uint8) * 255


def dilate5(e):
    e = np.asarray(e) != 0
    p = np.pad(e, 2)
    H, W = e.shape
    out = np.zeros_like(e)
    for dy in range(5):
        for dx in range(5):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def ringing(gray, edges):
    e = np.asarray(edges) != 0
    region = dilate5(e) & ~e
    g = np.asarray(gray)[region].astype(np.int64)
    n = int(g.size)
    if n == 0:
        return 0.0
    s1, s2 = int(g.sum()), int((g * g).sum())
    return math.sqrt(n * s2 - s1 * s1) / n


# ------------------------------------------------------------------ co-occurrence
def quantise(gray, levels):
    return ((np.asarray(gray).astype(np.float32) / 255.0) * (levels - 1)).astype(np.uint8)


def glcm_counts(q, levels, angles=(0, 1, 2, 3)):
    """Integer counts [nangles, L, L] before symmetrisation: pixel (r, c) pairs with (r + dr, c + dc), distance 1."""
    q = np.asarray(q).astype(np.int64)
    H, W = q.shape
    out = np.zeros((len(angles), levels, levels), np.int64)
    for n, a in enumerate(angles):
        dr, dc = ANGLE_OFFSETS[a]
        r0, r1 = max(0, -dr), min(H, H - dr)
        c0, c1 = max(0, -dc), min(W, W - dc)
        i = q[r0:r1, c0:c1]
        j = q[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
        out[n] = np.bincount((i * levels + j).ravel(), minlength=levels * levels).reshape(levels, levels)
    return out


def glcm_normed(counts):
    """graycomatrix(symmetric=True, normed=True) of one angle's counts -> fp64 [L, L]."""
    s = (counts + counts.T).astype(np.float64)
    return s / s.sum()


def glcm_props(P):
    """graycoprops' (contrast, homogeneity, correlation) of one normed matrix."""
    L = P.shape[0]
    I, J = np.ogrid[0:L, 0:L]
    contrast = float(np.sum(P * (I - J) ** 2))
    homogeneity = float(np.sum(P / (1.0 + (I - J) ** 2)))
    di, dj = I - np.sum(I * P), J - np.sum(J * P)
    si, sj = math.sqrt(np.sum(P * di ** 2)), math.sqrt(np.sum(P * dj ** 2))
    corr = 1.0 if si < 1e-15 or sj < 1e-15 else float(np.sum(P * (di * dj)) / (si * sj))
    return contrast, homogeneity, corr


def glcm_features(gray, levels, angles=(0,)):
    c = glcm_counts(quantise(gray, levels), levels, angles)
    p = np.array([glcm_props(glcm_normed(c[n])) for n in range(len(angles))])
    return tuple(float(np.mean(p[:, k])) for k in range(3))


# ------------------------------------------------------------------ fp64 pieces
def dct_operator(N):
    k, x = np.ogrid[0:N, 0:N]
    op = np.cos(np.pi * ((2 * x + 1) * k % (4 * N)) / (2.0 * N)) * math.sqrt(2.0 / N)
    op[0] *= math.sqrt(0.5)
    return op


def dct2(gray):
    g = np.asarray(gray).astype(np.float64)
    return dct_operator(g.shape[0]) @ g @ dct_operator(g.shape[1]).T


def blocking(gray):
    D = np.abs(dct2(gray))
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return float((np.mean(D[7::8, :]) + np.mean(D[:, 7::8])) / 2)


def sobel_mean(gray):
    """mean(skimage.filters.sobel(gray)) for a uint8 image."""
    g = _pad(np.asarray(gray).astype(np.float64) / 255.0, 1, "edge")
    H, W = gray.shape
    s = lambda dy, dx: g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    h = ((s(-1, -1) + 2 * s(-1, 0) + s(-1, 1)) - (s(1, -1) + 2 * s(1, 0) + s(1, 1))) / 4.0
    v = ((s(-1, -1) + 2 * s(0, -1) + s(1, -1)) - (s(-1, 1) + 2 * s(0, 1) + s(1, 1))) / 4.0
    return float(np.mean(np.sqrt((h * h + v * v) / 2.0)))


def fft_mag(gray):
    return np.abs(np.fft.fftshift(np.fft.fft2(np.asarray(gray).astype(np.float64))))


def grad5_mag(gray):
    gx, gy = sobel5(gray)
    return np.sqrt((gx * gx + gy * gy).astype(np.float64))


def moments(channel):
    """(mean, population std, skew, kurtosis) of a uint8 channel, the central moments exact in Python integers."""
    h = [int(c) for c in np.bincount(np.asarray(channel, np.uint8).ravel(), minlength=256)]       # power sums through the value counts
    n = sum(h)
    s1, s2, s3, s4 = (sum(c * v ** k for v, c in enumerate(h)) for k in (1, 2, 3, 4))
    n2 = n * s2 - s1 * s1
    n3 = n * n * s3 - 3 * n * s1 * s2 + 2 * s1 ** 3
    n4 = n ** 3 * s4 - 4 * n * n * s1 * s3 + 6 * n * s1 * s1 * s2 - 3 * s1 ** 4
    m2, m3, m4 = n2 / n ** 2, n3 / n ** 3, n4 / n ** 4
    if n2 == 0:
        return s1 / n, 0.0, math.nan, math.nan
    return s1 / n, math.sqrt(m2), m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0


def _var_int(x):
    x = np.asarray(x).astype(np.int64).ravel()
    n, s1, s2 = int(x.size), int(x.sum()), int((x * x).sum())
    return (n * s2 - s1 * s1) / (n * n)


# ------------------------------------------------------------------ the row
def image_stats(img):
    """Every per-image quantity of one BGR image -> dict (names without the _lr / _hr suffix) plus the raw planes."""
    img = np.asarray(img)
    g = gray_u8(img)
    N = g.size
    s, v = hsv_sv(img)
    b3, b5 = blur3_u8(g), blur5_u8(img)
    d = g.astype(np.int64) - b3.astype(np.int64)
    edges = canny_u8(g)
    out = {"rms_noise": math.sqrt(int((d * d).sum()) / N), "lap_var": _var_int(laplacian(g)), "blocking": blocking(g),
           "color_noise": int(np.abs(img.astype(np.int64) - b5.astype(np.int64)).sum()) / (3 * N), "ringing": ringing(g, edges),
           "saturation_mean": int(s.astype(np.int64).sum()) / N, "brightness_mean": int(v.astype(np.int64).sum()) / N, "sobel_mean": sobel_mean(g)}
    for c in range(3):
        out[f"ch{c}_mean"], out[f"ch{c}_std"], out[f"ch{c}_skew"], out[f"ch{c}_kurt"] = moments(img[..., c])
    raw = {"gray": g, "sat": s, "val": v, "blur3": b3, "blur5": b5, "edges": edges}
    return out, raw


def pair_stats(lr, hr, levels=64, angles=(0,), psnr_ssim=(math.nan, math.nan)):
    """The row of one pair in STAT_NAMES order (psnr / ssim as passed: they are sr_classic_scores' columns) -> (fp64 [46], raw dict)."""
    sl, rl = image_stats(lr)
    sh, rh = image_stats(hr)
    vals = {"psnr": psnr_ssim[0], "ssim": psnr_ssim[1]}
    vals["glcm_contrast"], vals["glcm_homogeneity"], vals["glcm_correlation"] = glcm_features(rl["gray"], levels, angles)
    for k, x in sl.items():
        vals[k + "_lr"] = x
    for k, x in sh.items():
        vals[k + "_hr"] = x
    for c in range(3):
        for k in ("skew", "kurt", "mean", "std"):
            vals[f"ch{c}_{k}_lr"] = sl[f"ch{c}_{k}"]
            vals[f"ch{c}_{k}_hr"] = sh[f"ch{c}_{k}"]
    vals["edge_diff"] = sh["sobel_mean"] - sl["sobel_mean"]
    raw = {k: np.stack([rl[k], rh[k]]) for k in rl}
    raw["glcm"] = glcm_counts(quantise(rl["gray"], levels), levels, angles)
    raw["dct"] = np.stack([dct2(rl["gray"]), dct2(rh["gray"])])
    return np.array([vals[k] for k in STAT_NAMES], np.float64), raw


def accumulate(lrs, hrs):
    """collect's global accumulators over the pairs, in order."""
    H, W = lrs[0].shape[:2]
    out = {"lr_fft_sum": np.zeros((H, W)), "hr_fft_sum": np.zeros((H, W)), "grad_hr_sum": np.zeros((H, W)), "glcm_sum": np.zeros((256, 256)),
           "sat_counts": np.zeros((2, 50), np.int64)}
    for lr, hr in zip(lrs, hrs):
        gl, gh = gray_u8(lr), gray_u8(hr)
        out["lr_fft_sum"] += fft_mag(gl)
        out["hr_fft_sum"] += fft_mag(gh)
        out["grad_hr_sum"] += grad5_mag(gh)
        out["glcm_sum"] += glcm_normed(glcm_counts(gl, 256, (0,))[0])
        out["sat_counts"][0] += sat_counts(hsv_sv(lr)[0])
        out["sat_counts"][1] += sat_counts(hsv_sv(hr)[0])
    return out
