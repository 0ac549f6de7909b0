"""fp64 NumPy restatement of the classical study's nine image-quality scores (skimage.metrics' PSNR / SSIM and
classic_super_resolution_algorithms/profiling_methods.py:45-167), the contract csrc/metrics.hip implements.

Per pair (hr, sr) of one shape [H, W] or [H, W, 3], each uint8 or float32:
  psnr      10 log10(dr^2 / mean((hr - sr)^2))
  ssim      skimage's default SSIM: 7 x 7 box means, covariances x 49/48, K1 0.01, K2 0.03, mean over the centres 3 pixels inside the
            border; RGB: the mean of the per-channel means
  mae, rmse over all channels as passed; rmse = sqrt(mean(d^2) + 1e-9)
  grad_mse, epi  on sobel_mag of the gray image (_ensure_gray_f32: divided by 255 when its own max > 1.5, in float32)
  hf_ratio  masked |fftshift(fft2(gray))| sums of the unscaled gray values, as the DFT matrix products the device runs
  kl_luma   256-bin gray histograms; kl_color 64 bins per channel, NaN for gray
The gray image of uint8 RGB is OpenCV's COLOR_RGB2GRAY for 8-bit images, the fixed-point Y = (4899 R + 9617 G + 1868 B + 8192) >> 14
(OpenCV's documented 14-bit coefficients).  cv2 is not installed where these tests run, so that formula is not pinned against cv2 itself
here.  A float RGB image has no gray image in this contract (NotImplementedError).

The CPU tests (test_classic_metrics_cpu.py) check each piece against an independent form: np.fft, scipy.ndimage, np.histogram."""
import numpy as np

NAMES = ("psnr", "ssim", "mae", "rmse", "grad_mse", "epi", "hf_ratio", "kl_luma", "kl_color")
DEF_EPS = 1e-9


def rgb2gray_u8(img):
    """OpenCV's COLOR_RGB2GRAY on uint8 RGB (14-bit fixed point, rounded) -> uint8."""
    x = np.asarray(img).astype(np.int64)
    return ((4899 * x[..., 0] + 9617 * x[..., 1] + 1868 * x[..., 2] + 8192) >> 14).astype(np.uint8)


def gray_of(img):
    """The gray image the gray-derived scores see, in the image's own dtype."""
    img = np.asarray(img)
    if img.ndim == 2:
        return img
    if img.dtype == np.uint8:
        return rgb2gray_u8(img)
    raise NotImplementedError("a float RGB image has no gray image here (cv2's float COLOR_RGB2GRAY is not part of this contract)")


def ensure_gray(img):
    """_ensure_gray_f32 (profiling_methods.py:58-68): float32 gray, divided by 255 (in float32) when its own max > 1.5 -> float64."""
    g = gray_of(img).astype(np.float32)
    if g.max() > 1.5:
        g = g / np.float32(255.0)
    return g.astype(np.float64)


def sobel_mag(img):
    """ksize-3 Sobel magnitude with BORDER_REFLECT_101 (np.pad 'reflect') of ensure_gray(img), fp64."""
    g = np.pad(ensure_gray(img), 1, mode="reflect")
    H, W = g.shape[0] - 2, g.shape[1] - 2
    s = lambda dy, dx: g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = (s(-1, 1) - s(-1, -1)) + 2.0 * (s(0, 1) - s(0, -1)) + (s(1, 1) - s(1, -1))
    gy = (s(1, -1) - s(-1, -1)) + 2.0 * (s(1, 0) - s(-1, 0)) + (s(1, 1) - s(-1, 1))
    return np.sqrt(gx * gx + gy * gy)


def _box7(x):
    """7 x 7 window sums at every centre whose window lies inside the image: [H - 6, W - 6]."""
    c = np.zeros((x.shape[0] + 1, x.shape[1] + 1))
    c[1:, 1:] = np.cumsum(np.cumsum(x, 0), 1)
    return c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]


def ssim_map(a, b, dr):
    """skimage's SSIM map (defaults) over the cropped centres of one channel, fp64."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    ux, uy = _box7(a) / 49.0, _box7(b) / 49.0
    uxx, uyy, uxy = _box7(a * a) / 49.0, _box7(b * b) / 49.0, _box7(a * b) / 49.0
    cn = 49.0 / 48.0
    vx, vy, vxy = cn * (uxx - ux * ux), cn * (uyy - uy * uy), cn * (uxy - ux * uy)
    C1, C2 = (0.01 * dr) ** 2, (0.03 * dr) ** 2
    return ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))


def ssim(hr, sr, dr):
    hr, sr = np.asarray(hr), np.asarray(sr)
    if hr.shape[0] < 7 or hr.shape[1] < 7:
        raise ValueError("images smaller than the 7 x 7 window")
    if hr.ndim == 2:
        return float(ssim_map(hr, sr, dr).mean())
    return float(np.mean([ssim_map(hr[..., c], sr[..., c], dr).mean() for c in range(hr.shape[2])]))


def psnr(hr, sr, dr):
    d = np.asarray(hr, np.float64) - np.asarray(sr, np.float64)
    mse = np.mean(d * d)
    with np.errstate(divide="ignore"):
        return float(10.0 * np.log10(float(dr) ** 2 / mse))


def dft_matrix(N):
    """exp(-2 pi i k x / N), the phase k x reduced mod N exactly."""
    k = np.arange(N, dtype=np.int64)
    return np.exp(-2j * np.pi * (np.outer(k, k) % N) / N)


def hf_mask(H, W, radius_frac):
    """The reference's r > radius_frac (r_max + 1e-9) on the fftshift-ed grid, mapped back to unshifted frequency indices."""
    cy, cx = H // 2, W // 2
    dy = (np.arange(H) + cy) % H - cy
    dx = (np.arange(W) + cx) % W - cx
    r = np.sqrt(dy[:, None] ** 2 + dx[None, :] ** 2)
    return r > radius_frac * (np.sqrt(cy * cy + cx * cx) + DEF_EPS)


def hf_ratio(hr_gray, sr_gray, radius_frac=0.6):
    """(sum_mask |F_sr| + 1e-9) / (sum_mask |F_hr| + 1e-9), F = A_H X A_W^T of the unscaled gray values."""
    H, W = hr_gray.shape
    AH, AW = dft_matrix(H), dft_matrix(W)
    m = hf_mask(H, W, radius_frac)
    s = [np.abs(AH @ np.asarray(g, np.float64) @ AW.T)[m].sum() for g in (hr_gray, sr_gray)]
    return float((s[1] + DEF_EPS) / (s[0] + DEF_EPS))


def hist_values(img):
    """What np.histogram(range=(0, 255)) bins (profiling_methods.py:119-126): uint8 as float32, float as clip(x, 0, 1) * 255 in float32."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        return img.astype(np.float32)
    return np.clip(img.astype(np.float32), 0, 1) * np.float32(255.0)


def u8_bin_lut(bins):
    """bin of each uint8 value 0..255, taken from np.histogram itself."""
    return np.array([int(np.argmax(np.histogram(np.float32(v), bins=bins, range=(0, 255))[0])) for v in range(256)])


def hist_counts(img, bins):
    """np.histogram(hist_values(img), bins, range=(0, 255)) counts, restated: ((v / 255) * bins) truncated, the right edge folded into the
    last bin, then corrected by one against the linspace edges; uint8 through u8_bin_lut."""
    img = np.asarray(img)
    if img.dtype == np.uint8:
        idx = u8_bin_lut(bins)[img.reshape(-1)]
    else:
        v = hist_values(img).astype(np.float64).reshape(-1)
        edges = np.arange(bins + 1) * (255.0 / bins)
        idx = np.minimum(((v / 255.0) * bins).astype(np.int64), bins - 1)
        idx -= v < edges[idx]
        idx += (v >= edges[idx + 1]) & (idx != bins - 1)
    return np.bincount(idx, minlength=bins)


def kl_from_counts(p, q, bins):
    n = float(np.sum(p))
    step = 255.0 / bins
    P = p / step / n + 1e-12
    Q = q / step / n + 1e-12
    return float(np.sum(P * np.log(P / Q)))


def kl_luma(hr, sr):
    return kl_from_counts(hist_counts(gray_of(hr), 256), hist_counts(gray_of(sr), 256), 256)


def kl_color(hr, sr):
    hr, sr = np.asarray(hr), np.asarray(sr)
    if hr.ndim == 2:
        return float("nan")
    total = 0.0
    for c in range(hr.shape[2]):
        total += kl_from_counts(hist_counts(hr[..., c], 64), hist_counts(sr[..., c], 64), 64)
    return float(total / hr.shape[2])


def scores(hr, sr, data_range=255.0, radius_frac=0.6):
    """The nine columns of one pair, fp64 (NaN for the gray-derived columns of a float RGB pair, as the device returns them)."""
    hr, sr = np.asarray(hr), np.asarray(sr)
    if data_range == "hr_span":
        span = hr.max() - hr.min()
        data_range = float(span) if span != 0 else 255.0
    dr = float(data_range)
    d = hr.astype(np.float64) - sr.astype(np.float64)
    mse = np.mean(d * d)
    out = {"psnr": psnr(hr, sr, dr), "ssim": ssim(hr, sr, dr), "mae": float(np.mean(np.abs(d))), "rmse": float(np.sqrt(mse + DEF_EPS))}
    try:
        mh, ms = sobel_mag(hr), sobel_mag(sr)
        gh, gs = gray_of(hr), gray_of(sr)
        out.update(grad_mse=float(np.mean((mh - ms) ** 2)), epi=float((ms.sum() + DEF_EPS) / (mh.sum() + DEF_EPS)),
                   hf_ratio=hf_ratio(gh.astype(np.float32), gs.astype(np.float32), radius_frac), kl_luma=kl_luma(hr, sr))
    except NotImplementedError:
        out.update(grad_mse=float("nan"), epi=float("nan"), hf_ratio=float("nan"), kl_luma=float("nan"))
    out["kl_color"] = kl_color(hr, sr)
    return np.array([out[k] for k in NAMES])
