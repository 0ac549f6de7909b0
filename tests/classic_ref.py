"""NumPy fp64 restatements of the classical study's back-projection, noise sigma + non-local means, edge-guided interpolation and
frequency extrapolation (reference classic_algorithms.py:23-108), written from the formulas the module docstring of
SRModels/classic_super_resolution_algorithms/classic_algorithms.py states.  The cv2.resize steps use oracle.ops's restatements of
OpenCV's tap tables.  Images are 2-D uint8 [h, w]."""
import numpy as np

from oracle import ops as O

NORM_PPF_075 = 0.6744897501960817
DB2_DEC_HI = np.array([-0.48296291314469025, 0.836516303737469, -0.22414386804185735, -0.12940952255092145])


# ---------------------------------------------------------------------------------------------------- resize helpers
def resize_f32(img, out_h, out_w, interpolation):
    """cv2.resize on a float32 [h, w] image with sr_resize's rule: an exact 2x INTER_LINEAR shrink is the 2 x 2 area mean."""
    h, w = img.shape
    if interpolation == O.INTER_LINEAR and w == 2 * out_w and h == 2 * out_h:
        interpolation = O.INTER_AREA
    return O.cv_resize(np.asarray(img, np.float32)[:, :, None], out_h, out_w, interpolation)[:, :, 0]


def resize_f64(img, out_h, out_w, interpolation):
    """cv2.resize on a float64 image: float tap weights, double arithmetic, horizontal pass first."""
    h, w = img.shape
    ix, wx = O.resize_axis_taps(w, out_w, interpolation)
    iy, wy = O.resize_axis_taps(h, out_h, interpolation)
    img = np.asarray(img, np.float64)
    tmp = np.zeros((h, out_w))
    for k in range(ix.shape[1]):
        tmp = tmp + img[:, ix[:, k]] * wx[None, :, k].astype(np.float64)
    out = np.zeros((out_h, out_w))
    for k in range(iy.shape[1]):
        out = out + tmp[iy[:, k], :] * wy[:, k, None].astype(np.float64)
    return out


# ---------------------------------------------------------------------------------------------------- back-projection
def back_projection(hr_u8, lr_u8, iterations=10):
    """-> (uint8 output, float32 estimate before the clip)."""
    H, W = hr_u8.shape
    h, w = lr_u8.shape
    hr = hr_u8.astype(np.float32)
    lr = lr_u8.astype(np.float32)
    for _ in range(iterations):
        diff = (lr - resize_f32(hr, h, w, O.INTER_LINEAR)).astype(np.float32)
        hr = (hr + resize_f32(diff, H, W, O.INTER_LINEAR)).astype(np.float32)
    return np.clip(hr, 0, 255).astype(np.uint8), hr


# ---------------------------------------------------------------------------------------------------- noise sigma
def _db2_hi_axis0(x):
    """pywt's downsampling convolution along axis 0 with 'symmetric' extension: d[o] = sum_j hi[j] x[2o+1-j], (n+3)//2 outputs,
    evaluated as sum_{j<3} hi[j] (x[2o+1-j] - x[2o-2]) (db2's high-pass annihilates constants)."""
    n = x.shape[0]
    o = np.arange((n + 3) // 2)
    period = 2 * n

    def ext(i):
        i = np.mod(i, period)
        return np.where(i < n, i, period - 1 - i)

    base = x[ext(2 * o - 2)]
    s = np.zeros((len(o),) + x.shape[1:])
    for j in range(3):
        s = s + DB2_DEC_HI[j] * (x[ext(2 * o + 1 - j)] - base)
    return s


def db2_hh(x):
    """The 'dd' band of pywt.dwtn(x, 'db2') (axis 0, then axis 1)."""
    t = _db2_hi_axis0(np.asarray(x, np.float64))
    return _db2_hi_axis0(t.T).T


def noise_sigma(x):
    """estimate_sigma on the uint8 values: median(|dd| over the non-zero entries) / norm.ppf(0.75); NaN when all are zero."""
    d = np.abs(db2_hh(x)).ravel()
    d = d[d != 0]
    if d.size == 0:
        return float("nan")
    return float(np.median(d) / NORM_PPF_075)


# ---------------------------------------------------------------------------------------------------- non-local means
def nl_means(x_u8, h, patch=5, distance=6):
    """skimage's fast 2-D NL-means on x / 255 as the per-pixel gather: y[p] = sum_t w P[p+t] / sum_t w over t in [-d, d]^2,
    D = sum_{k in [-s, s]^2} (P[p+k] - P[p+t+k])^2 (exact integer SSD of the uint8 values / 255^2), dist = D / (h^2 patch^2),
    w = exp(-dist) if dist <= 5 else 0.  The image is reflect-padded (numpy 'reflect')."""
    s = patch // 2
    R = s + distance
    hh, ww = x_u8.shape
    P = np.pad(x_u8.astype(np.int64), R, mode="reflect")
    h2s2 = h * h * patch * patch
    num = np.zeros((hh, ww))
    den = np.zeros((hh, ww))
    core = P[R:R + hh, R:R + ww].astype(np.float64)
    for ty in range(-distance, distance + 1):
        for tx in range(-distance, distance + 1):
            sq = (P[distance:distance + hh + 2 * s, distance:distance + ww + 2 * s]
                  - P[distance + ty:distance + ty + hh + 2 * s, distance + tx:distance + tx + ww + 2 * s]) ** 2
            c = np.cumsum(np.cumsum(np.pad(sq, ((1, 0), (1, 0))), axis=0), axis=1)
            D = c[patch:, patch:] - c[:-patch, patch:] - c[patch:, :-patch] + c[:-patch, :-patch]
            dist = D.astype(np.float64) / 65025.0 / h2s2
            wgt = np.where(dist <= 5.0, np.exp(-np.minimum(dist, 5.0)), 0.0)
            den += wgt
            num += wgt * P[R + ty:R + ty + hh, R + tx:R + tx + ww]
    del core
    return num / 255.0 / den


def nl_means_dist(x_u8, h, patch=5, distance=6):
    """nl_means' own `dist` of every (shift, pixel) pair, [(2d+1)^2, h, w] in its shift order, and the shifted pixel values beside it (the same
    expressions as in nl_means; tests/test_classic_args_cpu.py holds nl_means_of_dist(dist, vals, dist <= 5) to nl_means bit for bit)."""
    s = patch // 2
    R = s + distance
    hh, ww = x_u8.shape
    P = np.pad(x_u8.astype(np.int64), R, mode="reflect")
    h2s2 = h * h * patch * patch
    dist, vals = [], []
    for ty in range(-distance, distance + 1):
        for tx in range(-distance, distance + 1):
            sq = (P[distance:distance + hh + 2 * s, distance:distance + ww + 2 * s]
                  - P[distance + ty:distance + ty + hh + 2 * s, distance + tx:distance + tx + ww + 2 * s]) ** 2
            c = np.cumsum(np.cumsum(np.pad(sq, ((1, 0), (1, 0))), axis=0), axis=1)
            D = c[patch:, patch:] - c[:-patch, patch:] - c[patch:, :-patch] + c[:-patch, :-patch]
            dist.append(D.astype(np.float64) / 65025.0 / h2s2)
            vals.append(P[R + ty:R + ty + hh, R + tx:R + tx + ww])
    return np.stack(dist), np.stack(vals)


def nl_means_of_dist(dist, vals, keep):
    """nl_means' weighted mean from nl_means_dist's arrays, with the weights of the pairs where `keep` is false dropped."""
    num = np.zeros(dist.shape[1:])
    den = np.zeros(dist.shape[1:])
    for d, v, k in zip(dist, vals, keep):
        wgt = np.where(k, np.exp(-np.minimum(d, 5.0)), 0.0)
        den += wgt
        num += wgt * v
    return num / 255.0 / den


def nl_means_pairloop(x_u8, h, patch=5, distance=6):
    """The same denoising as skimage's fast-mode loop runs it: pad by s + d + 1, for each shift (t_row, t_col >= 0) an integral image
    of the squared differences, the patch distance from four corners, and each pair (p, p+t) visited once, with weight alpha*w added
    to both ends (alpha = 0.5 for t_col == 0, whose shifts come in +-t_row pairs)."""
    s = patch // 2
    pad = s + distance + 1
    img = x_u8.astype(np.float64) / 255.0
    Pd = np.pad(img, pad, mode="reflect")
    n_row, n_col = Pd.shape
    weights = np.zeros_like(Pd)
    result = np.zeros_like(Pd)
    h2s2 = h * h * patch * patch
    for t_row in range(-distance, distance + 1):
        r0, r1 = max(s, s - t_row), min(n_row - s, n_row - s - t_row)
        for t_col in range(0, distance + 1):
            alpha = 0.5 if t_col == 0 else 1.0
            c0, c1 = max(s, s - t_col), min(n_col - s, n_col - s - t_col)
            integral = np.zeros_like(Pd)
            rr0, rr1 = max(1, -t_row), min(n_row, n_row - t_row)
            cc0, cc1 = max(1, -t_col), min(n_col, n_col - t_col)
            sq = np.zeros_like(Pd)
            sq[rr0:rr1, cc0:cc1] = (Pd[rr0:rr1, cc0:cc1] - Pd[rr0 + t_row:rr1 + t_row, cc0 + t_col:cc1 + t_col]) ** 2
            integral = np.cumsum(np.cumsum(sq, axis=0), axis=1)
            rows = np.arange(r0, r1)[:, None]
            cols = np.arange(c0, c1)[None, :]
            dist = (integral[rows + s, cols + s] + integral[rows - s - 1, cols - s - 1]
                    - integral[rows - s - 1, cols + s] - integral[rows + s, cols - s - 1])
            dist = np.maximum(dist, 0.0) / h2s2
            w = np.where(dist <= 5.0, alpha * np.exp(-np.minimum(dist, 5.0)), 0.0)
            weights[r0:r1, c0:c1] += w
            weights[r0 + t_row:r1 + t_row, c0 + t_col:c1 + t_col] += w
            result[r0:r1, c0:c1] += w * Pd[r0 + t_row:r1 + t_row, c0 + t_col:c1 + t_col]
            result[r0 + t_row:r1 + t_row, c0 + t_col:c1 + t_col] += w * Pd[r0:r1, c0:c1]
    out = result / np.where(weights > 0, weights, 1.0)
    return out[pad:-pad, pad:-pad]


def non_local_means(hr_shape, lr_u8, h_scale=1.15):
    """-> (float64 [H, W] after Lanczos-4, denoised [h, w], sigma)."""
    sigma = noise_sigma(lr_u8)
    den = nl_means(lr_u8, h_scale * sigma)
    return resize_f64(den, hr_shape[0], hr_shape[1], O.INTER_LANCZOS4), den, sigma


# ---------------------------------------------------------------------------------------------------- edge-guided
def sobel_mag(x_u8):
    """hypot(Sobel_x, Sobel_y), ksize 3, BORDER_REFLECT_101 (numpy 'reflect'), float64."""
    P = np.pad(x_u8.astype(np.int64), 1, mode="reflect")
    h, w = x_u8.shape

    def at(dy, dx):
        return P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    gx = (at(-1, 1) - at(-1, -1)) + 2 * (at(0, 1) - at(0, -1)) + (at(1, 1) - at(1, -1))
    gy = (at(1, -1) - at(-1, -1)) + 2 * (at(1, 0) - at(-1, 0)) + (at(1, 1) - at(-1, 1))
    return np.hypot(gx.astype(np.float64), gy.astype(np.float64)), gx, gy


def edge_guided(x_u8, H, W, weight=0.3):
    """-> (uint8 [H, W], float32 up-sized edges)."""
    edges = sobel_mag(x_u8)[0]
    up = O.cv_resize_u8(x_u8[:, :, None], H, W, O.INTER_LINEAR)[:, :, 0]
    up_e = resize_f64(edges, H, W, O.INTER_LINEAR).astype(np.float32)
    s = (up.astype(np.float32) * np.float32(1.0) + up_e * np.float32(weight)) + np.float32(0.0)
    return np.clip(s, 0, 255).astype(np.uint8), up_e


# ---------------------------------------------------------------------------------------------------- frequency extrapolation
def dft_operator(N, n):
    """A_{N,n}[y, x] = (1/N) sum_{k=-(n//2)}^{n-1-n//2} exp(2 pi i k (y n - x N) / (N n)), phase reduced exactly in integers."""
    y = np.arange(N, dtype=np.int64)[:, None]
    x = np.arange(n, dtype=np.int64)[None, :]
    acc = np.zeros((N, n), complex)
    for k in range(-(n // 2), n - n // 2):
        m = np.mod(k * (y * n - x * N), N * n)
        acc += np.exp(2j * np.pi * m / (N * n))
    return acc / N


def freq_extrapolate(x, H, W):
    """|A_H X A_W^T| in float64."""
    X = np.asarray(x, np.float64)
    return np.abs(dft_operator(H, X.shape[0]) @ X @ dft_operator(W, X.shape[1]).T)


def freq_extrapolate_fft(x, H, W):
    """The reference's procedure: fftshift(fft2), zero-pad centred to H x W, ifftshift, |ifft2|."""
    f = np.fft.fftshift(np.fft.fft2(np.asarray(x, np.float64)))
    h, w = f.shape
    pad = np.zeros((H, W), complex)
    r0, c0 = H // 2 - h // 2, W // 2 - w // 2
    pad[r0:r0 + h, c0:c0 + w] = f
    return np.abs(np.fft.ifft2(np.fft.ifftshift(pad)))
