"""NumPy restatement of the dataset-synthesis stages (reference data/common_methods.py::degrade_image; the device side is csrc/degrade.hip,
the contract include/sr355.h): the two 8-bit blurs, the noise stage with its Philox4x32-10 generator, and the baseline-JPEG round trip that
cv2.imencode / cv2.imdecode compute with libjpeg's defaults (4:2:0, "islow" integer DCTs, fancy up-sampling).  Plain integer arithmetic on
whole planes; nothing here follows the kernels' tiling.  Images are uint8 BGR [H, W, 3]."""
import numpy as np

INTERP_NAMES = ("INTER_LINEAR", "INTER_CUBIC", "INTER_AREA", "INTER_LANCZOS4")
INTERP_CODES = (1, 2, 3, 4)


# ---------------------------------------------------------------------------------------------- blurs
def reflect101(i, n):
    i = np.abs(np.asarray(i))
    return np.where(i >= n, 2 * n - 2 - i, i)


def gauss_taps(ksize, sigma):
    """Integer 8.8 taps that sum to 256: t_i = floor(256 g_i / sum g + 0.5), the centre tap takes the residue."""
    r = ksize // 2
    g = np.exp(-((np.arange(ksize, dtype=np.float64) - r) ** 2) / (2.0 * float(sigma) ** 2))
    t = np.floor(256.0 * g / g.sum() + 0.5).astype(np.int64)
    t[r] += 256 - int(t.sum())
    return t


def gaussian_blur(img, taps):
    """(sum_j t_j sum_i t_i p[y + j - r, x + i - r] + 32768) >> 16 per channel, BORDER_REFLECT_101."""
    a = np.asarray(img).astype(np.int64)
    H, W = a.shape[:2]
    k = len(taps)
    r = k // 2
    hor = sum(int(taps[i]) * a[:, reflect101(np.arange(W) + i - r, W)] for i in range(k))
    ver = sum(int(taps[j]) * hor[reflect101(np.arange(H) + j - r, H)] for j in range(k))
    return ((ver + 32768) >> 16).astype(np.uint8)


def motion_blur(img, size):
    """filter2D with a centre row of 1 / size: (2 sum p + size) // (2 size), BORDER_REFLECT_101."""
    a = np.asarray(img).astype(np.int64)
    W = a.shape[1]
    r = size // 2
    s = sum(a[:, reflect101(np.arange(W) + i - r, W)] for i in range(size))
    return ((2 * s + size) // (2 * size)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- noise
def noise_apply(img, field):
    """np.clip(img.astype(float32) + field, 0, 255).astype(uint8), field float32."""
    v = np.asarray(img).astype(np.float32) + np.asarray(field, dtype=np.float32)
    return np.minimum(np.maximum(v, np.float32(0)), np.float32(255)).astype(np.uint8)


PHILOX_M0, PHILOX_M1, PHILOX_W0, PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Vectorised: counter [..., 4], key [..., 2] (or broadcastable) uint32 -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(key)[..., i].astype(np.uint64) for i in range(2))
    m = np.uint64(MASK32)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & m, (k1 + np.uint64(PHILOX_W1)) & m
        p0, p1 = np.uint64(PHILOX_M0) * c[0], np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & m]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def philox4x32_10_scalar(counter, key):
    """The same rounds on Python integers, one counter at a time."""
    c0, c1, c2, c3 = (int(v) for v in counter)
    k0, k1 = (int(v) for v in key)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
    return (c0, c1, c2, c3)


def philox_words(seed, image, n):
    """The first n words of image `image`'s stream: counter (e // 4, 0, image, 0), key the 64-bit seed, word e % 4."""
    nb = (n + 3) // 4
    ctr = np.zeros((nb, 4), np.uint32)
    ctr[:, 0] = np.arange(nb, dtype=np.uint32)
    ctr[:, 2] = image
    key = np.array([seed & MASK32, (seed >> 32) & MASK32], np.uint32)
    return philox4x32_10(ctr, key[None]).reshape(-1)[:n + (-n) % 4]


def philox_normal(seed, image, shape):
    """fp64 Box-Muller per pair of words: u1 = ((x0 >> 8) + 1) 2^-24, u2 = (x1 >> 8) 2^-24, z = sqrt(-2 ln u1) (cos, sin)(2 pi u2)."""
    n = int(np.prod(shape))
    w = philox_words(seed, image, n).reshape(-1, 2).astype(np.int64)
    u1 = ((w[:, 0] >> 8) + 1).astype(np.float64) * 2.0 ** -24
    u2 = (w[:, 1] >> 8).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.stack([rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)], -1).reshape(-1)
    return z[:n].reshape(shape)


def noise_from_z(img, z, std):
    """The kernel path's last step: n = float32(std) * float32(z) (one rounding), then noise_apply."""
    return noise_apply(img, np.float32(std) * np.asarray(z, dtype=np.float32))


# ---------------------------------------------------------------------------------------------- JPEG
# ITU-T T.81 Annex K, tables K.1 and K.2, in natural (row-major) order
K1_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
                   np.int64).reshape(8, 8)
K2_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                     + [99] * 32, np.int64).reshape(8, 8)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def quant_tables(quality):
    """jpeg_set_quality(q, force_baseline): scale 5000 / q below 50, 200 - 2 q from 50 up; (base scale + 50) / 100 clamped to 1..255.
    -> (luma, chroma) int64 [8, 8], natural order."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * scale + 50) // 100, 1, 255) for b in (K1_LUMA, K2_CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def bgr_to_ycc(img):
    b, g, r = (np.asarray(img)[..., i].astype(np.int64) for i in range(3))
    half = 1 << 15
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + (128 << 16) + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + (128 << 16) + half - 1) >> 16
    return y, cb, cr


def ycc_to_bgr(y, cb, cr):
    half = 1 << 15
    u, v = cb - 128, cr - 128
    r = y + ((_fix(1.40200) * v + half) >> 16)
    g = y + ((-_fix(0.34414) * u - _fix(0.71414) * v + half) >> 16)
    b = y + ((_fix(1.77200) * u + half) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def _pad_edge(p, h, w):
    return np.pad(p, ((0, h - p.shape[0]), (0, w - p.shape[1])), mode="edge")


def downsample_h2v2(p):
    """libjpeg's h2v2_downsample with its padding: columns replicated to twice the chroma plane's block width, rows to an even count;
    (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2 ... along a row; then the last CHROMA row replicated to whole blocks."""
    H, W = p.shape
    wc, hc = 8 * ((W + 15) // 16), (H + 1) // 2
    q = _pad_edge(p, 2 * hc, 2 * wc)
    bias = 1 + (np.arange(wc) & 1)
    d = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + bias[None, :]) >> 2
    return _pad_edge(d, 8 * ((H + 15) // 16), wc)


F_0_298631336, F_0_390180644, F_0_541196100, F_0_765366865, F_0_899976223, F_1_175875602 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501321110, F_1_847759065, F_1_961570560, F_2_053119869, F_2_562915447, F_3_072711026 = 12299, 15137, 16069, 16819, 20995, 25172


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """One pass of jpeg_fdct_islow along the last axis of d [..., 8] (13-bit constants; pass 1 keeps 2 extra bits)."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    sh = 13 - 2 if first else 13 + 2
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541196100
    o[2] = _descale(z1 + t13 * F_0_765366865, sh)
    o[6] = _descale(z1 - t12 * F_1_847759065, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175875602
    t4, t5, t6, t7 = t4 * F_0_298631336, t5 * F_2_053119869, t6 * F_3_072711026, t7 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh), _descale(t6 + z2 + z3, sh), _descale(t7 + z1 + z4, sh)
    return np.stack(o, -1)


def _idct_1d(c, first):
    """One pass of jpeg_idct_islow along the last axis of c [..., 8]."""
    z2, z3 = c[..., 2], c[..., 6]
    z1 = (z2 + z3) * F_0_541196100
    t2, t3 = z1 - z3 * F_1_847759065, z1 + z2 * F_0_765366865
    t0, t1 = (c[..., 0] + c[..., 4]) << 13, (c[..., 0] - c[..., 4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c[..., 7], c[..., 5], c[..., 3], c[..., 1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175875602
    t0, t1, t2, t3 = t0 * F_0_298631336, t1 * F_2_053119869, t2 * F_3_072711026, t3 * F_1_501321110
    z1, z2, z3, z4 = -z1 * F_0_899976223, -z2 * F_2_562915447, -z3 * F_1_961570560 + z5, -z4 * F_0_390180644 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    sh = 13 - 2 if first else 13 + 2 + 3
    return np.stack([_descale(v, sh) for v in (t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3)], -1)


def _blocks(p):
    """[8 n, 8 m] -> [n, m, 8 (row), 8 (column)]"""
    n, m = p.shape[0] // 8, p.shape[1] // 8
    return p.reshape(n, 8, m, 8).transpose(0, 2, 1, 3)


def _unblocks(b):
    n, m = b.shape[:2]
    return b.transpose(0, 2, 1, 3).reshape(8 * n, 8 * m)


def plane_codec(p, qt):
    """Level shift, forward DCT, quantisation (round half away from zero), dequantisation, inverse DCT, range limit, of a plane whose
    sides are multiples of 8 -> (quantised coefficients int64 in the plane's layout, decoded uint8 plane)."""
    b = _blocks(p.astype(np.int64) - 128)
    f = _fdct_1d(b, True)                                                   # rows
    f = _fdct_1d(f.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)      # columns; 8 x the DCT
    div = qt[None, None] * 8
    q = np.sign(f) * ((np.abs(f) + (div >> 1)) // div)
    w = _idct_1d((q * qt[None, None]).transpose(0, 1, 3, 2), True).transpose(0, 1, 3, 2)    # columns first, as libjpeg
    o = _idct_1d(w, False)
    return _unblocks(q), np.clip(_unblocks(o) + 128, 0, 255).astype(np.uint8)


def upsample_h2v2_fancy(c, H, W):
    """libjpeg's h2v2_fancy_upsample on the chroma plane's real part [ceil(H/2), ceil(W/2)] -> [H, W]: 3/4 nearer + 1/4 further row
    (the edge rows taking themselves), then the same triangle along the row with the rounding biases 8 / 7 for even / odd columns."""
    hc, wc = (H + 1) // 2, (W + 1) // 2
    c = c[:hc, :wc].astype(np.int64)
    rows = np.arange(2 * hc)
    near = rows >> 1
    far = np.clip(np.where(rows & 1, near + 1, near - 1), 0, hc - 1)
    s = 3 * c[near] + c[far]                                                # [2 hc, wc]
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((2 * hc, 2 * wc), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:H, :W]


def jpeg_roundtrip(img, quality, raw=False):
    """cv2.imdecode(cv2.imencode('.jpeg', img, [IMWRITE_JPEG_QUALITY, q])[1], 1) without the (lossless) entropy coding.
    raw=True -> (out, dict: 'coef_y' [8 ceil(H/8), 8 ceil(W/8)], 'coef_cb', 'coef_cr' [8 ceil(H/16), 8 ceil(W/16)] quantised coefficients in
    plane layout (block (i, j)'s coefficient (v, u) at (8 i + v, 8 j + u)), 'y', 'cb', 'cr' the decoded uint8 planes of those sizes)."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    ql, qc = quant_tables(quality)
    y, cb, cr = bgr_to_ycc(img)
    planes = {"y": _pad_edge(y, 8 * ((H + 7) // 8), 8 * ((W + 7) // 8)), "cb": downsample_h2v2(cb), "cr": downsample_h2v2(cr)}
    inter = {}
    for k, p in planes.items():
        inter["coef_" + k], inter[k] = plane_codec(p, ql if k == "y" else qc)
    out = ycc_to_bgr(inter["y"][:H, :W].astype(np.int64), upsample_h2v2_fancy(inter["cb"], H, W), upsample_h2v2_fancy(inter["cr"], H, W))
    return (out, inter) if raw else out


# ---------------------------------------------------------------------------------------------- the chain
def degrade_with_record(img, rec, noise_field=None):
    """The reference's stage order driven by a draw record (data.common_methods.draw_degradation): keys gauss_ksize / gauss_sigma (or None),
    motion_size, interp_code, lr_size (w, h), noise_std, jpeg_quality; noise_field overrides rec['noise']."""
    from oracle import ops as O
    x = np.asarray(img)
    if rec["gauss_ksize"]:
        x = gaussian_blur(x, gauss_taps(rec["gauss_ksize"], rec["gauss_sigma"]))
    if rec["motion_size"]:
        x = motion_blur(x, rec["motion_size"])
    w, h = rec["lr_size"]
    x = O.cv_resize_u8(x, h, w, rec["interp_code"])
    if rec["noise_std"] is not None:
        x = noise_apply(x, rec["noise"] if noise_field is None else noise_field)
    if rec["jpeg_quality"]:
        x = jpeg_roundtrip(x, rec["jpeg_quality"])
    return x
