"""fp64 restatement of the LPIPS contract (include/sr355.h, the LPIPS section) for the tests: lpips.LPIPS(net="alex"), version 0.1,
spatial = False, eval mode.  The input steps are exact in fp32 by contract (the [3][256] table, or one fp32 subtract and divide), so the
restatement starts from those fp32 values and runs the trunk and the distance in float64 on the CPU (torch conv2d / max_pool2d)."""
import numpy as np
import torch
import torch.nn.functional as F

from sr355.lpips import SCALE, SHIFT, input_table

PADS = (2, 2, 1, 1, 1)


def make_pair(B, H, W, seed):
    """The tests' inputs: hr uniform uint8 BGR, lr = hr + uniform integer noise in [-20, 20], clipped."""
    rng = np.random.default_rng(seed)
    hr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    lr = np.clip(hr.astype(np.int64) + rng.integers(-20, 21, hr.shape), 0, 255).astype(np.uint8)
    return lr, hr


def scaled_from_u8(bgr):
    """uint8 BGR [B,H,W,3] -> the scaled RGB image, float64 holding the contract's fp32 values."""
    tab = input_table()
    rgb = np.asarray(bgr)[..., ::-1]
    return np.stack([tab[c][rgb[..., c]] for c in range(3)], -1).astype(np.float64)


def scaled_from_f32(rgb):
    """float32 RGB [B,H,W,3] in [-1, 1] -> the scaling layer in fp32, widened."""
    x = np.asarray(rgb, dtype=np.float32)
    return ((x - np.asarray(SHIFT, np.float32)) / np.asarray(SCALE, np.float32)).astype(np.float32).astype(np.float64)


def trunk(x, weights, dtype=torch.float64):
    """Scaled image [N,H,W,3] -> the five taps, NHWC arrays of `dtype`."""
    t = torch.from_numpy(np.ascontiguousarray(np.transpose(x, (0, 3, 1, 2)))).to(dtype)
    taps = []
    for i in range(5):
        w = torch.from_numpy(np.ascontiguousarray(np.transpose(weights["conv_w"][i], (3, 2, 0, 1)))).to(dtype)   # HWIO -> OIHW
        b = torch.from_numpy(np.asarray(weights["conv_b"][i])).to(dtype)
        t = F.relu(F.conv2d(t, w, b, stride=4 if i == 0 else 1, padding=PADS[i]))
        taps.append(t.permute(0, 2, 3, 1).contiguous().numpy())
        if i < 2:
            t = F.max_pool2d(t, 3, 2)
    return taps


def distance(fa, fb, lin):
    """One tap's term per pair: mean_{h,w} sum_c l_c (na_c - nb_c)^2, n = f / (sqrt(sum_c f^2) + 1e-10).  Arrays keep their dtype."""
    eps = fa.dtype.type(1e-10)
    na = fa / (np.sqrt((fa * fa).sum(-1, keepdims=True)) + eps)
    nb = fb / (np.sqrt((fb * fb).sum(-1, keepdims=True)) + eps)
    d = ((na - nb) ** 2 * np.asarray(lin).astype(fa.dtype)).sum(-1)
    return d.mean((1, 2))


def lpips_scaled(xa, xb, weights, dtype=torch.float64):
    """-> {'taps': five [2,B,h,w,C], 'terms': [B,5], 'score': [B]} from two scaled image stacks."""
    B = xa.shape[0]
    taps = trunk(np.concatenate([xa, xb]), weights, dtype)
    terms = np.stack([distance(t[:B], t[B:], weights["lin_w"][i]) for i, t in enumerate(taps)], 1)
    return {"taps": [t.reshape((2, B) + t.shape[1:]) for t in taps], "terms": terms, "score": terms.sum(1)}


def lpips_u8(a_bgr, b_bgr, weights, dtype=torch.float64):
    return lpips_scaled(scaled_from_u8(a_bgr), scaled_from_u8(b_bgr), weights, dtype)


def lpips_f32(a_rgb, b_rgb, weights, dtype=torch.float64):
    return lpips_scaled(scaled_from_f32(a_rgb), scaled_from_f32(b_rgb), weights, dtype)
