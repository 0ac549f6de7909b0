"""Host side of the device LPIPS (csrc/lpips.hip; contract in include/sr355.h): the weights of lpips.LPIPS(net="alex") -- read from the
user's two checkpoints or seeded for tests and benchmarks -- and the fp32 input table.  Importing this module needs no GPU.

A weights value is a dict {"conv_w": five HWIO float32 kernels, "conv_b": five biases, "lin_w": five [C] vectors}, what
Context.lpips_set_weights takes."""
import os

import numpy as np

CONV_SHAPES = ((11, 11, 3, 64), (5, 5, 64, 192), (3, 3, 192, 384), (3, 3, 384, 256), (3, 3, 256, 256))   # HWIO
TAP_CHANNELS = tuple(s[3] for s in CONV_SHAPES)
ALEXNET_CONVS = (0, 3, 6, 8, 10)          # indices of the convs in torchvision's AlexNet.features
SHIFT = (-.030, -.088, -.188)             # the scaling layer, per R, G, B
SCALE = (.458, .448, .450)


def conv_keys(i):
    return f"features.{ALEXNET_CONVS[i]}.weight", f"features.{ALEXNET_CONVS[i]}.bias"


def lin_key(i):
    return f"lin{i}.model.1.weight"


def input_table():
    """[3][256] float32, [c][v] for c = R, G, B: the notebook's to_tensor (2 (v / 255.0) - 1 in fp64, rounded to fp32) followed by the
    scaling layer (x - shift) / scale in fp32.  The library builds the same table (sr_lpips_input_table)."""
    x = (2.0 * (np.arange(256, dtype=np.float64) / 255.0) - 1.0).astype(np.float32)
    return np.stack([(x - np.float32(SHIFT[c])) / np.float32(SCALE[c]) for c in range(3)]).astype(np.float32)


def tap_shapes(H, W):
    """The five tap sizes [(h, w)] of an H x W image (sr_lpips_shapes); ValueError below 31 or above H, W <= 4096, H W <= 2^22."""
    import ctypes as C
    from . import _lib
    hw = (C.c_int * 10)()
    if _lib.load().sr_lpips_shapes(int(H), int(W), hw) != _lib.SR_OK:
        raise ValueError(f"lpips: images are 31 <= H, W <= 4096 with H * W <= 2^22, got {H} x {W}")
    return [(hw[2 * i], hw[2 * i + 1]) for i in range(5)]


def seeded_weights(seed):
    """Weights for tests and benchmarks: convs N(0, 2 / fan_in), biases U(-.05, .05), lins |N(0, 1 / C)| (the real lin weights are
    non-negative)."""
    rng = np.random.default_rng(seed)
    conv_w = [(rng.standard_normal(s) * np.sqrt(2.0 / (s[0] * s[1] * s[2]))).astype(np.float32) for s in CONV_SHAPES]
    conv_b = [rng.uniform(-.05, .05, s[3]).astype(np.float32) for s in CONV_SHAPES]
    lin_w = [np.abs(rng.standard_normal(c) * np.sqrt(1.0 / c)).astype(np.float32) for c in TAP_CHANNELS]
    return {"conv_w": conv_w, "conv_b": conv_b, "lin_w": lin_w}


def to_state_dicts(weights):
    """(AlexNet state dict, LPIPS state dict) of NumPy arrays under the checkpoints' key names and layouts (OIHW convs, [1,C,1,1] lins)."""
    alex, lins = {}, {}
    for i in range(5):
        kw, kb = conv_keys(i)
        alex[kw] = np.ascontiguousarray(np.transpose(weights["conv_w"][i], (3, 2, 0, 1)))
        alex[kb] = np.asarray(weights["conv_b"][i])
        lins[lin_key(i)] = np.asarray(weights["lin_w"][i]).reshape(1, -1, 1, 1)
    return alex, lins


def _read(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f"lpips.load_weights: no such file: {path}")
    if str(path).lower().endswith(".npz"):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    import torch
    sd = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(sd, dict):
        raise ValueError(f"lpips.load_weights: {path} does not hold a state dict")
    return {k: v.detach().cpu().numpy() for k, v in sd.items() if hasattr(v, "detach")}


def load_weights(alexnet=None, lpips=None):
    """The weights from torchvision's AlexNet checkpoint (keys features.{0,3,6,8,10}.{weight,bias}, OIHW) and the lpips package's alex.pth
    (keys lin{0..4}.model.1.weight, [1,C,1,1]), both torch checkpoints, or from one .npz holding the same fifteen arrays under those names
    (given as either argument).  FileNotFoundError for a missing file, ValueError naming the key for a missing key or a wrong shape."""
    paths = [p for p in (alexnet, lpips) if p is not None]
    if not paths:
        raise ValueError("lpips.load_weights: give the AlexNet and LPIPS checkpoints, or one .npz")
    arrays = {}
    for p in dict.fromkeys(os.fspath(p) for p in paths):
        arrays.update(_read(p))

    def get(key, shape):
        if key not in arrays:
            raise ValueError(f"lpips.load_weights: key {key!r} is missing")
        a = np.asarray(arrays[key])
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"lpips.load_weights: {key!r} has shape {tuple(a.shape)}, expected {tuple(shape)}")
        return a.astype(np.float32)

    out = {"conv_w": [], "conv_b": [], "lin_w": []}
    for i, (kh, kw_, ci, co) in enumerate(CONV_SHAPES):
        kw, kb = conv_keys(i)
        out["conv_w"].append(np.ascontiguousarray(np.transpose(get(kw, (co, ci, kh, kw_)), (2, 3, 1, 0))))   # OIHW -> HWIO
        out["conv_b"].append(np.ascontiguousarray(get(kb, (co,))))
    for i, c in enumerate(TAP_CHANNELS):
        out["lin_w"].append(np.ascontiguousarray(get(lin_key(i), (1, c, 1, 1)).reshape(c)))
    return out


def check_weights(weights):
    """The dict as contiguous float32 arrays of the contract's shapes; ValueError otherwise."""
    out = {}
    try:
        groups = {k: list(weights[k]) for k in ("conv_w", "conv_b", "lin_w")}
    except (KeyError, TypeError) as e:
        raise ValueError("lpips weights: a dict with 'conv_w', 'conv_b' and 'lin_w', five arrays each") from e
    want = {"conv_w": CONV_SHAPES, "conv_b": tuple((c,) for c in TAP_CHANNELS), "lin_w": tuple((c,) for c in TAP_CHANNELS)}
    for k, arrs in groups.items():
        if len(arrs) != 5:
            raise ValueError(f"lpips weights: {k} holds {len(arrs)} arrays, expected 5")
        out[k] = []
        for i, a in enumerate(arrs):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
            if tuple(a.shape) != tuple(want[k][i]):
                raise ValueError(f"lpips weights: {k}[{i}] has shape {tuple(a.shape)}, expected {tuple(want[k][i])}")
            out[k].append(a)
    return out
