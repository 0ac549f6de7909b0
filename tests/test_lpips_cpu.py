"""The host side of the device LPIPS: the pure shape function, the fp64 restatement the GPU tests compare against, the input table, the
conv1 identity the kernels rely on, the checkpoint loader and the EDA's scenario sort.  Nothing here needs a GPU."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_ref as R
from sr355 import _lib
from sr355 import lpips as LP


# ---------------------------------------------------------------------------------------------------- sr_lpips_shapes
def torch_shapes(H, W):
    """Output shapes of torchvision AlexNet's features at the five ReLUs, from torch's own conv2d / max_pool2d on one-channel stand-ins."""
    x = torch.zeros(1, 1, H, W)
    k = lambda n: torch.zeros(1, 1, n, n)
    out = []
    x = F.conv2d(x, k(11), stride=4, padding=2); out.append(tuple(x.shape[2:]))
    x = F.conv2d(F.max_pool2d(x, 3, 2), k(5), padding=2); out.append(tuple(x.shape[2:]))
    x = F.conv2d(F.max_pool2d(x, 3, 2), k(3), padding=1); out.append(tuple(x.shape[2:]))
    return out + [out[-1], out[-1]]


def test_shapes_match_torch():
    for H in range(31, 81):
        for W in range(31, 81):
            assert LP.tap_shapes(H, W) == torch_shapes(H, W), (H, W)
    for H, W in ((239, 239), (478, 478), (478, 850)):
        assert LP.tap_shapes(H, W) == torch_shapes(H, W), (H, W)
    assert LP.tap_shapes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]


@pytest.mark.parametrize("H,W", [(30, 40), (40, 30), (4097, 40), (40, 4097), (2049, 2048), (4096, 1025), (0, 0), (-5, 64)])
def test_shapes_refused(H, W):
    hw = (C.c_int * 10)()
    assert _lib.load().sr_lpips_shapes(H, W, hw) == _lib.SR_ERR_INVALID
    with pytest.raises(ValueError):
        LP.tap_shapes(H, W)
    assert _lib.load().sr_lpips_shapes(64, 64, None) == _lib.SR_ERR_INVALID


def test_shapes_at_the_limits_are_taken():
    assert LP.tap_shapes(2048, 2048) == torch_shapes(2048, 2048)
    assert LP.tap_shapes(1024, 4096) == torch_shapes(1024, 4096)


# ---------------------------------------------------------------------------------------------------- the fp64 restatement
def naive_lpips(xa, xb, w):
    """A second derivation in plain NumPy loops, fp64: scaled images [H,W,3] -> (five terms, score)."""
    def conv(x, k, b, stride, pad):
        K = k.shape[0]
        xp = np.zeros((x.shape[0] + 2 * pad, x.shape[1] + 2 * pad, x.shape[2]))
        xp[pad:pad + x.shape[0], pad:pad + x.shape[1]] = x
        oh, ow = (xp.shape[0] - K) // stride + 1, (xp.shape[1] - K) // stride + 1
        y = np.zeros((oh, ow, k.shape[3]))
        for i in range(oh):
            for j in range(ow):
                y[i, j] = np.tensordot(xp[i * stride:i * stride + K, j * stride:j * stride + K], k, 3) + b
        return np.maximum(y, 0.0)

    def pool(x):
        oh, ow = (x.shape[0] - 3) // 2 + 1, (x.shape[1] - 3) // 2 + 1
        y = np.zeros((oh, ow, x.shape[2]))
        for i in range(oh):
            for j in range(ow):
                y[i, j] = x[2 * i:2 * i + 3, 2 * j:2 * j + 3].max((0, 1))
        return y

    def taps(x):
        out = []
        for i in range(5):
            x = conv(x, w["conv_w"][i].astype(np.float64), w["conv_b"][i].astype(np.float64), 4 if i == 0 else 1, R.PADS[i])
            out.append(x)
            if i < 2:
                x = pool(x)
        return out

    terms = []
    for fa, fb, lin in zip(taps(xa), taps(xb), w["lin_w"]):
        total = 0.0
        for i in range(fa.shape[0]):
            for j in range(fa.shape[1]):
                na = fa[i, j] / (math.sqrt(float((fa[i, j] ** 2).sum())) + 1e-10)
                nb = fb[i, j] / (math.sqrt(float((fb[i, j] ** 2).sum())) + 1e-10)
                total += float((lin.astype(np.float64) * (na - nb) ** 2).sum())
        terms.append(total / (fa.shape[0] * fa.shape[1]))
    return np.array(terms), float(sum(terms))


def test_restatement_matches_a_naive_derivation():
    w = LP.seeded_weights(7)
    lr, hr = R.make_pair(1, 31, 33, seed=3)
    ref = R.lpips_u8(lr, hr, w)
    terms, score = naive_lpips(R.scaled_from_u8(lr)[0], R.scaled_from_u8(hr)[0], w)
    assert ref["taps"][0].shape == (2, 1, 7, 7, 64) and ref["taps"][4].shape == (2, 1, 1, 1, 256)
    assert np.abs(ref["terms"][0] - terms).max() <= 1e-12 * score and abs(ref["score"][0] - score) <= 1e-12 * score
    assert score > 0 and (terms > 0).all()
    # an all-zero pixel normalises to zeros
    z = np.zeros((1, 2, 2, 8))
    assert np.array_equal(R.distance(z, z + 0.0, np.ones(8)), [0.0])


# ---------------------------------------------------------------------------------------------------- the fp32 input table
def test_input_table_bit_for_bit():
    tab = LP.input_table()
    assert tab.shape == (3, 256) and tab.dtype == np.float32
    bgr = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2)            # [256, 1, 3]: every value in every channel
    x = torch.from_numpy(np.ascontiguousarray(2 * (bgr[..., ::-1] / 255.0) - 1)).float()   # the notebook's to_tensor, before the transpose
    y = (x - torch.tensor(LP.SHIFT, dtype=torch.float32)) / torch.tensor(LP.SCALE, dtype=torch.float32)
    assert y.dtype == torch.float32
    assert tab.T.tobytes() == y.numpy()[:, 0, :].tobytes()
    # the library builds the same table in C
    lib_tab = np.zeros((3, 256), np.float32)
    assert _lib.load().sr_lpips_input_table(lib_tab.ctypes.data_as(C.POINTER(C.c_float))) == _lib.SR_OK
    assert lib_tab.tobytes() == tab.tobytes()
    assert _lib.load().sr_lpips_input_table(None) == _lib.SR_ERR_INVALID
    # and the restatement's uint8 entry reads it with BGR -> RGB
    img = np.array([[[[10, 20, 30]]]], np.uint8)
    assert np.array_equal(R.scaled_from_u8(img)[0, 0, 0], [tab[0][30], tab[1][20], tab[2][10]])


# ---------------------------------------------------------------------------------------------------- the conv1 identity
def regroup_conv1(k):
    """[11,11,3,O] -> [3,3,48,O]: zero-extended to 12 x 12, channel (dy 4 + dx) 3 + c of block (by, bx) = pixel (4 by + dy, 4 bx + dx)."""
    k12 = np.zeros((12, 12) + k.shape[2:], k.dtype)
    k12[:11, :11] = k
    return k12.reshape(3, 4, 3, 4, 3, k.shape[3]).transpose(0, 2, 1, 3, 4, 5).reshape(3, 3, 48, k.shape[3])


def block_image(x, oh, ow):
    """Scaled image [H,W,3] -> shifted by 2 pixels into a zero canvas of (oh + 2) 4 x (ow + 2) 4, space-to-depth(4): [oh + 2, ow + 2, 48]."""
    H, W = x.shape[:2]
    canvas = np.zeros(((oh + 2) * 4, (ow + 2) * 4, 3), x.dtype)
    hh, ww = min(H, canvas.shape[0] - 2), min(W, canvas.shape[1] - 2)
    canvas[2:2 + hh, 2:2 + ww] = x[:hh, :ww]
    return canvas.reshape(oh + 2, 4, ow + 2, 4, 3).transpose(0, 2, 1, 3, 4).reshape(oh + 2, ow + 2, 48)


@pytest.mark.parametrize("H,W", [(31, 31), (35, 47), (64, 50)])
def test_conv1_identity_fp64(H, W):
    rng = np.random.default_rng(H)
    x = rng.standard_normal((H, W, 3))
    k = rng.standard_normal((11, 11, 3, 64))
    nchw = lambda a: torch.from_numpy(np.ascontiguousarray(np.transpose(a, (2, 0, 1))))[None]
    oihw = lambda a: torch.from_numpy(np.ascontiguousarray(np.transpose(a, (3, 2, 0, 1))))
    want = F.conv2d(nchw(x), oihw(k), stride=4, padding=2)[0].permute(1, 2, 0).numpy()
    oh, ow = LP.tap_shapes(H, W)[0]
    assert want.shape == (oh, ow, 64)
    same = F.conv2d(nchw(block_image(x, oh, ow)), oihw(regroup_conv1(k)), padding=1)[0].permute(1, 2, 0).numpy()
    assert same.shape == (oh + 2, ow + 2, 64)
    got = same[1:1 + oh, 1:1 + ow]
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


# ---------------------------------------------------------------------------------------------------- the loader
@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    d = tmp_path_factory.mktemp("lpips_ckpt")
    w = LP.seeded_weights(21)
    alex, lins = LP.to_state_dicts(w)
    pa, pl, pz = str(d / "alexnet.pth"), str(d / "alex.pth"), str(d / "both.npz")
    torch.save({**{k: torch.from_numpy(v) for k, v in alex.items()}, "classifier.1.weight": torch.zeros(2, 2)}, pa)
    torch.save({k: torch.from_numpy(v) for k, v in lins.items()}, pl)
    np.savez(pz, **alex, **lins)
    return {"w": w, "alex": alex, "lins": lins, "pa": pa, "pl": pl, "pz": pz, "dir": d}


def test_loader_reads_both_forms(checkpoints):
    c = checkpoints
    a, b = LP.load_weights(alexnet=c["pa"], lpips=c["pl"]), LP.load_weights(c["pz"])
    for got in (a, b, LP.load_weights(lpips=c["pz"])):
        for k in ("conv_w", "conv_b", "lin_w"):
            for i in range(5):
                assert got[k][i].dtype == np.float32 and got[k][i].flags["C_CONTIGUOUS"]
                assert np.array_equal(got[k][i], c["w"][k][i]), (k, i)
    # one asymmetric kernel value by index: OIHW [o, i, ky, kx] lands at HWIO [ky, kx, i, o]
    assert a["conv_w"][0].shape == (11, 11, 3, 64) and a["conv_w"][0][2, 7, 1, 5] == c["alex"]["features.0.weight"][5, 1, 2, 7]
    assert a["conv_w"][1][4, 0, 63, 191] == c["alex"]["features.3.weight"][191, 63, 4, 0]
    assert a["lin_w"][3].shape == (256,) and a["lin_w"][3][17] == c["lins"]["lin3.model.1.weight"][0, 17, 0, 0]
    assert LP.check_weights(a)["conv_w"][4].shape == (3, 3, 256, 256)


def test_loader_errors(checkpoints):
    c = checkpoints
    with pytest.raises(FileNotFoundError):
        LP.load_weights(alexnet=str(c["dir"] / "nowhere.pth"), lpips=c["pl"])
    with pytest.raises(FileNotFoundError):
        LP.load_weights(str(c["dir"] / "nowhere.npz"))
    with pytest.raises(ValueError):
        LP.load_weights()
    lins = dict(c["lins"])
    del lins["lin3.model.1.weight"]
    p = str(c["dir"] / "missing.pth")
    torch.save({k: torch.from_numpy(v) for k, v in lins.items()}, p)
    with pytest.raises(ValueError, match=r"lin3\.model\.1\.weight"):
        LP.load_weights(alexnet=c["pa"], lpips=p)
    with pytest.raises(ValueError, match=r"lin0\.model\.1\.weight"):
        LP.load_weights(alexnet=c["pa"])                      # the LPIPS checkpoint not given at all
    alex = dict(c["alex"])
    alex["features.0.weight"] = np.zeros((64, 3, 11, 10), np.float32)
    p = str(c["dir"] / "shape.npz")
    np.savez(p, **alex, **c["lins"])
    with pytest.raises(ValueError, match=r"features\.0\.weight"):
        LP.load_weights(p)
    with pytest.raises(ValueError):
        LP.check_weights({"conv_w": c["w"]["conv_w"]})
    with pytest.raises(ValueError):
        LP.check_weights({**c["w"], "lin_w": c["w"]["lin_w"][:4]})


def test_seeded_weights():
    a, b = LP.seeded_weights(7), LP.seeded_weights(7)
    assert all(np.array_equal(x, y) for k in a for x, y in zip(a[k], b[k]))
    assert not np.array_equal(a["conv_w"][0], LP.seeded_weights(8)["conv_w"][0])
    for i, s in enumerate(LP.CONV_SHAPES):
        assert a["conv_w"][i].shape == s and a["conv_b"][i].shape == (s[3],) and a["lin_w"][i].shape == (s[3],)
        assert abs(float(a["conv_w"][i].std()) / math.sqrt(2.0 / (s[0] * s[1] * s[2])) - 1) < 0.05
        assert np.abs(a["conv_b"][i]).max() <= 0.05 and (a["lin_w"][i] >= 0).all()


# ---------------------------------------------------------------------------------------------------- the EDA's host side
def test_lpips_scenarios():
    from data.eda_methods import StatsReporter as S
    df = {"filename": np.array(["a", "b", "c", "d", "e"], dtype=object), "lpips": np.array([0.3, math.nan, 0.1, 0.3, 0.1])}
    assert S.lpips_scenarios(df) == (["c"], ["b"])                       # NaN sorts last, as pandas' sort_values puts it
    assert S.lpips_scenarios(df, top_k=2) == (["c", "e"], ["d", "b"])    # ties keep row order
    assert S.lpips_scenarios(df, top_k=4) == (["c", "e", "a", "d"], ["e", "a", "d", "b"])
    assert S.lpips_scenarios(df, top_k=9) == (["c", "e", "a", "d", "b"],) * 2
    assert S.lpips_scenarios(df, top_k=0) == ([], [])
    with pytest.raises(ValueError):
        S.lpips_scenarios({"filename": df["filename"], "lpips": np.full(5, math.nan)})
    with pytest.raises(ValueError):
        S.lpips_scenarios({"filename": np.array([], dtype=object), "lpips": np.array([])})


def test_unloaded_behaviour():
    from data.eda_methods import ImageDatasetAnalyzer as A
    assert A._lpips_ctx is None                                          # nothing loads it implicitly
    img = np.zeros((40, 40, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="LPIPS"):
        A.lpips_score(img, img)
    with pytest.raises(NotImplementedError, match="LPIPS"):
        A.loss_fn()
    A.unload_lpips()                                                     # unloading what is not loaded does nothing
    assert A._lpips_ctx is None


def test_lpips_calls_without_a_context_are_refused():
    lib = _lib.load()
    assert lib.sr_lpips_set_weights(None, None, None, None) == _lib.SR_ERR_INVALID
    assert lib.sr_lpips(None, None, None, _lib.DTYPE_U8, 1, 64, 64, None, None, None, None) == _lib.SR_ERR_INVALID
