"""The dataset-synthesis stages without a device: the NumPy restatement (tests/degrade_ref.py, the device's contract) against a real
baseline-JPEG codec -- the committed golden file and, where Pillow is installed, Pillow itself, bit for bit -- the quantisation tables,
the Gaussian taps, the draw order of data.common_methods.draw_degradation against a hand-written replay of the reference's calls, and
Philox4x32-10 (two restatements and Random123's known-answer vectors)."""
import os

import numpy as np
import pytest

import degrade_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degrade_jpeg.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def golden_cases(g):
    return [(int(H), int(W), int(q)) for H, W in g["sizes"] for q in g["qualities"]]


def test_golden_file_covers_the_cases_the_contract_names(golden):
    assert {tuple(s) for s in golden["sizes"].tolist()} == {(16, 16), (17, 23), (23, 17), (40, 24), (33, 16)}
    assert golden["qualities"].tolist() == [20, 49, 50, 59]
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert "libjpeg" in str(golden["versions"][1])


def test_restatement_equals_the_codec_on_the_golden_cases(golden):
    for H, W, q in golden_cases(golden):
        got = R.jpeg_roundtrip(golden[f"in_{H}x{W}"], q)
        ref = golden[f"out_{H}x{W}_q{q}"]
        d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
        print(f"{H}x{W} q{q}: max level difference {d.max()}, differing share {(d > 0).mean():.4f}")
        assert np.array_equal(got, ref), (H, W, q)


def test_golden_images_exercise_range_limiting_and_zeroed_coefficients(golden):
    """What the images were built for: some decoded block leaves 0..255 before the clamp, and most high coefficients quantise to zero."""
    img = golden["in_40x24"]
    _, raw = R.jpeg_roundtrip(img, 20, raw=True)
    assert (raw["y"] == 255).any() and (raw["y"] == 0).any()
    assert (raw["coef_y"] == 0).mean() > 0.5 and (raw["coef_y"] != 0).sum() > 15


def test_restatement_equals_pillow_live(golden):
    pytest.importorskip("PIL")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_degrade_golden", os.path.join(os.path.dirname(GOLDEN), "make_degrade_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    for n, (H, W) in enumerate(mk.SIZES):
        img = mk.make_image(H, W, 100 + n)
        assert np.array_equal(img, golden[f"in_{H}x{W}"])
        for q in mk.QUALITIES:
            dec, _ = mk.pillow_roundtrip(img, q)
            assert np.array_equal(R.jpeg_roundtrip(img, q), dec), (H, W, q)
    rng = np.random.default_rng(5)                    # one frame-sized image more, at qualities the draw can give and at the scale's ends
    img = rng.integers(0, 256, (61, 47, 3), dtype=np.uint8)
    img[20:40, 10:30] = np.linspace(0, 255, 20, dtype=np.uint8)[None, :, None]
    for q in (1, 33, 100):
        dec, _ = mk.pillow_roundtrip(img, q)
        assert np.array_equal(R.jpeg_roundtrip(img, q), dec), q


def test_quant_tables_golden(golden):
    for q in golden["qualities"]:
        lum, chrom = R.quant_tables(int(q))
        assert np.array_equal(golden[f"qt_q{q}"], np.stack([lum.reshape(-1), chrom.reshape(-1)]))


def test_quant_tables_against_pillow():
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    for q in (1, 20, 49, 50, 59, 100):
        buf = io.BytesIO()
        Image.new("RGB", (16, 16)).save(buf, format="JPEG", quality=q, subsampling=2)
        buf.seek(0)
        with Image.open(buf) as im:
            tables = im.quantization
        lum, chrom = R.quant_tables(q)
        assert list(tables[0]) == lum.reshape(-1).tolist() and list(tables[1]) == chrom.reshape(-1).tolist(), q
    assert R.quant_tables(1)[0].max() == 255 and R.quant_tables(100)[0].tolist() == [[1] * 8] * 8          # baseline clamp; 200 - 2 q = 0


@pytest.mark.parametrize("ksize", [3, 5, 7])
@pytest.mark.parametrize("sigma", [0.8, 2.0])
def test_gauss_taps(ksize, sigma):
    from sr355.runtime import gauss_taps
    t = gauss_taps(ksize, sigma)
    assert t.dtype == np.int32 and len(t) == ksize and int(t.sum()) == 256
    assert np.array_equal(t, t[::-1]) and (t >= 0).all() and t[ksize // 2] == t.max()
    assert np.array_equal(t, R.gauss_taps(ksize, sigma))
    g = np.exp(-((np.arange(ksize) - ksize // 2) ** 2) / (2 * sigma ** 2))
    assert np.abs(t / 256.0 - g / g.sum()).max() <= 1.5 / 256            # half a step of rounding, one more on the centre tap at most


def test_gauss_taps_reject_what_the_kernel_does_not_take():
    from sr355.runtime import gauss_taps
    for k, s in ((4, 1.0), (9, 1.0), (3, 0.0), (3, -1.0)):
        with pytest.raises(ValueError):
            gauss_taps(k, s)


def replay_reference(seed, shape, scale):
    """The reference's degrade_image, its np.random calls only, on a RandomState of its own (data/common_methods.py:58-105)."""
    rs = np.random.RandomState(seed)
    out = {"gauss": None, "motion": None, "noise": None, "jpeg": None}
    if rs.rand() < 0.7:
        ksize = rs.choice([3, 5, 7])
        sigma = rs.uniform(0.8, 2.0)
        out["gauss"] = (ksize, sigma)
    if rs.rand() < 0.3:
        out["motion"] = rs.choice([5, 7, 9])
    out["interp"] = rs.choice([1, 2, 3, 4])
    h, w = shape[:2]
    out["size"] = (int(w * scale), int(h * scale))
    lr_shape = (out["size"][1], out["size"][0], 3)
    if rs.rand() < 0.7:
        noise_std = rs.uniform(2, 10)
        out["noise"] = (noise_std, rs.normal(0, noise_std, lr_shape).astype(np.float32))
    if rs.rand() < 0.7:
        out["jpeg"] = rs.randint(20, 60)
    return out


DRAW_SEEDS = tuple(range(20))


def test_draw_order_is_the_references():
    from data import common_methods as M
    seen = set()
    shape, scale = (34, 50, 3), 0.5
    for seed in DRAW_SEEDS:
        ref = replay_reference(seed, shape, scale)
        rec = M.draw_degradation(shape, scale, np.random.RandomState(seed))
        np.random.seed(seed)
        rec_global = M.draw_degradation(shape, scale)                    # the global state, as degrade_image draws
        for r in (rec, rec_global):
            assert (r["gauss_ksize"], r["gauss_sigma"]) == ((0, None) if ref["gauss"] is None else (int(ref["gauss"][0]), float(ref["gauss"][1])))
            assert r["motion_size"] == (0 if ref["motion"] is None else int(ref["motion"]))
            assert r["interp_code"] == int(ref["interp"]) and r["interp_name"] == R.INTERP_NAMES[R.INTERP_CODES.index(int(ref["interp"]))]
            assert r["lr_size"] == ref["size"] == (25, 17)
            if ref["noise"] is None:
                assert r["noise_std"] is None and r["noise"] is None
            else:
                assert r["noise_std"] == float(ref["noise"][0])
                assert r["noise"].dtype == np.float32 and r["noise"].shape == (17, 25, 3) and np.array_equal(r["noise"], ref["noise"][1])
            assert r["jpeg_quality"] == (0 if ref["jpeg"] is None else int(ref["jpeg"]))
        seen |= {("gauss", rec["gauss_ksize"]), ("motion", rec["motion_size"]), ("interp", rec["interp_code"]), ("noise", rec["noise_std"] is not None),
                 ("jpeg", rec["jpeg_quality"] > 0)}
    want = {("gauss", k) for k in (0, 3, 5, 7)} | {("motion", 0)} | {("interp", c) for c in (1, 2, 3, 4)} | {("noise", True), ("noise", False), ("jpeg", True), ("jpeg", False)}
    assert want <= seen, want - seen
    assert any(k == "motion" and v in (5, 7, 9) for k, v in seen)


def test_philox_restatements_agree_and_match_random123():
    # Random123's kat_vectors, philox4x32 with 10 rounds: counter, key -> output
    kat = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for ctr, key, out in kat:
        assert R.philox4x32_10_scalar(ctr, key) == out
        assert tuple(int(v) for v in R.philox4x32_10(np.array([ctr], np.uint32), np.array([key], np.uint32))[0]) == out
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, (64, 4), dtype=np.uint64).astype(np.uint32)
    key = rng.integers(0, 2 ** 32, (64, 2), dtype=np.uint64).astype(np.uint32)
    vec = R.philox4x32_10(ctr, key)
    for i in range(64):
        assert tuple(int(v) for v in vec[i]) == R.philox4x32_10_scalar(ctr[i], key[i])
    seed = 0x0123456789ABCDEF                          # the stream's layout: counter (e // 4, 0, image, 0), key (low, high), word e % 4
    w = R.philox_words(seed, 3, 10)
    assert tuple(int(v) for v in w[4:8]) == R.philox4x32_10_scalar((1, 0, 3, 0), (0x89ABCDEF, 0x01234567))


def test_philox_normal_is_standard_normal_and_bounded():
    z = R.philox_normal(7, 0, (64, 64, 3))
    assert z.shape == (64, 64, 3) and abs(z.mean()) < 0.05 and abs(z.std() - 1.0) < 0.05
    assert np.abs(z).max() <= np.sqrt(2 * 24 * np.log(2.0)) + 1e-12          # u1 >= 2^-24: |z| <= 5.77
    assert not np.array_equal(z, R.philox_normal(7, 1, (64, 64, 3)))


def test_blur_restatements_on_cases_with_known_answers():
    flat = np.full((16, 17, 3), 77, np.uint8)
    for k in (3, 5, 7):
        assert np.array_equal(R.gaussian_blur(flat, R.gauss_taps(k, 1.3)), flat)
    for size in (5, 7, 9):
        assert np.array_equal(R.motion_blur(flat, size), flat)
    x = np.zeros((16, 16, 3), np.uint8)
    x[:, 8] = 255
    m = R.motion_blur(x, 5)                            # 255 / 5 = 51 exactly over the five columns that see the line
    assert (m[:, 6:11] == 51).all() and (m[:, :6] == 0).all() and (m[:, 11:] == 0).all()
    rng = np.random.default_rng(2)                     # the integer form equals float accumulation rounded half to even
    y = rng.integers(0, 256, (16, 40, 3), dtype=np.uint8)
    for size in (5, 7, 9):
        r = size // 2
        cols = R.reflect101(np.arange(40)[:, None] + np.arange(-r, r + 1)[None, :], 40)
        acc = np.zeros((16, 40, 3), np.float32)
        for j in range(size):
            acc += y[:, cols[:, j]].astype(np.float32) * np.float32(1.0 / size)
        assert np.array_equal(np.rint(acc).astype(np.uint8), R.motion_blur(y, size))


def test_noise_restatement_truncates_after_the_clip():
    x = np.array([[[0, 0, 254]], [[255, 10, 10]]], np.uint8)
    f = np.array([[[-0.5, 0.0, 0.999]], [[0.5, 0.7, -0.7]]], np.float32)
    assert R.noise_apply(x, f).tolist() == [[[0, 0, 254]], [[255, 10, 9]]]


def test_common_methods_imports_without_a_device_and_crop_raises():
    from data import common_methods as M
    with pytest.raises(NotImplementedError, match="contour"):
        M.smart_square_crop(np.zeros((32, 32, 3), np.uint8))
    assert M.lr_size((478, 478, 3), 0.5) == (239, 239)
    with pytest.raises(NotImplementedError):
        M.degrade_image(np.zeros((32, 32, 3), np.float32))
    with pytest.raises(ValueError):
        M.degrade_image(np.zeros((15, 32, 3), np.uint8))
