"""The EDA restatement (tests/eda_ref.py) against independent forms that exist without a GPU: scipy.stats, scipy.fft, scipy.ndimage,
np.histogram, plain loops and a hand-made co-occurrence example; and the host side of data/eda_methods.py."""
import math

import numpy as np
import pytest
import scipy.fft
import scipy.ndimage as ndi
import scipy.stats

import eda_ref as R


def image(H, W, seed, smooth=True):
    """uint8 BGR: blocks and ramps with noise, so that edges, flat areas and every channel order occur."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = 110 + 90 * np.sign(np.sin(yy / 3.1) * np.cos(xx / 4.3)) * (rng.random() + 0.5) / 1.5
    img = np.stack([base + rng.normal(0, 12, (H, W)) + c * xx * 0.4 for c in range(3)], -1)
    if not smooth:
        img = rng.integers(0, 256, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


IMAGES = [image(41, 37, 1), image(23, 50, 2, smooth=False), image(7, 7, 3), image(64, 64, 4)]


def test_moments_match_scipy_stats():
    for img in IMAGES:
        for c in range(3):
            x = img[..., c].ravel().astype(np.float64)
            mean, std, skew, kurt = R.moments(img[..., c])
            assert mean == pytest.approx(x.mean(), rel=1e-13) and std == pytest.approx(x.std(), rel=1e-12)
            assert skew == pytest.approx(scipy.stats.skew(x), abs=1e-11) and kurt == pytest.approx(scipy.stats.kurtosis(x), abs=1e-11)
    flat = np.full((9, 8), 77, np.uint8)
    assert R.moments(flat)[:2] == (77.0, 0.0) and math.isnan(R.moments(flat)[2]) and math.isnan(R.moments(flat)[3])
    with np.errstate(all="ignore"):
        assert math.isnan(scipy.stats.skew(flat.ravel().astype(float))) and math.isnan(scipy.stats.kurtosis(flat.ravel().astype(float)))


def test_dct_matches_scipy_fft():
    for img in IMAGES:
        g = R.gray_u8(img)
        ref = scipy.fft.dctn(g.astype(np.float64), norm="ortho")
        assert np.max(np.abs(R.dct2(g) - ref)) <= 1e-10 * np.abs(ref).max()
    g = R.gray_u8(IMAGES[0])
    D = np.abs(scipy.fft.dctn(g.astype(np.float64), norm="ortho"))
    assert R.blocking(g) == pytest.approx((D[7::8].mean() + D[:, 7::8].mean()) / 2, rel=1e-10)
    assert math.isnan(R.blocking(R.gray_u8(IMAGES[2])))             # 7 x 7: D[7::8] is empty, the reference's mean of nothing


def test_stencils_match_scipy_ndimage():
    for img in IMAGES:
        g = R.gray_u8(img)
        gf = g.astype(np.float64)
        assert np.array_equal(R.laplacian(g), ndi.correlate(gf, R.LAP.astype(float), mode="mirror"))
        gx, gy = R.sobel5(g)
        assert np.array_equal(gx, ndi.correlate(gf, R.SOBEL5_X.astype(float), mode="mirror"))
        assert np.array_equal(gy, ndi.correlate(gf, R.SOBEL5_X.T.astype(float), mode="mirror"))
        assert np.array_equal(R.blur3_u8(g), np.floor(ndi.correlate(gf, R.B3 / 16.0, mode="mirror") + 0.5).astype(np.uint8))
        for c in range(3):
            f5 = ndi.correlate(img[..., c].astype(np.float64), R.B5 / 256.0, mode="mirror")
            assert np.array_equal(R.blur5_u8(img)[..., c], np.floor(f5 + 0.5).astype(np.uint8))
        # skimage.filters.sobel: image / 255, (1 2 1) x (1 0 -1) / 4, scipy 'reflect', sqrt((h^2 + v^2) / 2)
        s = gf / 255.0
        h = ndi.correlate(s, np.outer([1, 0, -1], [1, 2, 1]) / 4.0, mode="reflect")
        v = ndi.correlate(s, np.outer([1, 2, 1], [1, 0, -1]) / 4.0, mode="reflect")
        assert R.sobel_mean(g) == pytest.approx(np.sqrt((h * h + v * v) / 2).mean(), rel=1e-12)
        # Canny's Sobel pair: replicated borders are scipy's 'nearest'
        lab = R.canny_labels(g)
        gx3 = ndi.correlate(gf, R.SOBEL3_X.astype(float), mode="nearest")
        gy3 = ndi.correlate(gf, R.SOBEL3_X.T.astype(float), mode="nearest")
        m = np.abs(gx3) + np.abs(gy3)
        assert not (lab[m <= 100] != 0).any() and not (lab[m <= 200] == 2).any()
        assert not lab[0].any() and not lab[-1].any() and not lab[:, 0].any() and not lab[:, -1].any()


def test_gray_and_fft():
    img = IMAGES[0]
    g = R.gray_u8(img)
    f = 0.114 * img[..., 0] + 0.587 * img[..., 1] + 0.299 * img[..., 2]
    assert np.max(np.abs(g - f)) <= 0.51
    assert np.array_equal(R.gray_u8(np.repeat(g[..., None], 3, 2)), g)            # the coefficients sum to 2^14
    H, W = g.shape
    F = R.fft_mag(g)
    assert F[H // 2, W // 2] == pytest.approx(g.sum(), rel=1e-12)                  # DC at the centre after fftshift


def test_glcm_counts_match_a_double_loop():
    g = R.gray_u8(IMAGES[0])
    for levels in (64, 256):
        q = R.quantise(g, levels)
        assert q.max() < levels
        got = R.glcm_counts(q, levels)
        for n, (dr, dc) in enumerate(R.ANGLE_OFFSETS):
            ref = np.zeros((levels, levels), np.int64)
            for r in range(q.shape[0]):
                for c in range(q.shape[1]):
                    if 0 <= r + dr < q.shape[0] and 0 <= c + dc < q.shape[1]:
                        ref[q[r, c], q[r + dr, c + dc]] += 1
            assert np.array_equal(got[n], ref)
    assert [(round(math.sin(a)), round(math.cos(a))) for a in (0, math.pi / 4, math.pi / 2, 3 * math.pi / 4)] == list(R.ANGLE_OFFSETS)
    assert not R.quantise(np.zeros((8, 8), np.uint8), 256).any()
    # float32 truncation: 255 levels of 256 are not the identity
    assert R.quantise(np.arange(256, dtype=np.uint8), 256).tolist() == [int(np.float32(np.float32(v) / np.float32(255.0)) * np.float32(255)) for v in range(256)]


def test_glcm_properties_on_a_hand_made_example():
    """The 4-level image of the scikit-image documentation's kind, angle 0:
         0 0 1 1 / 0 0 1 1 / 0 2 2 2 / 2 2 3 3   -> horizontal pairs (0,0) x2, (0,1) x2, (1,1) x2, (0,2) x1, (2,2) x3, (2,3) x1, (3,3) x1.
       Symmetrised counts S = C + C^T, total 24:  S00 = 4, S01 = S10 = 2, S11 = 4, S02 = S20 = 1, S22 = 6, S23 = S32 = 1, S33 = 2.
       contrast     = (2 + 2) 1 / 24 + (1 + 1) 4 / 24 + (1 + 1) 1 / 24 = 14 / 24
       homogeneity  = (4 + 4 + 6 + 2) / 24 + (4 + 2) / 2 / 24 + 2 / 5 / 24 = (16 + 3 + 0.4) / 24
       marginals p = (7, 6, 8, 3) / 24: mean = (6 + 16 + 9) / 24 = 31 / 24, E[i^2] = (6 + 32 + 27) / 24 = 65 / 24,
       var = 65 / 24 - (31 / 24)^2 = 599 / 576;  E[ij] = (4 + 24 + 2 * 6 + 18) / 24 = 58 / 24;  cov = 58 / 24 - 961 / 576 = 431 / 576
       correlation  = 431 / 599."""
    q = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 2, 2, 2], [2, 2, 3, 3]], np.uint8)
    C = R.glcm_counts(q, 4, (0,))[0]
    assert C.tolist() == [[2, 2, 1, 0], [0, 2, 0, 0], [0, 0, 3, 1], [0, 0, 0, 1]]
    P = R.glcm_normed(C)
    assert P.sum() == pytest.approx(1.0) and np.array_equal(P, P.T)
    con, hom, cor = R.glcm_props(P)
    assert con == pytest.approx(14 / 24, rel=1e-14) and hom == pytest.approx(19.4 / 24, rel=1e-14) and cor == pytest.approx(431 / 599, rel=1e-13)
    flat = R.glcm_normed(R.glcm_counts(np.full((5, 5), 2, np.uint8), 4, (0,))[0])
    assert R.glcm_props(flat) == (0.0, 1.0, 1.0)


def test_hysteresis_matches_connected_components_and_dilation_matches_scipy():
    eight = np.ones((3, 3), bool)
    found = 0
    for img in IMAGES:
        lab = R.canny_labels(R.gray_u8(img))
        comp, n = ndi.label(lab > 0, structure=eight)
        keep = np.zeros(n + 1, bool)
        keep[np.unique(comp[lab == 2])] = True
        keep[0] = False
        ref = keep[comp]
        edges = R.hysteresis(lab)
        assert np.array_equal(edges, ref)
        found += int(((lab == 1) & edges).any()) + int(((lab == 1) & ~edges).any())
        assert np.array_equal(R.dilate5(edges), ndi.binary_dilation(edges, structure=np.ones((5, 5), bool)))
        e8 = R.canny_u8(R.gray_u8(img))
        region = ndi.binary_dilation(e8 > 0, structure=np.ones((5, 5), bool)) & ~(e8 > 0)
        want = float(np.std(R.gray_u8(img)[region])) if region.any() else 0.0
        assert R.ringing(R.gray_u8(img), e8) == pytest.approx(want, rel=1e-12)
    assert found >= 2           # both outcomes of a weak survivor occur in these images
    # a hand-made chain: strong - weak - weak, and a weak pixel alone
    lab = np.zeros((7, 9), np.uint8)
    lab[2, 2], lab[3, 3], lab[4, 4], lab[2, 6] = 2, 1, 1, 1
    e = R.hysteresis(lab)
    assert e[2, 2] and e[3, 3] and e[4, 4] and not e[2, 6] and e.sum() == 3
    assert R.ringing(np.full((7, 9), 9, np.uint8), np.zeros((7, 9), np.uint8)) == 0.0


def test_saturation_and_value_against_the_float_formula():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    img[:8] = img[:8, :, :1]                                   # gray pixels: S = 0
    img[8:10] = 0
    s, v = R.hsv_sv(img)
    x = img.astype(np.float64)
    vmax, vmin = x.max(-1), x.min(-1)
    assert np.array_equal(v, vmax.astype(np.uint8))
    with np.errstate(all="ignore"):
        sf = np.where(vmax > 0, 255.0 * (vmax - vmin) / np.where(vmax > 0, vmax, 1), 0.0)
    assert np.max(np.abs(s.astype(np.float64) - sf)) <= 1.0
    exact = sf == np.round(sf)
    assert exact.sum() > 100 and np.array_equal(s[exact], sf[exact].astype(np.uint8))
    # every (V, V - min) pair
    V, D = np.meshgrid(np.arange(1, 256), np.arange(0, 256), indexing="ij")
    ok = D <= V
    allp = np.stack([V[ok], V[ok] - D[ok], V[ok]], -1)[None].astype(np.uint8)
    s_all = R.hsv_sv(allp)[0][0].astype(np.float64)
    assert np.max(np.abs(s_all - 255.0 * D[ok] / V[ok])) <= 1.0


def test_saturation_histogram_matches_np_histogram():
    assert np.array_equal(R.SAT_BINS, np.linspace(0, 256, 51))
    allv = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.sat_counts(allv), np.histogram(allv, bins=R.SAT_BINS)[0])
    for v in range(256):
        assert np.array_equal(R.sat_counts(np.array([v], np.uint8)), np.histogram([v], bins=R.SAT_BINS)[0]), v
    s = R.hsv_sv(IMAGES[1])[0]
    assert np.array_equal(R.sat_counts(s), np.histogram(s, bins=R.SAT_BINS)[0])


def test_accumulate_and_row_shapes():
    lrs, hrs = [image(16, 18, 10 + i) for i in range(2)], [image(16, 18, 20 + i) for i in range(2)]
    acc = R.accumulate(lrs, hrs)
    assert acc["glcm_sum"].sum() == pytest.approx(2.0) and acc["sat_counts"].sum() == 4 * 16 * 18
    assert acc["grad_hr_sum"].shape == (16, 18) and acc["lr_fft_sum"][8, 9] == pytest.approx(sum(float(R.gray_u8(x).sum()) for x in lrs))
    row, raw = R.pair_stats(lrs[0], hrs[0], 64, (0, 1, 2, 3))
    assert row.shape == (46,) and len(R.ROW_COLUMNS) == 32 and raw["glcm"].shape == (4, 64, 64) and raw["dct"].shape == (2, 16, 18)


# ------------------------------------------------------------------ the Python surface without a GPU
def test_module_imports_and_host_helpers_run_without_a_gpu(tmp_path):
    from data import eda_methods as E
    from sr355 import _lib
    assert _lib.EDA_STAT_NAMES == R.STAT_NAMES and _lib.EDA_ROW_COLUMNS == R.ROW_COLUMNS
    assert E.ImagePairMetrics.FIELDS[2:] == R.ROW_COLUMNS and E.ImagePairMetrics.FIELDS[:2] == ("filename", "lpips")
    with pytest.raises(NotImplementedError, match="LPIPS"):
        E.ImageDatasetAnalyzer.lpips_score(IMAGES[0], IMAGES[0])
    from PIL import Image
    for base in ("lr", "hr"):
        (tmp_path / base / "a").mkdir(parents=True)
    Image.fromarray(IMAGES[0][..., ::-1]).save(tmp_path / "lr" / "a" / "x.png")
    Image.fromarray(IMAGES[0][..., ::-1]).save(tmp_path / "hr" / "a" / "x.png")
    Image.fromarray(IMAGES[0]).save(tmp_path / "hr" / "only_hr.png")
    assert list(E.ImagePairLoader.iter_pairs(str(tmp_path / "lr"), str(tmp_path / "hr"))) == [("a/x.png", "a/x.png")]
    assert np.array_equal(E.ImagePairLoader.read_bgr(str(tmp_path / "lr" / "a" / "x.png")), IMAGES[0])
    with pytest.raises(ValueError):
        list(E.ImagePairLoader.iter_pairs(str(tmp_path / "lr" / "a"), str(tmp_path / "hr")))
    assert E.ImagePairLoader.interpolation_for("x.png", {"x.png": "INTER_CUBIC"}) == "INTER_CUBIC"
    assert E.ImagePairLoader.interpolation_for("x.png", {"y.png": "INTER_CUBIC"}) == "INTER_LINEAR" == E.ImagePairLoader.interpolation_for("x.png")
    with pytest.raises(NotImplementedError, match="INTER_LINEAR_EXACT"):
        E.ImagePairLoader.interpolation_for("x.png", {"x.png": "INTER_LINEAR_EXACT"})
    row = E.ImagePairMetrics("f.png", *range(21))
    assert row.as_dict()["edge_diff"] == 20 and row.ch2_kurt_hr is None and list(row.as_dict()) == list(E.ImagePairMetrics.FIELDS)
    g = E.MetricsAggregator.new_global_data()
    assert g["count"] == 0 and g["sat_lr_counts"].shape == (50,) and np.array_equal(g["sat_bins"], np.linspace(0, 256, 51))


def test_stats_reporter_summary_follows_describe():
    from data import eda_methods as E
    rng = np.random.default_rng(6)
    rows = [E.ImagePairMetrics(f"{i}.png", math.nan, *rng.normal(30, 4, 20), ch0_skew_lr=(math.nan if i == 3 else float(i))) for i in range(11)]
    df = E.StatsReporter.dataframe(rows)
    assert list(df) == list(E.ImagePairMetrics.FIELDS) and df["filename"][2] == "2.png" and df["psnr"].shape == (11,)
    assert np.isnan(df["ch1_skew_lr"]).all()
    s = E.StatsReporter.summary(df)
    assert "filename" not in s and set(s["psnr"]) == {"mean", "std", "25%", "50%", "75%"}
    for k in ("psnr", "edge_diff", "ch0_skew_lr"):
        a = df[k][~np.isnan(df[k])]
        q = np.percentile(a, [25, 50, 75])
        assert s[k]["mean"] == pytest.approx(a.mean(), rel=1e-13) and s[k]["std"] == pytest.approx(np.std(a, ddof=1), rel=1e-12)
        assert [s[k]["25%"], s[k]["50%"], s[k]["75%"]] == pytest.approx(list(q), rel=1e-13)
    assert len(df["ch0_skew_lr"][~np.isnan(df["ch0_skew_lr"])]) == 10
    assert all(math.isnan(v) for v in s["lpips"].values())


def test_abi_lists_the_new_symbols():
    from sr355 import _lib
    import test_abi_cpu
    assert {"sr_eda_pair_stats", "sr_eda_accumulate"} <= set(test_abi_cpu.header_symbols()) and test_abi_cpu.header_symbols() == sorted(_lib.SIGNATURES)
