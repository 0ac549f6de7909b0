"""The dataset EDA's per-pair statistics and global accumulators on the device (sr_eda_pair_stats, sr_eda_accumulate, Context.eda_*,
data/eda_methods.py) against the NumPy restatement of tests/eda_ref.py, on synthetic 3D-print tiles from sr355.synth.

Bounds (the issue's): integer raw outputs are equal; statistics that are fixed-order fp64 functions of integers within rel 1e-12;
those through a DCT / DFT operator or a float stencil within rel 1e-9 (the accumulated spectra and gradient sums element by element);
differences that may sit near zero get the absolute form (skew / kurtosis 1e-12 max(1, |ref|), edge_diff 1e-9 of the larger mean,
glcm_correlation 1e-12).  The raw DCT plane is compared within 1e-9 of its largest coefficient (a choice of this file: the issue sets
no bound for it; blocking_* is the element-sensitive check of the transform)."""
import math

import numpy as np
import pytest
import torch

import eda_ref as R

pytestmark = pytest.mark.gpu

NAMES = R.STAT_NAMES
IDX = {k: i for i, k in enumerate(NAMES)}
REL12 = tuple(f"{k}_{s}" for k in ("rms_noise", "lap_var", "color_noise", "ringing", "saturation_mean", "brightness_mean") for s in ("lr", "hr")) \
    + ("glcm_contrast", "glcm_homogeneity") + tuple(f"ch{c}_{k}_{s}" for k in ("mean", "std") for c in range(3) for s in ("lr", "hr"))
REL9 = ("blocking_lr", "blocking_hr", "sobel_mean_lr", "sobel_mean_hr")
ALL_ANGLES = (0, 1, 2, 3)


def hr_image(H, W, seed, stretch=False):
    """uint8 BGR print-like tile (stretched to the full range for the 7 x 7 minimum, where a tile is otherwise nearly flat)."""
    from sr355.synth import hr_tile
    rng = np.random.default_rng(seed)
    t = hr_tile(rng, H, W).astype(np.float64)
    if stretch:
        t = (t - t.min()) / max(t.max() - t.min(), 1e-9)
    return rng, np.ascontiguousarray((t * 255).astype(np.uint8)[..., ::-1])


def make_pair(ctx, H, W, seed, stretch=False):
    """HR and a degraded LR: 2 x 2 box mean of the even crop, device bicubic back up, seeded noise."""
    from sr355.synth import box_down
    rng, hr = hr_image(H, W, seed, stretch)
    small = np.round(box_down(hr[:H // 2 * 2, :W // 2 * 2].astype(np.float32), 2)).astype(np.uint8)
    up = ctx.resize(ctx.to_device(small[None]), H, W, "INTER_CUBIC")[0].cpu().numpy().astype(np.float64)
    lr = np.clip(up + rng.normal(0, 4, up.shape), 0, 255).astype(np.uint8)
    return lr, hr


def assert_row(got, ref, skip=("psnr", "ssim"), dct_floor=0.0):
    for k in NAMES:
        if k in skip:
            continue
        g, r = float(got[IDX[k]]), float(ref[IDX[k]])
        print(f"{k}: device {g!r} reference {r!r}")
        if math.isnan(r):
            assert math.isnan(g), (k, g, r)
        elif k in REL12:
            assert abs(g - r) <= 1e-12 * abs(r), (k, g, r)
        elif k in REL9:
            assert abs(g - r) <= max(1e-9 * abs(r), dct_floor if k.startswith("blocking") else 0.0), (k, g, r)
        elif k == "glcm_correlation":
            assert abs(g - r) <= 1e-12, (k, g, r)
        elif k == "edge_diff":
            assert abs(g - r) <= 1e-9 * max(ref[IDX["sobel_mean_lr"]], ref[IDX["sobel_mean_hr"]]), (k, g, r)
        else:
            assert "_skew_" in k or "_kurt_" in k, k
            assert abs(g - r) <= 1e-12 * max(1.0, abs(r)), (k, g, r)


def assert_raw(raw, ref, b=0):
    for k in ("gray", "sat", "val", "blur3", "blur5", "edges"):
        assert np.array_equal(raw[k][b].cpu().numpy(), ref[k]), k
    assert np.array_equal(raw["glcm"][b].cpu().numpy(), ref["glcm"]), "glcm"
    d = raw["dct"][b].cpu().numpy()
    assert np.max(np.abs(d - ref["dct"])) <= 1e-9 * np.abs(ref["dct"]).max()


@pytest.fixture(scope="module")
def big(ctx):
    """Five 478 x 478 pairs (the dataset's size) on the device, and the reference of pair 0, computed once."""
    pairs = [make_pair(ctx, 478, 478, seed) for seed in (1, 2, 3, 4, 5)]
    lr, hr = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    row256, raw256 = R.pair_stats(lr[0], hr[0], 256, ALL_ANGLES)
    return {"lr": lr, "hr": hr, "dlr": ctx.to_device(lr), "dhr": ctx.to_device(hr), "row256": row256, "raw256": raw256}


def textured(img):
    """On the reference alone: Canny finds edges and the ringing region is not empty."""
    e = R.canny_u8(R.gray_u8(img)) > 0
    return bool(e.any()) and bool((R.dilate5(e) & ~e).any())


def test_478_pair_matches_restatement(ctx, big):
    assert textured(big["lr"][0]) and textured(big["hr"][0])
    lab = R.canny_labels(R.gray_u8(big["lr"][0]))
    assert ((lab == 1) & R.hysteresis(lab)).any()                     # hysteresis promotes weak survivors in this image
    got, raw = ctx.eda_pair_stats(big["dlr"][:1].contiguous(), big["dhr"][:1].contiguous(), 256, ALL_ANGLES, raw=True)
    assert_raw(raw, big["raw256"])
    assert_row(got[0].cpu().numpy(), big["row256"])
    # 64 levels, four angles and one
    q = R.quantise(big["raw256"]["gray"][0], 64)
    got64, raw64 = ctx.eda_pair_stats(big["dlr"][:1].contiguous(), big["dhr"][:1].contiguous(), 64, ALL_ANGLES, raw=True)
    assert np.array_equal(raw64["glcm"][0].cpu().numpy(), R.glcm_counts(q, 64, ALL_ANGLES))
    ref = R.glcm_features(big["raw256"]["gray"][0], 64, ALL_ANGLES)
    g = got64[0].cpu().numpy()
    assert abs(g[2] - ref[0]) <= 1e-12 * ref[0] and abs(g[3] - ref[1]) <= 1e-12 * ref[1] and abs(g[4] - ref[2]) <= 1e-12
    assert np.array_equal(np.delete(g, [2, 3, 4]), np.delete(got[0].cpu().numpy(), [2, 3, 4]), equal_nan=True)
    got1, raw1 = ctx.eda_pair_stats(big["dlr"][:1].contiguous(), big["dhr"][:1].contiguous(), 64, (2,), raw=True)
    assert np.array_equal(raw1["glcm"][0].cpu().numpy(), R.glcm_counts(q, 64, (2,)))
    ref = R.glcm_features(big["raw256"]["gray"][0], 64, (2,))
    g = got1[0].cpu().numpy()
    assert abs(g[2] - ref[0]) <= 1e-12 * ref[0] and abs(g[3] - ref[1]) <= 1e-12 * ref[1] and abs(g[4] - ref[2]) <= 1e-12


@pytest.mark.parametrize("H,W,seed,stretch", [(61, 45, 4, False), (7, 7, 4, True)])
def test_small_pairs_match_restatement(ctx, H, W, seed, stretch):
    lr, hr = make_pair(ctx, H, W, seed, stretch)
    assert textured(lr) and textured(hr)
    for levels in (256, 64):
        got, raw = ctx.eda_pair_stats(ctx.to_device(lr[None]), ctx.to_device(hr[None]), levels, ALL_ANGLES, raw=True)
        row, ref = R.pair_stats(lr, hr, levels, ALL_ANGLES)
        assert_raw(raw, ref)
        assert_row(got[0].cpu().numpy(), row)
    if H < 8:
        assert math.isnan(row[IDX["blocking_lr"]])            # D[7::8] is empty below 8 rows: the reference's mean of nothing


@pytest.mark.parametrize("value", [0, 93])
def test_constant_images(ctx, value):
    """The other branch of every rule: no edges (ringing 0.0), constant channels (skew / kurtosis NaN), one co-occurrence cell
    (correlation 1), the all-zero quantisation."""
    img = np.full((40, 52, 3), value, np.uint8)
    assert not textured(img)
    for levels in (256, 64):
        got, raw = ctx.eda_pair_stats(ctx.to_device(img[None]), ctx.to_device(img[None]), levels, ALL_ANGLES, raw=True)
        row, ref = R.pair_stats(img, img, levels, ALL_ANGLES)
        assert_raw(raw, ref)
        g = got[0].cpu().numpy()
        # blocking of a constant image is exactly 0; each side returns the rounding residue of its own DCT, which no relative bound can
        # hold.  Set as the project's rule for such a column: the reference's own spread on this input, fp64 restatement against its
        # longdouble form, is 6.93e-15 (restatement 6.927e-15, longdouble 2.8e-18; scipy.fft.dctn gives 0.0) for value 93 and 0 for
        # value 0; the bound is ten times that, 6.93e-14, absolute.
        assert_row(g, row, dct_floor=10 * 6.93e-15 if value else 0.0)
        assert g[IDX["ringing_lr"]] == 0.0 and g[IDX["glcm_correlation"]] == 1.0 and math.isnan(g[IDX["ch1_skew_hr"]]) and math.isnan(g[IDX["ch2_kurt_lr"]])
        assert g[IDX["glcm_contrast"]] == 0.0 and g[IDX["glcm_homogeneity"]] == 1.0 and g[IDX["psnr"]] == math.inf and g[IDX["ssim"]] == 1.0
        if value == 0:
            assert not raw["glcm"][0, :, 1:, :].any() and not raw["glcm"][0, :, :, 1:].any()


def test_psnr_ssim_are_classic_scores_columns(ctx, big):
    got = ctx.eda_pair_stats(big["dlr"], big["dhr"], 64, (0,)).cpu().numpy()
    swap = lambda t: t.flip(-1).contiguous()
    cs = ctx.classic_scores(swap(big["dhr"]), swap(big["dlr"]), 255.0).cpu().numpy()
    assert got[:, 0].tobytes() == cs[:, 0].tobytes() and got[:, 1].tobytes() == cs[:, 1].tobytes()
    assert np.all(np.isfinite(got[:, :2]))


def test_rows_do_not_depend_on_the_batch_or_the_run(ctx, big):
    full = ctx.eda_pair_stats(big["dlr"], big["dhr"], 256, ALL_ANGLES).cpu().numpy()
    again = ctx.eda_pair_stats(big["dlr"], big["dhr"], 256, ALL_ANGLES).cpu().numpy()
    assert full.tobytes() == again.tobytes()
    for i in (0, 3):
        one = ctx.eda_pair_stats(big["dlr"][i:i + 1].contiguous(), big["dhr"][i:i + 1].contiguous(), 256, ALL_ANGLES).cpu().numpy()
        assert one.tobytes() == full[i:i + 1].tobytes(), i
    assert_row(full[0], big["row256"])


def test_accumulators_match_restatement(ctx, big):
    n = 3
    acc = ctx.eda_accumulate(big["dlr"][:n].contiguous(), big["dhr"][:n].contiguous())
    ref = R.accumulate(big["lr"][:n], big["hr"][:n])
    assert np.array_equal(acc["sat_counts"].cpu().numpy(), ref["sat_counts"])
    for k in ("lr_fft_sum", "hr_fft_sum"):
        d = np.abs(acc[k].cpu().numpy() - ref[k])
        print(k, "max abs", d.max(), "of", ref[k].max(), "smallest bin", ref[k].min(), "max element-wise rel", (d / ref[k]).max())
        assert np.all(d <= 1e-9 * ref[k]), (k, (d / ref[k]).max())
    g = acc["grad_hr_sum"].cpu().numpy()
    assert np.all(np.abs(g - ref["grad_hr_sum"]) <= 1e-9 * ref["grad_hr_sum"])
    s = acc["glcm_sum"].cpu().numpy()
    assert np.all(np.abs(s - ref["glcm_sum"]) <= 1e-12 * ref["glcm_sum"]) and s.sum() == pytest.approx(n, rel=1e-12)
    # one call on three pairs equals three calls
    step = None
    for i in range(n):
        step = ctx.eda_accumulate(big["dlr"][i:i + 1].contiguous(), big["dhr"][i:i + 1].contiguous(), step)
    for k in acc:
        assert torch.equal(acc[k], step[k]), k


def test_python_surface(ctx, big, tmp_path):
    from data import eda_methods as E
    rows, g = E.MetricsAggregator.collect_arrays(big["lr"], big["hr"], glcm_multi_angle=True, glcm_levels=256)
    abi = ctx.eda_pair_stats(big["dlr"], big["dhr"], 256, ALL_ANGLES).cpu().numpy()
    assert len(rows) == 5
    for i, r in enumerate(rows):
        d = r.as_dict()
        assert list(d) == list(E.ImagePairMetrics.FIELDS) and len(d) == 34 and math.isnan(d["lpips"]) and d["filename"] == str(i)
        assert np.array([d[k] for k in R.ROW_COLUMNS]).tobytes() == abi[i, :32].tobytes()
    assert g["count"] == 5 and g["glcm_sum"].shape == (256, 256, 1, 1) and g["sat_lr_counts"].shape == (50,) and g["sat_hr_counts"].dtype == np.float64
    assert g["lr_fft_sum"].shape == g["hr_fft_sum"].shape == g["grad_hr_sum"].shape == (478, 478) and len(g["sat_bins"]) == 51
    assert g["noise_means_lr"] == [r.color_noise_lr for r in rows] and g["sat_lr_counts"].sum() == 5 * 478 * 478
    assert set(g) == {"count", "lr_fft_sum", "hr_fft_sum", "grad_hr_sum", "glcm_sum", "sat_lr_counts", "sat_hr_counts", "sat_bins", "noise_means_lr"}
    s = E.StatsReporter.summary(E.StatsReporter.dataframe(rows))
    assert s["psnr"]["mean"] == pytest.approx(abi[:, 0].mean(), rel=1e-13)

    # collect on written PNG pairs: two LR sizes (one already aligned, one half size with a mapped interpolation)
    from PIL import Image
    hrs = [hr_image(48, 40, 30 + i)[1] for i in range(4)]
    lrs = [make_pair(ctx, 48, 40, 30 + i)[0] for i in range(2)] + [np.ascontiguousarray(h[::2, ::2]) for h in hrs[2:]]
    names = ["a/p0.png", "a/p1.png", "b/p2.png", "b/p3.png"]
    for nm, l, h in zip(names, lrs, hrs):
        for base, im in (("lr", l), ("hr", h)):
            (tmp_path / base / nm).parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(im[..., ::-1]).save(tmp_path / base / nm)
    imap = {"p2.png": "INTER_CUBIC"}                                   # p3: the default, INTER_LINEAR
    rows_d, g_d = E.MetricsAggregator.collect(str(tmp_path / "lr"), str(tmp_path / "hr"), glcm_levels=64, interp_map=imap)
    up = lambda x, m: ctx.resize(ctx.to_device(x[None]), 48, 40, m)[0].cpu().numpy()
    aligned = np.stack(lrs[:2] + [up(lrs[2], "INTER_CUBIC"), up(lrs[3], "INTER_LINEAR")])
    rows_a, g_a = E.MetricsAggregator.collect_arrays(aligned, np.stack(hrs), glcm_levels=64, filenames=names)
    assert [r.filename for r in rows_d] == names
    for a, b in zip(rows_d, rows_a):
        da, db = a.as_dict(), b.as_dict()
        assert all(da[k] == db[k] or (math.isnan(da[k]) and math.isnan(db[k])) for k in R.ROW_COLUMNS) and da["filename"] == db["filename"]
    assert g_d["count"] == 4 and np.array_equal(g_d["sat_hr_counts"], g_a["sat_hr_counts"]) and np.array_equal(g_d["sat_lr_counts"], g_a["sat_lr_counts"])
    for k in ("lr_fft_sum", "hr_fft_sum", "grad_hr_sum", "glcm_sum"):
        assert np.array_equal(g_d[k], g_a[k]), k          # collect's batches visit the pairs in the same order: the same sums, bit for bit
    l0, h0 = E.ImagePairLoader.load_and_align(str(tmp_path / "lr" / names[2]), str(tmp_path / "hr" / names[2]), imap)
    assert np.array_equal(l0, aligned[2]) and np.array_equal(h0, hrs[2])
    with pytest.raises(NotImplementedError, match="INTER_NEAREST_EXACT"):
        E.MetricsAggregator.collect(str(tmp_path / "lr"), str(tmp_path / "hr"), interp_map={"p3.png": "INTER_NEAREST_EXACT"})

    # the single-image methods
    A = E.ImageDatasetAnalyzer
    lr, hr = aligned[0], hrs[0]
    row, raw = R.pair_stats(lr, hr, 64, (0,))
    gray, hsv = A.color_planes(lr)
    assert np.array_equal(gray, raw["gray"][0]) and np.array_equal(hsv[..., 1], raw["sat"][0]) and np.array_equal(hsv[..., 2], raw["val"][0])
    assert A.rms_noise(gray) == pytest.approx(row[IDX["rms_noise_lr"]], rel=1e-12) and isinstance(A.rms_noise(gray), float)
    assert A.laplacian_variance(gray) == pytest.approx(row[IDX["lap_var_lr"]], rel=1e-12)
    f = A.glcm_features(gray)
    assert f["glcm_contrast"] == pytest.approx(row[IDX["glcm_contrast"]], rel=1e-12) and set(f) == {"glcm_contrast", "glcm_homogeneity", "glcm_correlation"}
    f4 = A.glcm_features(gray, levels=256, multi_angle=True)
    assert f4["glcm_homogeneity"] == pytest.approx(R.glcm_features(gray, 256, ALL_ANGLES)[1], rel=1e-12)
    assert A.glcm_features(gray, angles=[np.pi / 2])["glcm_contrast"] == pytest.approx(R.glcm_features(gray, 64, (2,))[0], rel=1e-12)
    fd = A.feature_distribution(lr, hsv)
    assert len(fd) == 14 and fd["ch2_std"] == pytest.approx(row[IDX["ch2_std_lr"]], rel=1e-12) and fd["saturation_mean"] == pytest.approx(row[IDX["saturation_mean_lr"]], rel=1e-12)
    art = A.detect_artifacts(lr, gray)
    assert art["ringing_artifact"] == pytest.approx(row[IDX["ringing_lr"]], rel=1e-12) and art["blocking_score"] == pytest.approx(row[IDX["blocking_lr"]], rel=1e-9)
    assert A.psnr_metric(lr, hr) == rows_a[0].psnr and A.ssim_metric(lr, hr) == rows_a[0].ssim
    with pytest.raises(ValueError, match="hsv"):
        A.feature_distribution(lr, hsv[:, ::-1])
    with pytest.raises(ValueError, match="gray"):
        A.detect_artifacts(lr, 255 - gray)
    with pytest.raises(NotImplementedError):
        A.lpips_score(lr, hr)


def test_refused_shapes_come_back_as_value_errors(ctx):
    z = lambda *s: ctx.to_device(np.zeros(s, np.uint8))
    with pytest.raises(ValueError, match="at least 7"):
        ctx.eda_pair_stats(z(1, 6, 9, 3), z(1, 6, 9, 3))
    with pytest.raises(ValueError, match="at least 7"):
        ctx.eda_accumulate(z(1, 9, 6, 3), z(1, 9, 6, 3))
    with pytest.raises(ValueError, match="2\\^22 pixels"):
        ctx.eda_pair_stats(z(1, 2049, 2049, 3), z(1, 2049, 2049, 3))
    with pytest.raises(ValueError, match="4096"):
        ctx.eda_accumulate(z(1, 7, 4097, 3), z(1, 7, 4097, 3))
    with pytest.raises(ValueError):
        ctx.eda_pair_stats(z(1, 9, 9, 3), z(1, 9, 8, 3))
    with pytest.raises(ValueError):
        ctx.eda_pair_stats(z(1, 9, 9, 3).float(), z(1, 9, 9, 3))
    a, out = z(1, 9, 9, 3), ctx.empty((1, len(NAMES)), torch.float64)
    call = lambda levels, mask: ctx.check(ctx.lib.sr_eda_pair_stats(ctx.h, a.data_ptr(), a.data_ptr(), 1, 9, 9, levels, mask, out.data_ptr(), None, None, None,
                                                                    None, None, None, None, None, ctx.stream()))
    with pytest.raises(ValueError, match="glcm_levels must be 64 or 256"):
        call(128, 1)
    with pytest.raises(ValueError, match="angle_mask"):
        call(64, 0)
    with pytest.raises(ValueError, match="null tensor"):
        ctx.check(ctx.lib.sr_eda_accumulate(ctx.h, a.data_ptr(), a.data_ptr(), 1, 9, 9, None, None, None, None, None, ctx.stream()))
    call(64, 15)
