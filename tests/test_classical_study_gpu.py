"""The classical study's device loop: sr_ssim_map, sr_rgb2gray_u8 and sr_freq_to_u8 per element against the fp64 restatements of
tests/classical_study_ref.py and tests/metrics_ref.py, and sr355.study.classical_study against the per-image route through the drop-ins
(the body of test_classic_metrics_gpu.py::test_notebook_loop), bit for bit."""
import math

import numpy as np
import pytest
import torch

import classical_study_ref as SR
import metrics_ref as MR

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (9, 13), (33, 40), (64, 64)]       # window = image; odd and below a tile; one pixel past a tile edge; several whole tiles
RANGES = (255.0, 200.0, 100.0)
U8_TOL, FLOAT_TOL = 1e-9, 1e-6                        # the bars test_classic_metrics_gpu.py holds the ssim column to


def pairs(H, W, C_, seed):
    """B = 3 uint8 pairs [3,H,W] (C_ = 1) or [3,H,W,3]: uniformly random, a block where the two agree, a flat corner."""
    out = []
    for i in range(3):
        ch = [SR.u8_pair(H, W, seed + 10 * i + c) for c in range(C_)]
        out.append((np.stack([p[0] for p in ch], -1), np.stack([p[1] for p in ch], -1)) if C_ == 3 else ch[0])
    return np.stack([p[0] for p in out]), np.stack([p[1] for p in out])


def assert_map(got, ref, tol, what):
    """Per element, separately on the interior and on the four border strips (a wrong border rule moves only the strips)."""
    d = np.abs(got - ref)
    regions = {"interior": d[3:-3, 3:-3], "top": d[:3], "bottom": d[-3:], "left": d[:, :3], "right": d[:, -3:]}
    for name, r in regions.items():
        if r.size:
            assert r.max() <= tol, (what, name, float(r.max()))


@pytest.mark.parametrize("C_", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_ssim_map_matches_restatement(ctx, H, W, C_):
    a, b = pairs(H, W, C_, seed=H * 31 + W + C_)
    da, db = ctx.to_device(a), ctx.to_device(b)
    smap, mean = ctx.ssim_map(da, db, np.array(RANGES))
    assert smap.is_cuda and smap.dtype == torch.float64 and tuple(smap.shape) == a.shape and tuple(mean.shape) == (3,)
    smap_h, mean_h = smap.cpu().numpy(), mean.cpu().numpy()
    col = ctx.classic_scores(da, db, np.array(RANGES)).cpu().numpy()[:, MR.NAMES.index("ssim")]
    for i in range(3):
        S, m = SR.ssim_full(a[i], b[i], RANGES[i])
        assert_map(smap_h[i], S, U8_TOL, ("u8", i))
        assert abs(mean_h[i] - m) <= U8_TOL and abs(mean_h[i] - col[i]) <= 1e-9
        one_map, one_mean = ctx.ssim_map(da[i:i + 1].contiguous(), db[i:i + 1].contiguous(), RANGES[i])      # a batch is its single-image calls
        assert one_map.cpu().numpy().tobytes() == smap_h[i:i + 1].tobytes() and one_mean.cpu().numpy().tobytes() == mean_h[i:i + 1].tobytes()
    again = ctx.ssim_map(da, db, np.array(RANGES))
    assert again[0].cpu().numpy().tobytes() == smap_h.tobytes() and again[1].cpu().numpy().tobytes() == mean_h.tobytes()
    # a float32 pair at range 1
    af, bf = a.astype(np.float32) / np.float32(255), b.astype(np.float32) / np.float32(255)
    fmap, fmean = ctx.ssim_map(ctx.to_device(af), ctx.to_device(bf), 1.0)
    fcol = ctx.classic_scores(ctx.to_device(af), ctx.to_device(bf), 1.0).cpu().numpy()[:, MR.NAMES.index("ssim")]
    for i in range(3):
        S, m = SR.ssim_full(af[i], bf[i], 1.0)
        assert_map(fmap[i].cpu().numpy(), S, FLOAT_TOL, ("f32", i))
        assert abs(float(fmean[i]) - m) <= FLOAT_TOL and abs(float(fmean[i]) - fcol[i]) <= 1e-9
    # the notebook's mixed pair: uint8 HR against a [0, 1] float SR at range 255
    mmap, mmean = ctx.ssim_map(da, ctx.to_device(bf), 255.0)
    mcol = ctx.classic_scores(da, ctx.to_device(bf), 255.0).cpu().numpy()[:, MR.NAMES.index("ssim")]
    for i in range(3):
        S, m = SR.ssim_full(a[i], bf[i], 255.0)
        assert_map(mmap[i].cpu().numpy(), S, FLOAT_TOL, ("u8/f32", i))
        assert abs(float(mmean[i]) - m) <= FLOAT_TOL and abs(float(mmean[i]) - mcol[i]) <= 1e-9
    # float(uint8) goes through the float kernel with exact window sums: the same bits as the integer kernel
    pmap, pmean = ctx.ssim_map(da, ctx.to_device(b.astype(np.float32)), np.array(RANGES))
    assert pmap.cpu().numpy().tobytes() == smap_h.tobytes() and pmean.cpu().numpy().tobytes() == mean_h.tobytes()


def test_ssim_map_refusals_write_nothing(ctx):
    z = ctx.to_device(np.zeros((1, 6, 9), np.uint8))
    with pytest.raises(ValueError, match="7 x 7"):
        ctx.ssim_map(z, z)
    out = torch.full((1, 6, 9), -7.0, dtype=torch.float64, device=ctx.torch_device)
    mean = torch.full((1,), -7.0, dtype=torch.float64, device=ctx.torch_device)
    dr = ctx.to_device(np.array([255.0]))
    call = lambda H, W, C_, dt: ctx.lib.sr_ssim_map(ctx.h, z.data_ptr(), dt, z.data_ptr(), dt, 1, H, W, C_, dr.data_ptr(), out.data_ptr(), mean.data_ptr(),
                                                    ctx.stream())
    from sr355 import _lib as L
    assert call(6, 9, 1, L.DTYPE_U8) == L.SR_ERR_INVALID and b"at least 7" in ctx.lib.sr_last_error(ctx.h)
    assert call(9, 6, 1, L.DTYPE_U8) == L.SR_ERR_INVALID
    assert call(9, 9, 2, L.DTYPE_U8) == L.SR_ERR_INVALID and b"C must be" in ctx.lib.sr_last_error(ctx.h)
    assert call(9, 9, 1, L.DTYPE_BF16) == L.SR_ERR_INVALID
    assert ctx.lib.sr_ssim_map(ctx.h, z.data_ptr(), L.DTYPE_U8, None, L.DTYPE_U8, 1, 9, 9, 1, dr.data_ptr(), out.data_ptr(), mean.data_ptr(), ctx.stream()) < 0
    assert ctx.lib.sr_rgb2gray_u8(ctx.h, z.data_ptr(), 0, 4, 4, out.data_ptr(), ctx.stream()) == L.SR_ERR_INVALID
    assert ctx.lib.sr_freq_to_u8(ctx.h, out.data_ptr(), 1, 0, 4, z.data_ptr(), mean.data_ptr(), ctx.stream()) == L.SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((mean == -7.0).all()) and not bool(z.any())
    with pytest.raises(ValueError):
        ctx.ssim_map(z.to(torch.float32), z)                                     # fine dtypes, still below the window
    with pytest.raises(ValueError):
        ctx.ssim_map(ctx.to_device(np.zeros((1, 8, 8), np.uint8)), ctx.to_device(np.zeros((1, 8, 9), np.uint8)))


def test_structural_similarity_full(ctx):
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    a, b = pairs(33, 40, 3, seed=77)
    m, S = P.structural_similarity(a[0], b[0], data_range=255, channel_axis=2, full=True)
    ref_S, ref_m = SR.ssim_full(a[0], b[0], 255.0)
    assert isinstance(m, float) and S.dtype == np.float64 and S.shape == (33, 40, 3)
    assert np.max(np.abs(S - ref_S)) <= U8_TOL and abs(m - ref_m) <= U8_TOL
    assert m == P.structural_similarity(a[0], b[0], data_range=255, channel_axis=2)
    m2, S2 = P.structural_similarity(a[1, ..., 0], b[1, ..., 0].astype(np.float64) / 255.0, data_range=255, full=True)
    ref_S2, ref_m2 = SR.ssim_full(a[1, ..., 0], (b[1, ..., 0].astype(np.float64) / 255.0).astype(np.float32), 255.0)
    assert S2.shape == (33, 40) and np.max(np.abs(S2 - ref_S2)) <= FLOAT_TOL and abs(m2 - ref_m2) <= FLOAT_TOL


@pytest.mark.parametrize("H,W", [(257, 33), (16, 64)])
def test_rgb2gray_is_bit_exact(ctx, H, W):
    rng = np.random.default_rng(H + W)
    x = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8)
    x[0, 0, :8] = corners
    x[1, -1, -8:] = corners[::-1]
    y = ctx.rgb2gray(ctx.to_device(x))
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.uint8 and tuple(y.shape) == (2, H, W)
    assert np.array_equal(y.cpu().numpy(), MR.rgb2gray_u8(x))
    assert y.cpu().numpy()[0, 0, :8].tolist() == [0, 29, 150, 179, 76, 105, 226, 255]
    # a dense tensor that starts at an odd byte: the byte path
    flat = ctx.to_device(np.concatenate([np.zeros(1, np.uint8), x[0, :H - 1, :W - 1].reshape(-1)]))
    odd = flat[1:].view(1, H - 1, W - 1, 3)
    assert odd.data_ptr() % 4 == 1 and odd.is_contiguous()
    assert np.array_equal(ctx.rgb2gray(odd).cpu().numpy()[0], MR.rgb2gray_u8(x[0, :H - 1, :W - 1]))
    with pytest.raises(ValueError):
        ctx.rgb2gray(ctx.to_device(x[..., 0]))
    with pytest.raises(ValueError):
        ctx.rgb2gray(ctx.to_device(x.astype(np.float32)))


@pytest.mark.parametrize("H,W", [(1, 1), (15, 17), (16, 16), (1, 257), (96, 96)])      # 1, 255, 256, 257 and 9216 elements
def test_freq_to_u8_is_numpys_expression(ctx, H, W):
    rng = np.random.default_rng(H * W)
    f = np.abs(rng.normal(0, 300.0, (5, H, W)))                  # fp64, as sr_freq_extrapolate returns it
    f[1] = 0.0                                                   # an all-zero image in the middle: truncated as it is
    f[3] = 0.3                                                   # every element is the maximum: 255
    f[4] *= 1e-3                                                 # a maximum below 1
    f[0].reshape(-1)[-1] = f[0].max() * 2.0                      # the maximum in the last element
    y, mx = ctx.freq_to_u8(ctx.to_device(f))
    assert y.is_cuda and y.dtype == torch.uint8 and tuple(y.shape) == (5, H, W) and mx.dtype == torch.float64
    y_h, mx_h = y.cpu().numpy(), mx.cpu().numpy()
    for i in range(5):
        ref, m = SR.freq_to_u8(f[i])
        assert mx_h[i] == m and np.array_equal(y_h[i], ref), i
    assert not y_h[1].any() and (y_h[3] == 255).all()
    one = ctx.freq_to_u8(ctx.to_device(f[2:3]))
    assert np.array_equal(one[0].cpu().numpy(), y_h[2:3]) and one[1].cpu().numpy()[0] == mx_h[2]
    with pytest.raises(ValueError):
        ctx.freq_to_u8(ctx.to_device(f.astype(np.float32)))


def test_freq_to_u8_on_the_extrapolation(ctx):
    rng = np.random.default_rng(4)
    lr = rng.integers(0, 256, (2, 24, 33)).astype(np.uint8)
    f = ctx.freq_extrapolate(ctx.to_device(lr), 50, 70)
    y, mx = ctx.freq_to_u8(f)
    f_h = f.cpu().numpy()
    for i in range(2):
        ref, m = SR.freq_to_u8(f_h[i])
        assert np.array_equal(y[i].cpu().numpy(), ref) and float(mx[i]) == m


def test_non_local_means_check_false_returns_the_flags(ctx):
    rng = np.random.default_rng(6)
    lr = rng.integers(0, 256, (3, 24, 33)).astype(np.uint8)
    x = ctx.to_device(lr)
    up = ctx.non_local_means(x, 50, 70)
    up2, bad = ctx.non_local_means(x, 50, 70, check=False)
    assert up2.cpu().numpy().tobytes() == up.cpu().numpy().tobytes() and bad.is_cuda and bad.dtype == torch.bool and not bool(bad.any())
    lr[1] = 90
    xf = ctx.to_device(lr)
    with pytest.raises(ValueError, match=r"image\(s\) \[1\]"):
        ctx.non_local_means(xf, 50, 70)
    up3, den3, sigma3, bad3 = ctx.non_local_means(xf, 50, 70, raw=True, check=False)
    assert bad3.cpu().tolist() == [False, True, False]
    assert up3[0].cpu().numpy().tobytes() == up[0].cpu().numpy().tobytes() and up3[2].cpu().numpy().tobytes() == up[2].cpu().numpy().tobytes()


# ------------------------------------------------------------------ classical_study against the per-image route
N, HS, WS, hs, ws = 3, 70, 50, 33, 24


def rgb_pairs(n, H, W, h, w, seed, noise=6.0):
    """uint8 RGB pairs from sr355.synth plus noise, as gray_pair of test_classic_gpu.py makes its gray ones."""
    import classic_ref as CR
    from sr355.synth import hr_tile
    rng = np.random.default_rng(seed)
    hrs, lrs = [], []
    for _ in range(n):
        hr = np.clip(hr_tile(rng, H, W).astype(np.float64) * 255.0 + rng.normal(0, noise, (H, W, 3)), 0, 255).astype(np.uint8)
        lr = np.clip(np.asarray(CR.O.cv_resize(hr.astype(np.float32), h, w, CR.O.INTER_AREA)) + rng.normal(0, noise, (h, w, 3)), 0, 255).astype(np.uint8)
        hrs.append(hr)
        lrs.append(lr)
    return np.stack(hrs), np.stack(lrs)


@pytest.fixture(scope="module")
def study(ctx):
    from sr355.study import classical_study
    hr, lr = rgb_pairs(N, HS, WS, hs, ws, seed=21)
    res = classical_study(hr, lr, example_index=2, chunk=2)        # chunks of 2 and 1
    per, outs = SR.per_image_route(hr, lr)
    return hr, lr, res, per, outs


def test_study_scores_equal_the_per_image_route(study):
    hr, lr, res, per, outs = study
    assert list(res["stats"]) == list(SR.STAT_KEYS)
    for k in SR.STAT_KEYS[2:]:
        assert list(res["stats"][k]) == list(SR.ALGORITHMS)
        for a in SR.ALGORITHMS:
            got, ref = res["stats"][k][a], np.array(per[k][a], np.float64)
            assert got.dtype == np.float64 and got.shape == (N,)
            assert np.array_equal(got, ref, equal_nan=True), (k, a, got.tolist(), ref.tolist())
    for a in ("ibp", "nlm", "egi", "freq"):
        assert np.isnan(res["stats"]["kl_color"][a]).all()
    for a in ("bilinear", "bicubic", "area", "lanczos"):
        assert np.isfinite(res["stats"]["kl_color"][a]).all()
    assert np.array_equal(res["freq_max"], np.array([o["freq_max"] for o in outs]))
    # and the route's own numbers are the restatement's (one pair, one RGB and one gray algorithm)
    ref = MR.scores(hr[1], outs[1]["bicubic"])
    assert res["stats"]["mae"]["bicubic"][1] == pytest.approx(ref[MR.NAMES.index("mae")], rel=1e-12)
    ref = MR.scores(outs[1]["hr_g"], outs[1]["freq"])
    assert res["stats"]["ssim"]["freq"][1] == pytest.approx(ref[MR.NAMES.index("ssim")], abs=1e-9)


def test_study_examples_equal_the_per_image_route(study):
    hr, lr, res, per, outs = study
    o = outs[2]
    ex = res["examples"]
    assert list(ex) == ["vis", "ibp_example", "nlm_example", "egi_example", "freq_example"]
    want = {"vis": (hr[2], lr[2], o["bilinear"], o["bicubic"], o["area"], o["lanczos"]), "ibp_example": (o["hr_g"], o["lr_g"], o["ibp"]),
            "nlm_example": (o["hr_g"], o["nlm"]), "egi_example": (o["hr_g"], o["lr_g"], o["egi"]), "freq_example": (o["hr_g"], o["freq"])}
    for k, imgs in want.items():
        assert len(ex[k]) == len(imgs)
        for got, ref in zip(ex[k], imgs):
            assert isinstance(got, np.ndarray) and got.dtype == ref.dtype and got.shape == ref.shape and np.array_equal(got, ref), k
    assert ex["nlm_example"][1].dtype == np.float64 and ex["freq_example"][1].dtype == np.uint8


def test_study_time_memory_and_summary(study):
    from test_classic_metrics_gpu import REFERENCE_SUMMARY_KEYS
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    _, _, res, _, _ = study
    for a in SR.ALGORITHMS:
        t, m = res["stats"]["time"][a], res["stats"]["memory"][a]
        assert t.shape == (N,) and np.isfinite(t).all() and (t > 0).all()
        assert m.shape == (N,) and np.isfinite(m).all() and (m >= 0).all()
        assert t[0] == t[1] and m[0] == m[1]                        # per-chunk averages, repeated for the chunk's images
        assert m[0] >= HS * WS                                      # at least the algorithm's own output, one byte per pixel
    summary = res["summary"]
    assert list(summary) == list(SR.ALGORITHMS) and all(set(v) == REFERENCE_SUMMARY_KEYS for v in summary.values())
    assert summary["nlm"]["psnr_mean"] == pytest.approx(float(np.mean(res["stats"]["psnr"]["nlm"])))
    assert all(math.isfinite(summary[a]["psnr_ci_low"]) for a in SR.ALGORITHMS)
    ranked, scores, _ = P.rank_algorithms(summary)
    assert sorted(a for a, _ in ranked) == sorted(SR.ALGORITHMS) and all(0.0 <= s <= 1.0 for s in scores.values())


def test_study_ssim_maps(study):
    from SRModels.classic_super_resolution_algorithms import visualization_methods as VM
    _, _, res, _, outs = study
    maps = res["ssim_maps"]
    assert list(maps) == ["Bilinear", "Bicubic", "Area", "Lanczos", "IBP", "NLM", "EGI", "FREQ"]
    o = outs[2]
    hr_gray = MR.rgb2gray_u8(res["examples"]["vis"][0])
    assert np.array_equal(hr_gray, o["hr_g"])
    srs = {"Bilinear": MR.rgb2gray_u8(o["bilinear"]), "Bicubic": MR.rgb2gray_u8(o["bicubic"]), "Area": MR.rgb2gray_u8(o["area"]),
           "Lanczos": MR.rgb2gray_u8(o["lanczos"]), "IBP": o["ibp"], "NLM": o["nlm"].astype(np.float32), "EGI": o["egi"], "FREQ": o["freq"]}
    for name, (smap, val) in maps.items():
        assert smap.shape == (HS, WS) and smap.dtype == np.float64 and isinstance(val, float)
        # val is the mean over the cropped map; the two sums run in different orders over (HS - 6)(WS - 6) = 2816 values of magnitude <= 1
        assert abs(val - smap[3:-3, 3:-3].mean()) <= 1e-12, name
        S, m = SR.ssim_full(hr_gray, srs[name], 255.0)              # the reference's rule: range 255, the HR image is uint8 (NLM too)
        tol = FLOAT_TOL if name == "NLM" else U8_TOL
        assert np.max(np.abs(smap - S)) <= tol and abs(val - m) <= tol, name
    # NumPy in gives what the device tensors gave
    ex = res["examples"]
    again = VM.ssim_similarity_maps(ex["vis"], ex["ibp_example"], ex["nlm_example"], ex["egi_example"], ex["freq_example"])
    assert list(again) == list(maps)
    for name in maps:
        assert again[name][0].tobytes() == maps[name][0].tobytes() and again[name][1] == maps[name][1]
    titles = VM.super_resolution_example(ex["vis"], ex["ibp_example"], ex["nlm_example"], ex["egi_example"], ex["freq_example"])
    assert [t for t, _ in titles] == ["HR", "LR"] + list(maps) and titles[7][1] is ex["nlm_example"][1]


def test_study_inputs(ctx, study):
    from sr355.study import classical_study
    hr, lr, res, _, _ = study
    # device tensors and lists of frames, one chunk: the same scores (the kernels do not depend on the batch)
    for args in ((ctx.to_device(hr), ctx.to_device(lr)), (list(hr), list(lr))):
        r2 = classical_study(*args, example_index=2)
        for k in SR.STAT_KEYS[2:]:
            for a in SR.ALGORITHMS:
                assert np.array_equal(r2["stats"][k][a], res["stats"][k][a], equal_nan=True), (k, a)
        assert np.array_equal(r2["examples"]["nlm_example"][1], res["examples"]["nlm_example"][1])
        assert r2["ssim_maps"]["NLM"][0].tobytes() == res["ssim_maps"]["NLM"][0].tobytes()
    flat = lr.copy()
    flat[1] = 90                                                    # an LR image without detail: NL-means' noise estimate has nothing to stand on
    with pytest.raises(ValueError, match=r"non_local_means: the noise estimate of image\(s\) \[1\]"):
        classical_study(hr, flat, chunk=2)
    with pytest.raises(NotImplementedError, match="float"):
        classical_study(hr.astype(np.float32) / 255.0, lr)
    with pytest.raises(ValueError, match="same size"):
        classical_study(list(hr), [lr[0], lr[1], lr[2][:, :-1]])
    with pytest.raises(ValueError, match="HR images for"):
        classical_study(hr, lr[:2])
    with pytest.raises(ValueError, match="example_index"):
        classical_study(hr, lr, example_index=3)
