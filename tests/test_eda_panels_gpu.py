"""The EDA's per-pair panels on the device (sr_eda_pair_panels, Context.eda_pair_panels, data/eda_methods.py's ImageDataVisualization,
run_eda_panels, run_eda_pipeline) against the NumPy restatement of tests/eda_panels_ref.py, on pairs made as test_eda_gpu makes them.

Bounds (the issue's): diff, sat_hist and noise_lr are the restatement's bits; glcm_lr is the bits of counts_sym / T formed in fp64;
noise_mean and glcm_contrast are the bits of sr_eda_pair_stats' columns (256 levels, angle 0); grad_hr within 1e-9 relative, the bound
test_accumulators_match_restatement uses; a spectrum bin within max(1e-9 ref, floor), floor = (H + W) 2^-52 sum(gray): the a-priori
bound of two chained dot products with unit-modulus factors (a bin near zero has no meaningful relative bound).  For one pair the
spectra, the gradient and the matrix equal sr_eda_accumulate's sums from zero bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

import eda_panels_ref as P
import eda_ref as R
from test_eda_gpu import make_pair

pytestmark = pytest.mark.gpu

SHAPES = [(61, 45, 4, False), (64, 48, 5, False), (7, 7, 4, True)]       # both odd (fftshift's (n + 1) / 2), even, the minimum stretched to full range
MAPS = ("spec_lr", "spec_hr", "grad_hr", "glcm_lr", "noise_lr", "diff", "sat_hist", "glcm_contrast", "noise_mean")


@pytest.fixture(scope="module")
def cases(ctx):
    """Per shape: the pair, its device tensors, the restatement and the B = 1 panel outputs, computed once."""
    out = {}
    for H, W, seed, stretch in SHAPES:
        lr, hr = make_pair(ctx, H, W, seed, stretch)
        dlr, dhr = ctx.to_device(lr[None]), ctx.to_device(hr[None])
        out[(H, W)] = {"lr": lr, "hr": hr, "dlr": dlr, "dhr": dhr, "ref": P.pair_panels(lr, hr), "dev": ctx.eda_pair_panels(dlr, dhr)}
    return out


def assert_spectrum(got, ref, gray_sum, who):
    floor = P.spectrum_floor(ref.shape, gray_sum)
    d = np.abs(got - ref)
    need = d > 1e-9 * ref
    print(f"{who}: max abs {d.max():.3e} of {ref.max():.3e}, floor {floor:.3e}, bins that needed the floor {int(need.sum())} of {ref.size}")
    assert np.all(d <= np.maximum(1e-9 * ref, floor)), (who, float(d.max()))


@pytest.mark.parametrize("H,W", [s[:2] for s in SHAPES])
def test_outputs_match_restatement(ctx, cases, H, W):
    c = cases[(H, W)]
    dev, ref = {k: v[0].cpu().numpy() for k, v in c["dev"].items()}, c["ref"]
    assert set(dev) == set(MAPS)
    assert dev["diff"].dtype == np.uint8 and np.array_equal(dev["diff"], ref["diff"])
    assert dev["sat_hist"].dtype == np.int64 and np.array_equal(dev["sat_hist"], ref["sat_hist"]) and dev["sat_hist"].sum() == 2 * H * W
    assert dev["noise_lr"].tobytes() == ref["noise_lr"].tobytes()
    assert ref["glcm_total"] == 2 * H * (W - 1)
    assert dev["glcm_lr"].tobytes() == (ref["glcm_sym_counts"].astype(np.float64) / float(ref["glcm_total"])).tobytes()
    g = np.abs(dev["grad_hr"] - ref["grad_hr"])
    print("grad_hr max rel", float((g / np.maximum(ref["grad_hr"], 1e-300)).max()))
    assert np.all(g <= 1e-9 * ref["grad_hr"])
    for k, s in (("spec_lr", 0), ("spec_hr", 1)):
        assert_spectrum(dev[k], ref[k], ref["gray_sum"][s], f"{k} {H}x{W}")
    # the scalars: the bits of sr_eda_pair_stats' columns, and the restatement's values
    row = ctx.eda_pair_stats(c["dlr"], c["dhr"], 256, (0,))[0].cpu().numpy()
    names = ctx.EDA_STAT_NAMES
    assert dev["glcm_contrast"].tobytes() == row[names.index("glcm_contrast")].tobytes()
    assert dev["noise_mean"].tobytes() == row[names.index("color_noise_lr")].tobytes()
    assert float(dev["noise_mean"]) == ref["noise_mean"]
    assert abs(float(dev["glcm_contrast"]) - ref["glcm_contrast"]) <= 1e-12 * ref["glcm_contrast"]


@pytest.mark.parametrize("H,W", [s[:2] for s in SHAPES])
def test_one_pair_equals_the_accumulators_from_zero(ctx, cases, H, W):
    c = cases[(H, W)]
    acc = ctx.eda_accumulate(c["dlr"], c["dhr"])
    for a, p in (("lr_fft_sum", "spec_lr"), ("hr_fft_sum", "spec_hr"), ("grad_hr_sum", "grad_hr"), ("glcm_sum", "glcm_lr")):
        assert torch.equal(acc[a], c["dev"][p][0]), (a, p)
    hist = c["dev"]["sat_hist"][0].cpu().numpy()
    folded = np.zeros((2, 50), np.int64)
    np.add.at(folded, (np.repeat([0, 1], 256), np.tile(np.arange(256) * 25 // 128, 2)), hist.ravel())
    assert np.array_equal(folded, acc["sat_counts"].cpu().numpy())


def test_outputs_do_not_depend_on_the_batch_or_the_run(ctx, cases):
    H, W = 61, 45
    pairs = [(cases[(H, W)]["lr"], cases[(H, W)]["hr"])] + [make_pair(ctx, H, W, seed) for seed in (11, 12)]
    dlr, dhr = ctx.to_device(np.stack([p[0] for p in pairs])), ctx.to_device(np.stack([p[1] for p in pairs]))
    full, again = ctx.eda_pair_panels(dlr, dhr), ctx.eda_pair_panels(dlr, dhr)
    for k in MAPS:
        assert torch.equal(full[k], again[k]), k
    for i in (0, 2):
        one = cases[(H, W)]["dev"] if i == 0 else ctx.eda_pair_panels(dlr[i:i + 1].contiguous(), dhr[i:i + 1].contiguous())
        for k in MAPS:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    assert not torch.equal(full["spec_hr"][0], full["spec_hr"][2])


def test_a_dft_chunk_boundary_inside_a_pair(ctx):
    """The DFT runs in chunks of images, lr and hr interleaved: a chunk holds EDA_CHUNK_BYTES / (planes per image x 8 bytes x H W) images.
    With csrc/eda.hip's 256 MiB and four fp64 planes per image (X, T's real and imaginary parts, |F|), 500 x 500 gives
    floor(2^28 / (4 * 8 * 250000)) = 33 images: odd, so B = 17 (34 images) needs two chunks and the second begins at image 33, pair 16's
    hr, between that pair's two images.  A change of the workspace layout changes these numbers: redo the arithmetic here."""
    H = W = 500
    per_img = 4 * 8 * H * W
    chunk = (256 << 20) // per_img
    assert chunk == 33 and chunk % 2 == 1 and chunk < 2 * 17 <= 2 * chunk
    a, b, c = (make_pair(ctx, H, W, seed) for seed in (21, 22, 23))
    order = [a] + [b, c] * 8                                            # pair 15 is b, pair 16 is c
    dlr, dhr = ctx.to_device(np.stack([p[0] for p in order])), ctx.to_device(np.stack([p[1] for p in order]))
    which = ("spec_lr", "spec_hr")
    full = ctx.eda_pair_panels(dlr, dhr, which=which)
    for i in (0, 16):
        one = ctx.eda_pair_panels(dlr[i:i + 1].contiguous(), dhr[i:i + 1].contiguous(), which=which)
        for k in which:
            assert torch.equal(one[k][0], full[k][i]), (k, i)
    gl, gh = R.gray_u8(c[0]), R.gray_u8(c[1])
    assert_spectrum(full["spec_lr"][16].cpu().numpy(), R.fft_mag(gl), int(gl.astype(np.int64).sum()), "spec_lr pair 16")
    assert_spectrum(full["spec_hr"][16].cpu().numpy(), R.fft_mag(gh), int(gh.astype(np.int64).sum()), "spec_hr pair 16")


def test_constant_pair(ctx):
    H, W, value = 40, 52, 93
    img = np.full((H, W, 3), value, np.uint8)
    x = ctx.to_device(img[None])
    dev = {k: v[0].cpu().numpy() for k, v in ctx.eda_pair_panels(x, x).items()}
    assert not dev["diff"].any() and not dev["noise_lr"].any() and not dev["grad_hr"].any()
    cell = np.zeros((256, 256))
    cell[value, value] = 1.0
    assert np.array_equal(dev["glcm_lr"], cell) and float(dev["glcm_contrast"]) == 0.0 and float(dev["noise_mean"]) == 0.0
    floor = P.spectrum_floor((H, W), value * H * W)
    for k in ("spec_lr", "spec_hr"):
        above = np.argwhere(dev[k] > floor)
        assert above.tolist() == [[H // 2, W // 2]] and dev[k][H // 2, W // 2] == pytest.approx(value * H * W, rel=1e-12), k
    hist = np.zeros((2, 256), np.int64)
    hist[:, 0] = H * W                                                  # a gray image: S = 0 everywhere
    assert np.array_equal(dev["sat_hist"], hist)
    from data import eda_methods as E
    panel = E.ImageDataVisualization.advanced_panel(img, img)
    ref = np.histogram(np.zeros(H * W, np.uint8), bins=50, density=True)
    for side in ("sat_lr", "sat_hr"):
        assert panel[side][0].tobytes() == ref[0].tobytes() and panel[side][1].tobytes() == ref[1].tobytes()
    assert panel["lr_glcm_contrast"] == 0.0 and panel["color_noise_mean"] == 0.0


def test_which_subsets(ctx, cases):
    c = cases[(61, 45)]
    for which in (("diff",), ("spec_hr",), ("noise_mean",), ("glcm_contrast", "sat_hist"), ("grad_hr", "glcm_lr", "noise_lr", "spec_lr")):
        got = ctx.eda_pair_panels(c["dlr"], c["dhr"], which=which)
        assert set(got) == set(which)
        for k in which:
            assert torch.equal(got[k], c["dev"][k]), (which, k)
    with pytest.raises(ValueError, match="which"):
        ctx.eda_pair_panels(c["dlr"], c["dhr"], which=("spectrum",))
    with pytest.raises(ValueError, match="which"):
        ctx.eda_pair_panels(c["dlr"], c["dhr"], which=())


def test_refused_shapes_come_back_as_value_errors(ctx):
    z = lambda *s: ctx.to_device(np.zeros(s, np.uint8))
    with pytest.raises(ValueError, match="at least 7"):
        ctx.eda_pair_panels(z(1, 6, 9, 3), z(1, 6, 9, 3))
    with pytest.raises(ValueError, match="2\\^22 pixels"):
        ctx.eda_pair_panels(z(1, 2049, 2049, 3), z(1, 2049, 2049, 3), which=("diff",))
    with pytest.raises(ValueError, match="4096"):
        ctx.eda_pair_panels(z(1, 7, 4097, 3), z(1, 7, 4097, 3), which=("diff",))
    with pytest.raises(ValueError):
        ctx.eda_pair_panels(z(1, 9, 9, 3), z(1, 9, 8, 3))
    with pytest.raises(ValueError):
        ctx.eda_pair_panels(z(1, 9, 9, 3).float(), z(1, 9, 9, 3))
    a = z(1, 9, 9, 3)
    with pytest.raises(ValueError, match="null tensor"):
        ctx.check(ctx.lib.sr_eda_pair_panels(ctx.h, a.data_ptr(), None, 1, 9, 9, None, None, None, None, None, None, None, None, ctx.stream()))
    with pytest.raises(ValueError, match="batch"):
        ctx.check(ctx.lib.sr_eda_pair_panels(ctx.h, a.data_ptr(), a.data_ptr(), 0, 9, 9, None, None, None, None, None, None, None, None, ctx.stream()))
    ctx.check(ctx.lib.sr_eda_pair_panels(ctx.h, a.data_ptr(), a.data_ptr(), 1, 9, 9, None, None, None, None, None, None, None, None, ctx.stream()))


def assert_panels_equal(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], tuple):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a[k], b[k])), k
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def test_advanced_panel_and_visual_example(ctx, cases):
    from data import eda_methods as E
    V = E.ImageDataVisualization
    c = cases[(61, 45)]
    dev, ref = {k: v[0].cpu().numpy() for k, v in c["dev"].items()}, P.advanced_panel(c["lr"], c["hr"])
    panel = V.advanced_panel(c["lr"], c["hr"])
    assert set(panel) == set(ref)
    assert panel["lr_log_spectrum"].tobytes() == np.log(dev["spec_lr"] + 1e-8).tobytes()
    assert panel["hr_log_spectrum"].tobytes() == np.log(dev["spec_hr"] + 1e-8).tobytes()
    s_lr, s_hr = c["ref"]["sat_planes"]
    for side, s in (("sat_lr", s_lr), ("sat_hr", s_hr)):
        density, edges = np.histogram(s.ravel(), 50, density=True)
        assert panel[side][0].tobytes() == density.tobytes() and panel[side][1].tobytes() == edges.tobytes(), side
        assert ref[side][0].tobytes() == density.tobytes()
    assert panel["noise_map"].tobytes() == ref["noise_map"].tobytes() and panel["color_noise_mean"] == ref["color_noise_mean"]
    assert panel["lr_glcm"].tobytes() == dev["glcm_lr"].tobytes() and isinstance(panel["lr_glcm_contrast"], float)
    assert panel["gradient_magnitude"].tobytes() == dev["grad_hr"].tobytes()
    vis, vref = V.visual_example(c["lr"], c["hr"]), P.visual_example(c["lr"], c["hr"])
    assert set(vis) == {"lr_rgb", "hr_rgb", "diff_gray"} and all(vis[k].dtype == np.uint8 and np.array_equal(vis[k], vref[k]) for k in vis)
    stack = V.advanced_panels(np.stack([c["lr"], c["hr"]]), np.stack([c["hr"], c["hr"]]))
    first = dict(stack[0])
    assert np.array_equal(first.pop("diff_gray"), vis["diff_gray"]) and not stack[1]["diff_gray"].any()
    assert_panels_equal(first, panel)
    with pytest.raises(ValueError, match="aligned"):
        V.advanced_panel(c["lr"], c["hr"][:-1])


@pytest.fixture(scope="module")
def tree(ctx, tmp_path_factory):
    """Six 48 x 40 PNG pairs in two sub-folders."""
    from PIL import Image
    base = tmp_path_factory.mktemp("eda_tree")
    names = ["a/p0.png", "a/p1.png", "a/p2.png", "b/q0.png", "b/q1.png", "b/q2.png"]
    for i, nm in enumerate(names):
        lr, hr = make_pair(ctx, 48, 40, 40 + i)
        for side, im in (("lr", lr), ("hr", hr)):
            (base / side / nm).parent.mkdir(parents=True, exist_ok=True)
            Image.fromarray(im[..., ::-1]).save(base / side / nm)
    return base, names


def expected_examples(df, names, k):
    order = np.argsort(df["psnr"], kind="stable")
    keys = []
    for label, idx in (("best", order[:k]), ("worst", order[len(names) - k:])):
        for rank, i in enumerate(idx, 1):
            parent, basic, adv = P.example_names(label, rank, names[i])
            keys.append((names[i], f"{label}_scenarios/{parent}/{basic}", f"{label}_scenarios/{parent}/{adv}"))
    return keys


def test_run_eda_panels_ranked_by_psnr(ctx, tree):
    from data import eda_methods as E
    base, names = tree
    df, panels = E.run_eda_panels(str(base / "lr"), str(base / "hr"), top_k_examples=2, rank_by="psnr")
    assert [str(f) for f in df["filename"]] == names and len(df["psnr"]) == 6 and np.all(np.isnan(df["lpips"]))
    assert set(panels) == set(E.PANEL_NAMES) | {"examples"}
    assert panels["advanced_global_panel"]["lr_fft_avg"].shape == (48, 40) and panels["distributions"]["lpips"] is None
    assert panels["correlation_matrix"]["corr"].shape == (10, 10) and len(panels["scatter_relations"]) == 8
    keys = expected_examples(df, names, 2)
    assert list(panels["examples"]) == [k for _, b, a in keys for k in (b, a)] and len(keys) == 4
    for rel, basic, adv in keys:
        lr, hr = E.ImagePairLoader.load_and_align(str(base / "lr" / rel), str(base / "hr" / rel))
        assert_panels_equal(panels["examples"][adv], E.ImageDataVisualization.advanced_panel(lr, hr))
        assert_panels_equal(panels["examples"][basic], E.ImageDataVisualization.visual_example(lr, hr))
    with pytest.raises(ValueError, match="rank_by"):
        E.run_eda_panels(str(base / "lr"), str(base / "hr"), rank_by="filename")


def test_run_eda_pipeline_writes_the_npz_tree(ctx, tree, tmp_path, capsys):
    from data import eda_methods as E
    base, names = tree
    out = tmp_path / "eda_results"
    df = E.run_eda_pipeline(str(base / "lr"), str(base / "hr"), output_dir=str(out), rank_by="psnr")
    assert "Interpolation map not found; default interpolation will be used." in capsys.readouterr().out
    _, panels = E.run_eda_panels(str(base / "lr"), str(base / "hr"), rank_by="psnr")
    expect = {f"{k}.npz": panels[k] for k in E.PANEL_NAMES}
    for rel, basic, adv in expected_examples(df, names, 1):
        expect[f"LPIPS_Scenarios/{basic}.npz"] = panels["examples"][basic]
        expect[f"LPIPS_Scenarios/{adv}.npz"] = panels["examples"][adv]
    written = sorted(os.path.relpath(os.path.join(r, f), out).replace(os.sep, "/") for r, _, fs in os.walk(out) for f in fs)
    assert written == sorted(expect) and len(written) == 7 + 4
    for rel, panel in expect.items():
        flat = E.ImageDataVisualization.flatten_panel(panel)
        with np.load(out / rel) as z:
            assert set(z.files) == set(flat), rel
            for k in flat:
                assert z[k].dtype == flat[k].dtype and z[k].tobytes() == flat[k].tobytes(), (rel, k)
    assert (out / "LPIPS_Scenarios" / "best_scenarios").is_dir() and (out / "LPIPS_Scenarios" / "worst_scenarios").is_dir()
    with pytest.raises(NotImplementedError, match="load_lpips"):
        E.run_eda_pipeline(str(base / "lr"), str(base / "hr"), output_dir=str(tmp_path / "other"))
    assert not math.isnan(df["psnr"][0])
