"""The host half of the EDA panels (data/eda_methods.py: ImageDataVisualization's table numbers and global panel) against NumPy,
matplotlib.cbook and scipy.stats, on a seeded 40-row frame with one NaN; no GPU."""
import math

import numpy as np
import pytest

import eda_panels_ref as P
from data import eda_methods as E

V = E.ImageDataVisualization
NAN_COLUMN, NAN_ROW = "blocking_hr", 11


@pytest.fixture(scope="module")
def frame():
    rng = np.random.default_rng(2024)
    df = {"filename": np.array([f"a/p{i}.png" for i in range(40)], dtype=object)}
    for k in E.ImagePairMetrics.FIELDS[1:]:
        df[k] = rng.normal(rng.uniform(-3, 30), rng.uniform(0.5, 4), 40)
    df["ssim"] = 0.02 * df["psnr"] + rng.normal(0, 0.01, 40)          # one strongly correlated pair
    df["ringing_lr"][5] = df["ringing_lr"].mean() + 40.0               # one certain flier
    df[NAN_COLUMN][NAN_ROW] = math.nan
    return df


def test_basic_distributions_are_np_histogram(frame):
    got = V.basic_distributions_data(frame)
    assert tuple(got) == V.DISTRIBUTION_COLUMNS and len(got) == 9
    for k, (counts, edges) in got.items():
        col = frame[k][np.isfinite(frame[k])]
        rc, re = np.histogram(col, bins=30)
        assert np.array_equal(counts, rc) and np.array_equal(edges, re) and counts.sum() == col.size, k
    assert got[NAN_COLUMN][0].sum() == 39
    assert V.basic_distributions_data({**frame, "lpips": np.full(40, math.nan)})["lpips"] is None


def test_overlay_histograms_take_each_side_on_its_own_range(frame):
    got = V.artifact_color_histograms_data(frame)
    assert list(got) == [t for _, _, t in V.OVERLAY_PAIRS] + ["edge_diff", "edge_diff_kde"]
    for l, h, title in V.OVERLAY_PAIRS:
        for side, k in (("lr", l), ("hr", h)):
            rc, re = np.histogram(frame[k][np.isfinite(frame[k])], bins=30)
            assert np.array_equal(got[title][side][0], rc) and np.array_equal(got[title][side][1], re)
    assert np.array_equal(got["edge_diff"][0], np.histogram(frame["edge_diff"], bins=30)[0])


def test_kde_is_scipys_gaussian_kde_on_seaborns_grid(frame):
    stats = pytest.importorskip("scipy.stats")
    x = frame["edge_diff"]
    k = V.artifact_color_histograms_data(frame)["edge_diff_kde"]
    bw = np.std(x, ddof=1) * 40 ** (-1 / 5)
    assert k["bw"] == pytest.approx(bw, rel=1e-15) and k["grid"].shape == k["density"].shape == (200,)
    assert k["grid"][0] == pytest.approx(x.min() - 3 * bw, rel=1e-14) and k["grid"][-1] == pytest.approx(x.max() + 3 * bw, rel=1e-14)
    ref = stats.gaussian_kde(x)(k["grid"])
    rel = np.abs(k["density"] - ref) / ref
    print("kde max rel", rel.max())
    assert np.all(rel <= 1e-12)
    assert float(((k["density"][1:] + k["density"][:-1]) * np.diff(k["grid"])).sum() / 2) == pytest.approx(1.0, abs=5e-3)
    with_nan = np.concatenate([x, [math.nan]])
    assert np.array_equal(V.kde(with_nan)[1], k["density"]) and V.kde([1.0]) is None and V.kde([2.0, 2.0]) is None


def test_boxplot_stats_are_matplotlibs(frame):
    cbook = pytest.importorskip("matplotlib.cbook")
    got = V.artifact_boxplots_data(frame)
    labels = [f"{n} {s}" for n in ("Blocking", "Ringing", "Saturation", "Brightness", "ColorNoise") for s in ("LR", "HR")]
    assert list(got) == labels
    nfliers = 0
    for (l, h, name) in V.BOX_GROUPS:
        for side, k in (("LR", l), ("HR", h)):
            ref = cbook.boxplot_stats(frame[k][np.isfinite(frame[k])], whis=1.5)[0]
            g = got[f"{name} {side}"]
            for f in ("mean", "med", "q1", "q3", "iqr", "whislo", "whishi"):
                assert g[f] == float(ref[f]), (k, f)
            assert np.array_equal(g["fliers"], ref["fliers"]), k
            nfliers += g["fliers"].size
    assert nfliers >= 1 and got["Ringing LR"]["fliers"].max() == frame["ringing_lr"][5]
    assert V.boxplot_stats([math.nan]) is None


def test_correlation_matrix_is_pairwise_pearson(frame):
    got = V.correlation_matrix_data(frame)
    cols, c = got["columns"], got["corr"]
    assert cols == list(V.CORRELATION_COLUMNS) and c.shape == (10, 10)
    assert np.array_equal(c, c.T) and np.all(np.diag(c) == 1.0)
    for i, a in enumerate(cols):
        for j, b in enumerate(cols):
            m = np.isfinite(frame[a]) & np.isfinite(frame[b])
            assert m.sum() == (39 if NAN_COLUMN in (a, b) else 40)
            assert c[i, j] == pytest.approx(np.corrcoef(frame[a][m], frame[b][m])[0, 1], rel=1e-12, abs=1e-15), (a, b)
    assert c[cols.index("psnr"), cols.index("ssim")] > 0.9
    pd = pytest.importorskip("pandas")
    ref = pd.DataFrame({k: frame[k] for k in cols}).corr().to_numpy()
    assert np.allclose(c, ref, rtol=1e-12, atol=1e-15)
    two = {k: frame[k] for k in ("psnr", "ssim")}
    assert V.correlation_matrix_data(two) is None
    nan_col = V.correlation_matrix_data({**frame, "lpips": np.full(40, math.nan)})["corr"]
    assert np.all(np.isnan(nan_col[0])) and np.all(np.isnan(nan_col[:, 0])) and nan_col[1, 1] == 1.0


def test_channel_bars_and_scatter(frame):
    bars = V.channel_shape_bars_data(frame)
    assert set(bars) == {"skew_means_lr", "skew_means_hr", "kurt_means_lr", "kurt_means_hr"}
    assert bars["kurt_means_hr"] == [float(frame[f"ch{c}_kurt_hr"].mean()) for c in range(3)]
    assert V.channel_shape_bars_data({k: v for k, v in frame.items() if k != "ch1_skew_lr"}) is None
    sc = V.scatter_relations_data(frame)
    assert [(s["x"], s["y"]) for s in sc] == [(x, y) for x, y, _ in V.SCATTER_PAIRS] and len(sc) == 8
    assert np.array_equal(sc[4]["y_values"], frame["ringing_hr"]) and sc[4]["title"] == "Blocking vs Ringing"
    no_lpips = {k: v for k, v in frame.items() if k != "lpips"}
    assert [(s["x"], s["y"]) for s in V.scatter_relations_data(no_lpips)] == [(x, y) for x, y, _ in V.SCATTER_PAIRS[2:]]


def test_global_panel_on_hand_made_data():
    rng = np.random.default_rng(5)
    g = E.MetricsAggregator.new_global_data()
    assert V.global_advanced_panel(g) is None and V.global_advanced_panel(None) is None          # count == 0: the reference prints and returns
    glcm = rng.integers(0, 9, (256, 256)).astype(np.float64)
    g.update(count=4, lr_fft_sum=rng.uniform(0, 50, (9, 11)), hr_fft_sum=rng.uniform(0, 50, (9, 11)), grad_hr_sum=rng.uniform(0, 900, (9, 11)),
             glcm_sum=(glcm + glcm.T).reshape(256, 256, 1, 1), sat_lr_counts=rng.integers(0, 99, 50).astype(np.float64),
             sat_hr_counts=rng.integers(0, 99, 50).astype(np.float64), noise_means_lr=[1.5, 2.25, 0.5, 3.0])
    got, ref = V.global_advanced_panel(g), P.global_advanced_panel(g)
    for k, r in ref.items():
        assert np.array_equal(got[k], r), k
    assert got["glcm_avg"].shape == (256, 256) and got["glcm_avg"].sum() == pytest.approx(1.0, rel=1e-13)
    assert got["lr_log_spectrum"].tobytes() == np.log(g["lr_fft_sum"] / 4 + 1e-8).tobytes()
    assert got["sat_lr_density"].sum() * 5.12 == pytest.approx(1.0, rel=1e-9) and got["sat_centers"][0] == 2.56
    assert got["noise_mean"] == 1.8125 and np.array_equal(got["noise_hist"][0], np.histogram(g["noise_means_lr"], bins=30)[0])
    # a hand-made 3-level matrix: contrast = sum P (i - j)^2
    small = dict(g, glcm_sum=np.array([[2.0, 1, 0], [1, 0, 3], [0, 3, 2]]).reshape(3, 3, 1, 1))
    assert V.global_advanced_panel(small)["glcm_contrast"] == pytest.approx((2 * 1 + 6 * 1) / 12.0, rel=1e-15)


def test_plotting_names_raise_and_name_the_numeric_method():
    assert len(V._PLOTS) == 9
    for plot, numeric in V._PLOTS.items():
        assert callable(getattr(V, numeric))
        with pytest.raises(NotImplementedError, match=numeric):
            getattr(V, plot)(None, None, "out.png")
    with pytest.raises(NotImplementedError, match="advanced_panel"):
        V.create_advanced_visualizations(np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8), "x.png")


def test_flatten_panel_names(frame):
    flat = V.flatten_panel({"a": (np.arange(3), np.arange(4.0)), "b": {"c": [1.0, 2.0], "d": None}, "e": "name", "f": [{"x": "p", "v": np.zeros(2)}]})
    assert set(flat) == {"a.0", "a.1", "b.c", "e", "f.0.x", "f.0.v"} and flat["b.c"].tolist() == [1.0, 2.0] and str(flat["e"]) == "name"
    assert V.flatten_panel(None) == {}
    assert all(v.dtype != object for v in V.flatten_panel(V.correlation_matrix_data(frame)).values())


def test_pipeline_needs_lpips_weights_to_rank_by_lpips(tmp_path):
    assert E.ImageDatasetAnalyzer._lpips_ctx is None
    with pytest.raises(NotImplementedError, match="load_lpips"):
        E.run_eda_panels(str(tmp_path), str(tmp_path))
    with pytest.raises(NotImplementedError, match="load_lpips"):
        E.run_eda_pipeline(str(tmp_path), str(tmp_path), output_dir=str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_symbol_is_declared():
    from sr355 import _lib
    res, args = _lib.SIGNATURES["sr_eda_pair_panels"]
    assert len(args) == 15 and len(_lib.SIGNATURES["sr_eda_accumulate"][1]) == 12
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sr355.h")).read()
    assert "int  sr_eda_pair_panels(" in header and "SR_NUM_EDA_PANEL_SCALARS" in header
