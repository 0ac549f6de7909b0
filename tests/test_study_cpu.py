"""The SR comparison's numbers without a device: classification_reports_metrics and its restatement (tests/study_ref.py) against
sklearn.metrics.classification_report read the way the reference reads it, confidence_panel_stats against the restatement, the vote
restatement against sr355.pipeline.majority_vote, and compare_sr_methods' argument checks."""
import numpy as np
import pytest

import study_ref as R


def _sklearn_metrics(y_true, algo_names, preds_lists, class_names=None):
    """plot_classification_reports_panel :259-314 with scikit-learn itself."""
    from sklearn.metrics import classification_report
    y_true = np.asarray(y_true)
    classes_sorted = sorted(np.unique(y_true))
    if class_names is None:
        class_names = [str(c) for c in classes_sorted]
    A, C = len(algo_names), len(class_names)
    out = {k: [] for k in ("accuracy", "macro_f1", "weighted_f1", "macro_recall")}
    f1_pc, acc_pc = np.full((C, A), np.nan), np.full((C, A), np.nan)
    for j, y_pred in enumerate(preds_lists):
        y_pred = np.asarray(y_pred)
        n = int(min(len(y_true), len(y_pred)))
        if n == 0:
            for k in out:
                out[k].append(np.nan)
            continue
        rep = classification_report(y_true[:n], y_pred[:n], labels=classes_sorted, target_names=class_names, output_dict=True, zero_division=0)
        out["accuracy"].append(float(rep.get("accuracy", np.nan)))
        out["macro_f1"].append(float(rep.get("macro avg", {}).get("f1-score", np.nan)))
        out["weighted_f1"].append(float(rep.get("weighted avg", {}).get("f1-score", np.nan)))
        out["macro_recall"].append(float(rep.get("macro avg", {}).get("recall", np.nan)))
        for i, cname in enumerate(class_names):
            f1_pc[i, j], acc_pc[i, j] = rep[cname]["f1-score"], rep[cname]["recall"]
    out["f1_per_class"], out["acc_per_class"] = f1_pc, acc_pc
    return out


def _report_cases():
    rng = np.random.default_rng(2024)
    y2, y4 = rng.integers(0, 2, 60), rng.integers(0, 4, 90)
    never = rng.integers(0, 3, 90)                                       # class 3 is never predicted
    y3 = rng.integers(0, 3, 50)
    stray = rng.integers(0, 4, 50)                                       # class 3 is predicted, y_true never has it
    assert 3 in stray and 3 not in y3 and 3 in y4 and 3 not in never
    return {
        "two_classes": (y2, [rng.integers(0, 2, 60), y2.copy(), 1 - y2]),
        "four_classes": (y4, [rng.integers(0, 4, 90), np.where(rng.random(90) < 0.7, y4, rng.integers(0, 4, 90))]),
        "class_never_predicted": (y4, [never, np.zeros(90, int)]),
        "predicted_class_absent_from_y_true": (y3, [stray, y3.copy()]),
        "unequal_lengths": (y4, [rng.integers(0, 4, 40), rng.integers(0, 4, 130), rng.integers(0, 4, 90)]),
        "empty_predictions": (y2, [np.zeros(0, int), rng.integers(0, 2, 60)]),
    }


@pytest.mark.parametrize("case", sorted(_report_cases()))
def test_report_metrics_equal_scikit_learn(case):
    pytest.importorskip("sklearn")
    from SRModels.deep_lerning_visualizations import classification_reports_metrics
    y, preds = _report_cases()[case]
    names = [f"m{i}" for i in range(len(preds))]
    want = _sklearn_metrics(y, names, preds)
    assert R.same(R.report_ref(y, names, preds), want, 1e-12)
    assert R.same(classification_reports_metrics(y, names, preds), want, 1e-12)
    if case == "predicted_class_absent_from_y_true":
        assert np.isnan(want["accuracy"][0]) and want["accuracy"][1] == 1.0 and np.isfinite(want["macro_f1"][0])
    if case == "empty_predictions":
        assert np.isnan(want["accuracy"][0]) and np.isnan(want["f1_per_class"][:, 0]).all()


def test_report_metrics_from_counts_equal_the_label_path():
    """The counts path (what sr355.study reads back from classification_counts) gives the label path's numbers, stray class included."""
    from SRModels.deep_lerning_visualizations import classification_reports_metrics, confidence_panel_stats, confusion_matrices
    rng = np.random.default_rng(5)
    y = rng.integers(0, 3, 70)
    preds = [rng.integers(0, 4, 70), rng.integers(0, 3, 70), y.copy()]
    conf = [rng.random(70).astype(np.float32).astype(np.float64) for _ in preds]
    cms = np.stack([R.confusion_ref(y, p, 4) for p in preds])
    assert np.array_equal(confusion_matrices(y, preds, labels=range(4)), cms)
    assert np.array_equal(confusion_matrices(y, preds), cms)
    sums = np.array([[c.sum(), c[p == y].sum()] for p, c in zip(preds, conf)])
    names = ["a", "b", "c"]
    assert R.same(classification_reports_metrics(y, names, None, counts=(cms, sums)), R.report_ref(y, names, preds), 1e-12)
    assert R.same(confidence_panel_stats(y, names, None, None, counts=(cms, sums)), R.confidence_ref(y, names, preds, conf), 1e-12)


def test_confidence_stats_equal_the_restatement():
    from SRModels.deep_lerning_visualizations import confidence_panel_stats
    rng = np.random.default_rng(11)
    y = rng.integers(0, 2, 40)
    with_nan = rng.random(40)
    with_nan[[3, 17, 30]] = np.nan
    labels = [rng.integers(0, 2, 40), y.copy(), 1 - y, rng.integers(0, 2, 25), np.zeros(0, int), rng.integers(0, 2, 40)]
    confs = [rng.random(40), rng.random(40), rng.random(40), rng.random(40), rng.random(40), with_nan]
    names = ["mixed", "all_correct", "all_wrong", "short", "empty", "nan_confidences"]
    got, want = confidence_panel_stats(y, names, labels, confs), R.confidence_ref(y, names, labels, confs)
    assert R.same(got, want, 1e-12)
    assert np.isnan(got["mean_conf_wrong"][1]) and np.isnan(got["mean_conf_correct"][2]) and got["counts"] == [40, 40, 40, 25, 0, 40]
    assert got["counts_wrong"][1] == 0 and got["error_rates"][2] == 1.0 and np.isnan(got["error_rates"][4])
    assert np.isfinite(got["mean_conf_all"][5]) and abs(got["mean_conf_all"][5] - np.nanmean(with_nan)) <= 1e-12


def test_vote_restatement_is_the_pipeline_vote():
    from sr355.pipeline import majority_vote
    rng = np.random.default_rng(77)
    for i in range(200):
        K, P = int(rng.integers(2, 6)), int(rng.integers(1, 40))
        if i % 3 == 0:                                                   # coarse grid: vote ties and equal entries do occur
            probs = rng.integers(0, 4, (P, K)).astype(np.float32) / 4
        else:
            e = np.exp(rng.normal(size=(P, K)))
            probs = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
        win, conf, votes = R.vote_ref(probs)
        assert (win, conf) == majority_vote(probs) and votes.sum() == P
        if i % 3 == 0:                                                   # grid values: the sums are exact, distinct sums are distinct means
            assert R.vote_ref64(probs)[0] == win


@pytest.mark.parametrize("name", ["plot_classification_reports_panel", "plot_confidence_panel", "plot_confusion", "plot_sr_metrics",
                                  "plot_sr_time", "plot_sr_memory", "plot_4x3"])
def test_plot_stubs_raise(name):
    from SRModels import deep_lerning_visualizations as V
    with pytest.raises(NotImplementedError) as e:
        getattr(V, name)([0, 1], ["a"], [[0, 1]])
    numeric = {"plot_classification_reports_panel": "classification_reports_metrics", "plot_confidence_panel": "confidence_panel_stats",
               "plot_confusion": "confusion_matrices"}.get(name)
    if numeric:
        assert numeric in str(e.value) and callable(getattr(V, numeric))


def test_compare_sr_methods_rejects_bad_arguments_before_touching_a_device(monkeypatch, tmp_path):
    from sr355 import _lib, study
    from sr355.runtime import Context
    monkeypatch.setattr(_lib, "_lib", None)                              # any attempt to reach the library (a device) would raise ImportError
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "libsr355.so"))
    monkeypatch.setattr(Context, "_instances", {})
    lr = [np.zeros((24, 24, 3), np.float32), np.zeros((24, 20, 3), np.float32)]
    hr = np.zeros((2, 48, 48, 3), np.float32)
    with pytest.raises(ValueError, match="same size"):
        study.compare_sr_methods(None, lr, hr, [0, 1], {"LR": None})
    with pytest.raises(ValueError, match="same size"):
        study.compare_sr_methods(None, hr, [hr[0], np.zeros((40, 48, 3), np.float32)], [0, 1], {"HR": None})
    with pytest.raises(ValueError, match="same number"):
        study.compare_sr_methods(None, hr[:, :24, :24], hr, [0, 1, 1], {"HR": None})
    with pytest.raises(ValueError, match="neither a callable"):
        study.compare_sr_methods(None, hr[:, :24, :24], hr, [0, 1], {"bicubic": "INTER_CUBIC"})
    for bad in ("INTER_BICUBIC", 17, True, None):
        with pytest.raises(ValueError, match="unknown interpolation"):
            study.resize_method(bad, 48, 48)
    with pytest.raises(ValueError, match="super_resolve_images"):
        study.model_method(object())
    assert callable(study.resize_method("INTER_CUBIC", 48, 48)) and callable(study.resize_method(1, 48, 48))
