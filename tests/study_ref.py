"""NumPy restatements the study tests compare against (reference: defect_detection_models/VGG16_model.py:247-268 and
SRModels/deep_lerning_visualizations.py:259-314, 455-495), written from the reference's lines with loops over classes."""
import numpy as np

from oracle import ops as OO


def _vote(probs, mean_dtype):
    probs = np.asarray(probs)
    if probs.ndim != 2:
        probs = probs.reshape((probs.shape[0], -1))
    num_classes = int(probs.shape[1])
    patch_preds = np.argmax(probs, axis=1)
    votes = np.bincount(patch_preds, minlength=num_classes)
    top_classes = np.where(votes == votes.max())[0]
    probs = probs.astype(mean_dtype)
    if len(top_classes) == 1:
        win = int(top_classes[0])
    else:
        mean_probs = probs.mean(axis=0)
        win = int(top_classes[np.argmax(mean_probs[top_classes])])
    return win, probs[:, win].mean(), votes


def vote_ref(probs):
    """VGG16_model.py:247-268 in NumPy fp32 -> (class, confidence float, votes)."""
    win, conf, votes = _vote(np.asarray(probs, np.float32), np.float32)
    return win, float(conf), votes


def vote_ref64(probs):
    """The same vote with fp64 means."""
    win, conf, votes = _vote(np.asarray(probs, np.float32), np.float64)
    return win, float(conf), votes


def tied_means(probs):
    """(tied classes, their fp64 means) of a frame's vote: the near-tie rule of the end-to-end test looks at these."""
    probs = np.asarray(probs, np.float32)
    votes = np.bincount(np.argmax(probs, axis=1), minlength=probs.shape[1])
    top = np.where(votes == votes.max())[0]
    return top, probs.astype(np.float64).mean(axis=0)[top]


def patches_ref(img, patch, stride):
    """[H,W,C] -> [P,patch,patch,C] fp32: oracle add_padding (reflect, bottom / right) and patch_positions."""
    img = np.asarray(img, np.float32)
    padded = OO.add_padding(img, patch, stride)
    pos = OO.patch_positions(padded.shape[0], padded.shape[1], patch, stride)
    return np.stack([padded[i:i + patch, j:j + patch, :] for i, j in pos]).astype(np.float32)


def report_ref(y_true, algo_names, preds_lists, class_names=None):
    """The metrics dict of plot_classification_reports_panel (:259-314, 416-423) with classification_report(labels=classes of y_true,
    zero_division=0) spelled out per class."""
    y_true = np.asarray(y_true)
    classes = sorted(np.unique(y_true))
    if class_names is None:
        class_names = [str(c) for c in classes]
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
        yt, yp = y_true[:n], y_pred[:n]
        f1s, recs, sups = [], [], []
        for c in classes:
            tp = float(np.sum((yt == c) & (yp == c)))
            n_pred, n_true = float(np.sum(yp == c)), float(np.sum(yt == c))
            prec = tp / n_pred if n_pred else 0.0
            rec = tp / n_true if n_true else 0.0
            f1s.append(2 * prec * rec / (prec + rec) if prec + rec else 0.0)
            recs.append(rec)
            sups.append(n_true)
        stray = any(v not in classes for v in np.unique(yp))          # classification_report then has 'micro avg' and no 'accuracy'
        out["accuracy"].append(np.nan if stray else float(np.mean(yt == yp)))
        out["macro_f1"].append(float(np.mean(f1s)))
        out["weighted_f1"].append(float(np.dot(f1s, sups) / np.sum(sups)))
        out["macro_recall"].append(float(np.mean(recs)))
        for i in range(min(C, len(classes))):
            f1_pc[i, j], acc_pc[i, j] = f1s[i], recs[i]
    out["f1_per_class"], out["acc_per_class"] = f1_pc, acc_pc
    return out


def confidence_ref(y, algo_names, label_lists, conf_lists):
    """The seven lists of plot_confidence_panel (:455-495)."""
    keys = ("mean_conf_all", "mean_conf_correct", "mean_conf_wrong", "error_rates", "counts", "counts_correct", "counts_wrong")
    out = {k: [] for k in keys}
    yt = np.asarray(y, dtype=int)
    with np.errstate(all="ignore"):
        import warnings
        for preds, confs in zip(label_lists, conf_lists):
            yp, cf = np.asarray(preds, dtype=int), np.asarray(confs, dtype=float)
            n = int(min(len(yt), len(yp), len(cf)))
            if n == 0:
                vals = (np.nan, np.nan, np.nan, np.nan, 0, 0, 0)
            else:
                correct = yp[:n] == yt[:n]
                cfs = cf[:n]
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore", RuntimeWarning)
                    vals = (float(np.nanmean(cfs)), float(np.nanmean(cfs[correct])) if np.any(correct) else np.nan,
                            float(np.nanmean(cfs[~correct])) if np.any(~correct) else np.nan, 1.0 - float(np.mean(correct)), n,
                            int(np.sum(correct)), int(n - np.sum(correct)))
            for k, v in zip(keys, vals):
                out[k].append(v)
    return out


def confusion_ref(y_true, preds, K):
    cm = np.zeros((K, K), np.int64)
    for t, p in zip(np.asarray(y_true), np.asarray(preds)):
        cm[int(t), int(p)] += 1
    return cm


def same(a, b, tol=1e-12):
    """Two metric dicts (lists / arrays of floats with NaNs, ints) agree: NaN where NaN, else within tol."""
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert x.shape == y.shape, (k, x.shape, y.shape)
        assert np.array_equal(np.isnan(x), np.isnan(y)), (k, x, y)
        assert np.all(np.abs(np.nan_to_num(x) - np.nan_to_num(y)) <= tol), (k, x, y)
    return True
