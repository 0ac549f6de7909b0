"""The numeric halves of the reference's SRModels/deep_lerning_visualizations.py (the file name keeps the reference's spelling): the module in
which the comparison "which SR method makes the defect classifier more accurate" is scored.

Built: `classification_reports_metrics` (the `metrics` dict of plot_classification_reports_panel, :259-314, 416-423, without scikit-learn),
`confidence_panel_stats` (the seven lists of plot_confidence_panel, :455-495) and `confusion_matrices` (the `cm` plot_confusion draws).
Given device tensors (labels [A,N] as sr_patch_vote writes them) they go through one `Context.classification_counts` call and one small read;
given anything else they are plain NumPy and need no GPU.  `counts=(confusion, conf_sums)` hands over counts already read (sr355.study).
Not built: every matplotlib panel -- the `plot_*` functions raise NotImplementedError and name the numeric function.
"""
import numpy as np

try:                                                    # the NumPy halves need no torch tensor; only the device path looks at the type
    import torch
except ImportError:                                     # pragma: no cover
    torch = None


def _is_device(x):
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _device_counts(y_true, preds, conf, num_classes):
    """-> (confusion int64 [A,K,K], conf_sums float64 [A,2]) on the host: one classification_counts call, one read."""
    from sr355 import Context
    if num_classes is None:
        raise ValueError("num_classes is required with device labels")
    ctx = Context.get(preds.device)
    cm, sums = ctx.classification_counts(y_true, preds, conf, num_classes=num_classes)
    words = torch.cat([cm.reshape(-1), sums.reshape(-1).view(torch.int64)]).cpu().numpy()
    n = cm.numel()
    return words[:n].reshape(tuple(cm.shape)).copy(), words[n:].view(np.float64).reshape(-1, 2).copy()


def _host(x):
    return x.cpu().numpy() if torch is not None and isinstance(x, torch.Tensor) else np.asarray(x)


def _confusion_host(yt, yp, labels):
    """rows = true label, columns = predicted label, both over `labels`; a pair with a label outside `labels` is counted in no cell."""
    labels = list(labels)
    cm = np.zeros((len(labels), len(labels)), np.int64)
    for i, a in enumerate(labels):
        ta = yt == a
        for j, b in enumerate(labels):
            cm[i, j] = int(np.sum(ta & (yp == b)))
    return cm


def confusion_matrices(y_true, preds_lists, labels=None, num_classes=None):
    """The `cm` plot_confusion draws, per method: int64 [A,K,K], rows = true label, columns = predicted label.  `labels` defaults to the sorted
    labels found in y_true and the predictions (sklearn's confusion_matrix default); device tensors are counted by
    Context.classification_counts over range(num_classes)."""
    if _is_device(preds_lists):
        return _device_counts(y_true, preds_lists, None, num_classes)[0]
    yt = _host(y_true)
    preds = [_host(p) for p in preds_lists]
    if labels is None:
        labels = sorted(np.unique(np.concatenate([yt.reshape(-1)] + [p.reshape(-1) for p in preds])))
    out = []
    for yp in preds:
        n = int(min(len(yt), len(yp)))
        out.append(_confusion_host(yt[:n], yp[:n], labels))
    return np.stack(out) if out else np.zeros((0, len(labels), len(labels)), np.int64)


def _report_row(cm, is_class):
    """One method's numbers from its confusion matrix over every label met (classes and stray predictions alike); `is_class` marks the
    labels classification_report is given (the classes of y_true).  -> (accuracy, macro_f1, weighted_f1, macro_recall, f1 [C], recall [C])."""
    cm = np.asarray(cm, np.float64)
    idx = np.where(is_class)[0]
    n = cm[idx].sum()                                   # every true label is a class
    tp = np.diag(cm)[idx]
    true_sum, pred_sum = cm.sum(axis=1)[idx], cm.sum(axis=0)[idx]
    div = lambda a, b: np.divide(a, b, out=np.zeros_like(a), where=b != 0)          # zero_division=0
    recall, f1 = div(tp, true_sum), div(2.0 * tp, true_sum + pred_sum)
    stray = cm[:, ~np.asarray(is_class)].sum() > 0      # a predicted label y_true never has: sklearn emits 'micro avg', not 'accuracy'
    acc = np.nan if stray else float(tp.sum() / n)
    return acc, float(np.mean(f1)), float(np.sum(f1 * true_sum) / n), float(np.mean(recall)), f1, recall


def classification_reports_metrics(y_true, algo_names, preds_lists, class_names=None, num_classes=None, counts=None):
    """The `metrics` dict of plot_classification_reports_panel (:259-314, 416-423): 'accuracy', 'macro_f1', 'weighted_f1', 'macro_recall' (lists,
    one entry per method) and 'f1_per_class', 'acc_per_class' ([C,A] arrays; the latter is the per-class recall), as
    sklearn.metrics.classification_report(labels=classes of y_true, zero_division=0) gives them.  Classes are the sorted unique values of
    y_true; a method's length is truncated to the shorter of (y_true, its predictions), an empty one gives NaN; macro and weighted averages
    run over those classes only; a prediction holding a label y_true never has makes that method's 'accuracy' NaN (classification_report then
    emits 'micro avg' instead, and the reference reads report.get('accuracy', nan)).

    preds_lists a device tensor [A,N] (with y_true host or device, num_classes given): counted by Context.classification_counts, one read.
    counts=(confusion [A,K,K], ...) over labels range(K): those counts are used and nothing is counted again."""
    if counts is not None or _is_device(preds_lists):
        cms = np.asarray(counts[0]) if counts is not None else _device_counts(y_true, preds_lists, None, num_classes)[0]
        A, K = cms.shape[0], cms.shape[1]
        # the classes of y_true: every method's matrix has the same row sums
        is_class = cms[0].sum(axis=1) > 0 if A else np.zeros(K, bool)
        classes_sorted = [int(k) for k in np.where(is_class)[0]]
        rows = [(cm, is_class) for cm in cms]
    else:
        yt_all = _host(y_true)
        classes_sorted = sorted(np.unique(yt_all))
        rows = []
        for y_pred in preds_lists:
            yp = _host(y_pred)
            n = int(min(len(yt_all), len(yp)))
            if n == 0:
                rows.append(None)
                continue
            yt, yp = yt_all[:n], yp[:n]
            labels = list(classes_sorted) + [v for v in np.unique(yp) if v not in set(classes_sorted)]
            rows.append((_confusion_host(yt, yp, labels), np.arange(len(labels)) < len(classes_sorted)))
    if class_names is None:
        class_names = [str(c) for c in classes_sorted]
    n_methods, n_classes = len(algo_names), len(class_names)
    accuracies, macro_f1s, weighted_f1s, macro_recalls = [], [], [], []
    f1_per_class = np.full((n_classes, n_methods), np.nan, dtype=float)
    acc_per_class = np.full((n_classes, n_methods), np.nan, dtype=float)
    for j, (_, row) in enumerate(zip(algo_names, rows)):
        if row is None or np.asarray(row[0]).sum() == 0:
            for lst in (accuracies, macro_f1s, weighted_f1s, macro_recalls):
                lst.append(np.nan)
            continue
        acc, mf1, wf1, mrec, f1, rec = _report_row(*row)
        accuracies.append(acc)
        macro_f1s.append(mf1)
        weighted_f1s.append(wf1)
        macro_recalls.append(mrec)
        for i in range(min(n_classes, len(f1))):        # report[cname]: a name beyond the classes is a KeyError there, NaN here
            f1_per_class[i, j], acc_per_class[i, j] = f1[i], rec[i]
    return {"accuracy": accuracies, "macro_f1": macro_f1s, "weighted_f1": weighted_f1s, "macro_recall": macro_recalls,
            "f1_per_class": f1_per_class, "acc_per_class": acc_per_class}


def _nanmean(a):
    """np.nanmean without its warning: NaN for an empty or all-NaN selection."""
    a = a[~np.isnan(a)]
    return float(np.mean(a)) if a.size else float("nan")


def confidence_panel_stats(y, algo_names, label_lists, conf_lists, num_classes=None, counts=None):
    """The seven lists plot_confidence_panel computes (:455-495), as a dict: 'mean_conf_all', 'mean_conf_correct', 'mean_conf_wrong',
    'error_rates', 'counts', 'counts_correct', 'counts_wrong', one entry per method.  Lengths are truncated to the shortest of (y, labels,
    confidences); an empty method gives NaN means and zero counts; the means are nanmeans, NaN where no prediction is correct / wrong.

    label_lists and conf_lists device tensors [A,N] (num_classes given), or counts=(confusion [A,K,K], conf_sums [A,2]): the means are
    quotients of classification_counts' fp64 sums and the matrices' traces.  Those sums are plain sums: the device path is for the finite
    confidences sr_patch_vote writes (a NaN confidence makes that method's means NaN there, where nanmean would skip it)."""
    if counts is not None or _is_device(label_lists):
        cms, sums = counts if counts is not None else _device_counts(y, label_lists, conf_lists, num_classes)
        out = {k: [] for k in ("mean_conf_all", "mean_conf_correct", "mean_conf_wrong", "error_rates", "counts", "counts_correct", "counts_wrong")}
        for cm, (s_all, s_ok) in zip(np.asarray(cms), np.asarray(sums, np.float64)):
            n, ok = int(cm.sum()), int(np.trace(cm))
            out["mean_conf_all"].append(float(s_all / n) if n else np.nan)
            out["mean_conf_correct"].append(float(s_ok / ok) if ok else np.nan)
            out["mean_conf_wrong"].append(float((s_all - s_ok) / (n - ok)) if n - ok else np.nan)
            out["error_rates"].append(1.0 - ok / n if n else np.nan)
            out["counts"].append(n)
            out["counts_correct"].append(ok)
            out["counts_wrong"].append(n - ok)
        return out
    mean_conf_all, mean_conf_correct, mean_conf_wrong, error_rates, counts_, counts_correct, counts_wrong = [], [], [], [], [], [], []
    yt = np.asarray(_host(y), dtype=int)
    for preds, confs in zip(label_lists, conf_lists):
        yp = np.asarray(_host(preds), dtype=int)
        cf = np.asarray(_host(confs), dtype=float)
        n = int(min(len(yt), len(yp), len(cf)))
        if n == 0:
            mean_conf_all.append(np.nan)
            mean_conf_correct.append(np.nan)
            mean_conf_wrong.append(np.nan)
            error_rates.append(np.nan)
            counts_.append(0)
            counts_correct.append(0)
            counts_wrong.append(0)
            continue
        y_true, y_pred, cfs = yt[:n], yp[:n], cf[:n]
        correct = y_pred == y_true
        mean_conf_all.append(_nanmean(cfs))
        mean_conf_correct.append(_nanmean(cfs[correct]) if np.any(correct) else np.nan)
        mean_conf_wrong.append(_nanmean(cfs[~correct]) if np.any(~correct) else np.nan)
        error_rates.append(1.0 - float(np.mean(correct)))
        counts_.append(n)
        counts_correct.append(int(np.sum(correct)))
        counts_wrong.append(int(n - np.sum(correct)))
    return {"mean_conf_all": mean_conf_all, "mean_conf_correct": mean_conf_correct, "mean_conf_wrong": mean_conf_wrong,
            "error_rates": error_rates, "counts": counts_, "counts_correct": counts_correct, "counts_wrong": counts_wrong}


def _not_built(name, numeric):
    def plot(*args, **kwargs):
        raise NotImplementedError(f"{name}: the matplotlib panel is not built" + (f"; its numbers are {numeric}(...)" if numeric else ""))
    plot.__name__ = name
    plot.__doc__ = f"Not built (a matplotlib panel)." + (f"  The numbers it draws: {numeric}." if numeric else "")
    return plot


plot_classification_reports_panel = _not_built("plot_classification_reports_panel", "classification_reports_metrics")
plot_confidence_panel = _not_built("plot_confidence_panel", "confidence_panel_stats")
plot_confusion = _not_built("plot_confusion", "confusion_matrices")
plot_sr_metrics = _not_built("plot_sr_metrics", None)
plot_sr_time = _not_built("plot_sr_time", None)
plot_sr_memory = _not_built("plot_sr_memory", None)
plot_4x3 = _not_built("plot_4x3", None)
