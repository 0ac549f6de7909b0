"""The experiment the reference exists for: which super-resolution method makes the VGG16 defect classifier more accurate?

`load_predictions_dataset` returns (X_LR, X_HR, y); `compare_sr_methods` takes them, up-scales X_LR with every method, classifies each
method's frames (`FineTunedVGG16.classify_defects_batch`), and scores the comparison with the numeric halves of
SRModels/deep_lerning_visualizations.py.  Every method's labels and confidences stay on the device until one
`Context.classification_counts` call; the study ends in one read.
"""
from collections import OrderedDict

import numpy as np
import torch

from .runtime import Context

BASELINES = ("HR", "LR")            # method names classified as they are: the HR frames (the ceiling) and the LR frames (no SR at all)


def resize_method(code, H, W):
    """A `cv2.resize(img, (W, H), interpolation=code)` method over Context.resize: code is an OpenCV name ("INTER_CUBIC", ...) or number."""
    if isinstance(code, bool) or (code not in Context.INTERPOLATIONS and code not in Context.INTERPOLATIONS.values()):
        raise ValueError(f"resize_method: unknown interpolation {code!r} (one of {sorted(Context.INTERPOLATIONS)})")
    H, W = int(H), int(W)

    def method(batch):
        return Context.get(batch.device).resize(batch, H, W, code)
    return method


def model_method(sr_model, **super_resolve_kwargs):
    """An SR-model method over `sr_model.super_resolve_images(frames, **super_resolve_kwargs)` (SRCNN, EDSR, ESRGAN): the frames' patches
    share the model's launches, the SR frames stay on the device."""
    if not callable(getattr(sr_model, "super_resolve_images", None)):
        raise ValueError("model_method: the model has no super_resolve_images")
    super_resolve_kwargs.setdefault("timed", False)

    def method(batch):
        srs, _ = sr_model.super_resolve_images(list(batch), **super_resolve_kwargs)
        return torch.stack(srs)
    return method


def _frames(X, name):
    """[N,H,W,3] array / tensor / list of equally sized frames -> the same, checked (ValueError on unequal sizes), without touching a device."""
    if isinstance(X, (list, tuple)):
        shapes = {tuple(np.shape(f)) for f in X}
        if len(shapes) != 1:
            raise ValueError(f"compare_sr_methods: the {name} frames must all have the same size, got {sorted(shapes)}")
        X = torch.stack(list(X)) if isinstance(X[0], torch.Tensor) else np.stack([np.asarray(f) for f in X])
    if len(X.shape) != 4 or X.shape[3] != 3 or X.shape[0] < 1:
        raise ValueError(f"compare_sr_methods: {name} must be an [N,H,W,3] RGB stack")
    return X


def compare_sr_methods(classifier, X_LR, X_HR, y, methods, patch_size=None, stride=None, batch_size=32, class_names=None):
    """Classify every method's version of the N frames and score the comparison.

    X_LR [N,h,w,3], X_HR [N,H,W,3] (float in [0,1] as load_predictions_dataset returns them, arrays, device tensors or lists of equally sized
    frames), y [N] labels in [0, num_classes).  `methods`: ordered mapping name -> callable taking the [N,h,w,3] fp32 device batch in [0,1]
    and returning an [N,H',W',3] device batch (resize_method, model_method, or any callable); the names "HR" and "LR" map to None (or
    anything: the value is ignored) and classify X_HR / X_LR as they are.

    Returns {"labels": {name: int64 [N]}, "confidences": {name: float64 [N]}, "report": classification_reports_metrics(...),
    "confidence": confidence_panel_stats(...), "confusion": int64 [A,K,K]} with A = len(methods), K the classifier's classes."""
    from SRModels import deep_lerning_visualizations as V
    X_LR, X_HR = _frames(X_LR, "X_LR"), _frames(X_HR, "X_HR")
    y_host = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).reshape(-1)
    N = int(X_LR.shape[0])
    if int(X_HR.shape[0]) != N or len(y_host) != N:
        raise ValueError("compare_sr_methods: X_LR, X_HR and y must hold the same number of frames")
    names = list(methods)
    if not names:
        raise ValueError("compare_sr_methods: no methods")
    for name in names:
        if name not in BASELINES and not callable(methods[name]):
            raise ValueError(f"compare_sr_methods: method {name!r} is neither a callable nor one of {BASELINES}")
    ctx = classifier.ctx
    K = int(np.asarray(classifier.weights["predictions"][0]).shape[-1])
    if y_host.size and (y_host.min() < 0 or y_host.max() >= K):
        raise ValueError(f"compare_sr_methods: y holds labels outside [0, {K})")
    to_dev = lambda X: (X.to(ctx.torch_device, torch.float32) if isinstance(X, torch.Tensor) else ctx.to_device(np.asarray(X, np.float32))).contiguous()
    lr, hr = to_dev(X_LR), None
    cls, conf = [], []
    for name in names:
        if name == "HR":
            hr = to_dev(X_HR) if hr is None else hr
            frames = hr
        elif name == "LR":
            frames = lr
        else:
            frames = methods[name](lr)
        c, p = classifier.classify_defects_batch(frames, patch_size=patch_size, stride=stride, batch_size=batch_size, raw=True)
        cls.append(c)
        conf.append(p)
    cls, conf = torch.stack(cls), torch.stack(conf)                                    # int32 / fp32 [A,N]
    cm, sums = ctx.classification_counts(y_host.astype(np.int32), cls, conf, num_classes=K)
    A = len(names)
    words = torch.cat([cm.reshape(-1).view(torch.int32), sums.reshape(-1).view(torch.int32), cls.reshape(-1),
                       conf.reshape(-1).view(torch.int32)]).cpu().numpy()             # the study's one read
    n_cm, n_s = 2 * A * K * K, 4 * A
    cm_h = words[:n_cm].view(np.int64).reshape(A, K, K).copy()
    sums_h = words[n_cm:n_cm + n_s].view(np.float64).reshape(A, 2).copy()
    cls_h = words[n_cm + n_s:n_cm + n_s + A * N].reshape(A, N).astype(np.int64)
    conf_h = words[n_cm + n_s + A * N:].view(np.float32).reshape(A, N).astype(np.float64)
    return {"labels": OrderedDict((n, cls_h[i]) for i, n in enumerate(names)),
            "confidences": OrderedDict((n, conf_h[i]) for i, n in enumerate(names)),
            "report": V.classification_reports_metrics(y_host, names, None, class_names=class_names, counts=(cm_h, sums_h)),
            "confidence": V.confidence_panel_stats(y_host, names, None, None, counts=(cm_h, sums_h)),
            "confusion": cm_h}
