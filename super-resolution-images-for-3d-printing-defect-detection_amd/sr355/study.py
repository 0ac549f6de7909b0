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


CLASSIC_ALGORITHMS = ("bilinear", "bicubic", "area", "lanczos", "ibp", "nlm", "egi", "freq")
# the notebook's eleven per-image collections, in build_metrics_summary's argument order, and the sr_classic_scores column behind each score
# (CLASSIC_STAT_KEYS[2:], in that order)
CLASSIC_STAT_KEYS = ("time", "memory", "psnr", "ssim", "mae", "rmse", "gradient_mse", "epi", "hf_energy_ratio", "kl_luma", "kl_color")
SCORE_COLUMNS = ("psnr", "ssim", "mae", "rmse", "grad_mse", "epi", "hf_ratio", "kl_luma", "kl_color")
assert SCORE_COLUMNS == Context.SCORE_NAMES
_RESIZES = (("bilinear", "INTER_LINEAR"), ("bicubic", "INTER_CUBIC"), ("area", "INTER_AREA"), ("lanczos", "INTER_LANCZOS4"))


def _u8_rgb_stack(X, name):
    """[N,H,W,3] uint8 array / tensor / list of equally sized frames -> one array or tensor, checked, without touching a device."""
    if isinstance(X, (list, tuple)):
        if not len(X):
            raise ValueError(f"classical_study: no {name} images")
        shapes = {tuple(np.shape(f)) for f in X}
        if len(shapes) != 1:
            raise ValueError(f"classical_study: the {name} images must all have the same size, got {sorted(shapes)}")
        X = torch.stack(list(X)) if isinstance(X[0], torch.Tensor) else np.stack([np.asarray(f) for f in X])
    elif not isinstance(X, torch.Tensor):
        X = np.asarray(X)
    floating = X.dtype.is_floating_point if isinstance(X, torch.Tensor) else np.issubdtype(X.dtype, np.floating)
    if floating:
        raise NotImplementedError(f"classical_study: float {name} images are not scored here (the notebook's loop runs on uint8 RGB)")
    if X.dtype not in (torch.uint8, np.uint8):
        raise NotImplementedError(f"classical_study: {name} images of dtype {X.dtype} (uint8 RGB only)")
    if len(X.shape) != 4 or X.shape[3] != 3 or X.shape[0] < 1:
        raise ValueError(f"classical_study: {name} must be an [N,H,W,3] RGB stack, got shape {tuple(X.shape)}")
    return X


def _read_packed(tensors):
    """Device tensors of any dtypes -> their NumPy copies, through ONE device-to-host copy of their concatenated bytes."""
    tensors = [t.contiguous() for t in tensors]
    raw = torch.cat([t.reshape(-1).view(torch.uint8) for t in tensors]).cpu().numpy()
    out, at = [], 0
    for t in tensors:
        n = t.numel() * t.element_size()
        out.append(raw[at:at + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)).copy())
        at += n
    return out


def classical_study(hr_images, lr_images, example_index=0, iterations=10, radius_frac=0.6, chunk=None):
    """The classical study's main loop (the reference's super_resolucion_clasica.ipynb, cell 8, and its summary, cell 9) for N image pairs
    as device batches: the four cv2.resize up-scalers on the uint8 RGB images, then back-projection (`iterations` rounds), NL-means,
    edge-guided interpolation and frequency extrapolation (normalised to uint8 by its own maximum) on their COLOR_RGB2GRAY images, every
    output scored against its HR image with the notebook's nine scores (`radius_frac` is hf_energy_ratio's).

    hr_images [N,H,W,3], lr_images [N,h,w,3]: uint8 RGB, arrays, device tensors or lists of equally sized frames.  The pairs run in
    chunks of `chunk` images (default: all N; the last chunk may be partial).  Nothing returns to the host between the launches: one read
    at the end brings every score, the NL-means flags and the frequency maxima (an image without detail then raises the ValueError of
    Context.non_local_means); a second read brings the example's images and their SSIM maps.

    time and memory are measurements, and per-chunk averages: time[alg] is the HIP-event time of the algorithm's own launches for a chunk
    (without its scoring), divided by the chunk's size, in seconds; memory[alg] the peak of device bytes above the level at the
    algorithm's start (the library's workspace, sr_mem_info, plus the tensors it allocates), divided by the chunk's size.  Each is repeated
    for the chunk's images, so within a chunk their variance and jitter are 0.

    Returns {"stats": {key: {alg: float64 [N]}} for CLASSIC_STAT_KEYS, "summary": build_metrics_summary(**stats),
    "examples": {"vis", "ibp_example", "nlm_example", "egi_example", "freq_example"} of pair `example_index` as the notebook collects them
    (NumPy), "ssim_maps": ssim_similarity_maps of them, "freq_max": float64 [N]}."""
    from SRModels.classic_super_resolution_algorithms import profiling_methods as P
    from SRModels.classic_super_resolution_algorithms import visualization_methods as VM
    hr_all, lr_all = _u8_rgb_stack(hr_images, "HR"), _u8_rgb_stack(lr_images, "LR")
    N, H, W = int(hr_all.shape[0]), int(hr_all.shape[1]), int(hr_all.shape[2])
    if int(lr_all.shape[0]) != N:
        raise ValueError(f"classical_study: {N} HR images for {int(lr_all.shape[0])} LR images")
    if isinstance(example_index, bool) or int(example_index) != example_index or not 0 <= example_index < N:
        raise ValueError(f"classical_study: example_index {example_index!r} is outside [0, {N})")
    chunk = N if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("classical_study: chunk must be at least 1")
    ctx = Context.get(hr_all.device) if isinstance(hr_all, torch.Tensor) and hr_all.is_cuda else Context.get()
    dev = ctx.torch_device
    hr_all = (hr_all if isinstance(hr_all, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hr_all))).to(dev).contiguous()
    lr_all = (lr_all if isinstance(lr_all, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lr_all))).to(dev).contiguous()

    measured = []                                  # (alg, chunk size, start event, end event, peak bytes)

    def run(alg, n, fn):
        """fn() between two events on the stream, with the device bytes it holds at its peak above the level it started from."""
        torch.cuda.reset_peak_memory_stats(dev)
        t0, lib0 = torch.cuda.memory_allocated(dev), ctx.mem_info()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        lib1 = ctx.mem_info()
        lib_peak = max(lib1["current"], lib1["peak"] if lib1["peak"] > lib0["peak"] else 0) - lib0["current"]
        measured.append((alg, n, e0, e1, max(0, torch.cuda.max_memory_allocated(dev) - t0) + max(0, lib_peak)))
        return out

    blocks = {a: [] for a in CLASSIC_ALGORITHMS}   # per algorithm, per chunk: float64 [n, 9] on the device
    flags, maxima, example = [], [], None
    for s in range(0, N, chunk):
        e = min(N, s + chunk)
        n = e - s
        hr, lr = hr_all[s:e], lr_all[s:e]
        outs = {a: run(a, n, lambda code=code: ctx.resize(lr, H, W, code)) for a, code in _RESIZES}
        hr_unit = ctx.u8_to_unit(hr)
        for a, _ in _RESIZES:                      # PSNR / SSIM of float32(u8) / 255 at range 1, the other columns of the uint8 pair
            block = ctx.classic_scores(hr, outs[a], 255.0, radius_frac)
            block[:, :2] = ctx.classic_scores(hr_unit, ctx.u8_to_unit(outs[a]), 1.0, radius_frac)[:, :2]
            blocks[a].append(block)
        hr_g, lr_g = ctx.rgb2gray(hr), ctx.rgb2gray(lr)
        outs["ibp"] = run("ibp", n, lambda: ctx.back_projection(hr_g, lr_g, int(iterations)))
        outs["nlm"], bad = run("nlm", n, lambda: ctx.non_local_means(lr_g, H, W, check=False))
        outs["egi"] = run("egi", n, lambda: ctx.edge_guided(lr_g, H, W))
        freq = run("freq", n, lambda: ctx.freq_extrapolate(lr_g, H, W))
        outs["freq"], mx = ctx.freq_to_u8(freq)
        flags.append(bad)
        maxima.append(mx)
        for a in ("ibp", "nlm", "egi", "freq"):    # kl_color is NaN for a gray pair
            blocks[a].append(ctx.classic_scores(hr_g, outs[a].contiguous(), "hr_span" if a == "nlm" else 255.0, radius_frac))
        if s <= example_index < e:
            i = int(example_index) - s
            example = [t[i].clone() for t in (hr, lr, outs["bilinear"], outs["bicubic"], outs["area"], outs["lanczos"], hr_g, lr_g, outs["ibp"],
                                              outs["nlm"], outs["egi"], outs["freq"])]
        del outs, freq, hr_unit

    scores, bad, freq_max = _read_packed([torch.stack([torch.cat(blocks[a]) for a in CLASSIC_ALGORITHMS]), torch.cat(flags),
                                          torch.cat(maxima)])               # the study's one read of its numbers: [8, N, 9], [N], [N]
    if bad.any():
        raise ctx.nlm_sigma_error(np.nonzero(bad)[0].tolist())
    stats = {k: {a: np.empty(N, np.float64) for a in CLASSIC_ALGORITHMS} for k in ("time", "memory")}
    at = dict.fromkeys(CLASSIC_ALGORITHMS, 0)
    for a, n, e0, e1, peak in measured:                                     # the events have completed: the read above waited for the stream
        stats["time"][a][at[a]:at[a] + n] = e0.elapsed_time(e1) * 1e-3 / n
        stats["memory"][a][at[a]:at[a] + n] = peak / n
        at[a] += n
    for k, col in zip(CLASSIC_STAT_KEYS[2:], SCORE_COLUMNS):
        stats[k] = {a: scores[i, :, Context.SCORE_NAMES.index(col)].copy() for i, a in enumerate(CLASSIC_ALGORITHMS)}
    stats = OrderedDict((k, stats[k]) for k in CLASSIC_STAT_KEYS)

    hr_i, lr_i, bil, bic, area, lan, hr_g, lr_g, ibp, nlm, egi, frq = example
    smap, sval = VM.ssim_maps_device((hr_i, lr_i, bil, bic, area, lan), (hr_g, lr_g, ibp), (hr_g, nlm), (hr_g, lr_g, egi), (hr_g, frq))
    host = _read_packed(example + [smap, sval])                             # the second read: the example's images and their SSIM maps
    hr_i, lr_i, bil, bic, area, lan, hr_g, lr_g, ibp, nlm, egi, frq, smap, sval = host
    nlm = nlm.astype(np.float64)                                            # as classic_algorithms.non_local_means returns it
    examples = OrderedDict([("vis", (hr_i, lr_i, bil, bic, area, lan)), ("ibp_example", (hr_g, lr_g, ibp)), ("nlm_example", (hr_g, nlm)),
                            ("egi_example", (hr_g, lr_g, egi)), ("freq_example", (hr_g, frq))])
    return {"stats": stats, "summary": P.build_metrics_summary(*(stats[k] for k in CLASSIC_STAT_KEYS)), "examples": examples,
            "ssim_maps": OrderedDict((nm, (smap[i].copy(), float(sval[i]))) for i, nm in enumerate(VM.SSIM_MAP_NAMES)), "freq_max": freq_max}


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
