"""Classifying stacks of frames and scoring the SR comparison on the device (csrc/study.hip, Context.extract_patches_batch / patch_vote /
classification_counts, FineTunedVGG16.classify_defects_batch, stream_sr_classify(vote="device"), sr355.study.compare_sr_methods) against the
single-image path, the oracle and the NumPy restatements of tests/study_ref.py."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import study_ref as R
from oracle import models as M
from sr355 import _lib as L
from sr355.synth import make_pairs

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ 1. batched extraction, bit for bit
EXTRACT_CASES = [
    # F, H, W, C, patch, stride
    (3, 50, 37, 3, 16, 8),           # reflect tails of 8 on both axes, 6 x 4 windows
    (3, 32, 32, 3, 16, 16),          # no padding at all
    (3, 48, 48, 3, 32, 16),
    (3, 50, 37, 1, 16, 8),           # C = 1
    (3, 23, 19, 3, 7, 3),            # patch * C = 21, no multiple of 4: the per-element kernel
    (1, 50, 37, 3, 16, 8),           # F = 1
]


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("F,H,W,Cn,patch,stride", EXTRACT_CASES)
@pytest.mark.parametrize("in_u8", [False, True])
def test_extract_patches_batch_is_the_single_image_call_bit_for_bit(ctx, F, H, W, Cn, patch, stride, in_u8):
    from sr355.pipeline import patch_grid
    rng = np.random.default_rng(H * 1000 + W + Cn + patch)
    host = rng.integers(0, 256, (F, H, W, Cn)).astype(np.uint8) if in_u8 else rng.random((F, H, W, Cn)).astype(np.float32)
    imgs = ctx.to_device(host)
    ny, nx = patch_grid(H, W, patch, stride)
    if (H, W, patch, stride) == (50, 37, 16, 8):
        assert (ny, nx) == (6, 4)
    for out_dtype, mul, add in ((torch.float32, 1.0, 0.0), (torch.float32, 2.0, -1.0), (torch.bfloat16, 2.0, -1.0)):
        got = ctx.extract_patches_batch(imgs, patch, stride, mul=mul, add=add, out_dtype=out_dtype)
        assert tuple(got.shape) == (F * ny * nx, patch, patch, Cn) and got.dtype == out_dtype
        single = torch.cat([ctx.extract_patches(imgs[f].float().contiguous(), patch, stride, mul=mul, add=add, out_dtype=out_dtype) for f in range(F)])
        assert torch.equal(_bits(got), _bits(single))
        if out_dtype == torch.float32 and mul == 1.0:
            ref = np.concatenate([R.patches_ref(host[f], patch, stride) for f in range(F)])
            assert np.array_equal(got.cpu().numpy(), ref)


def test_extract_patches_batch_refuses_a_short_buffer_and_writes_nothing(ctx):
    imgs = ctx.to_device(np.random.default_rng(0).random((3, 50, 37, 3)).astype(np.float32))
    n = C.c_int()
    args = (ctx.h, imgs.data_ptr(), L.DTYPE_F32, 3, 50, 37, 3, 16, 8, 1.0, 0.0, L.DTYPE_F32)
    assert ctx.lib.sr_extract_patches_batch(*args, None, 0, C.byref(n), None) == L.SR_OK and n.value == 24
    need = 3 * 24 * 16 * 16 * 3
    out = torch.full((need,), -7.0, device=ctx.torch_device)
    assert ctx.lib.sr_extract_patches_batch(*args, out.data_ptr(), need - 1, C.byref(n), ctx.stream()) == L.SR_ERR_CAPACITY
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert ctx.lib.sr_extract_patches_batch(*args, out.data_ptr(), need, C.byref(n), ctx.stream()) == L.SR_OK
    assert torch.equal(out.view(72, 16, 16, 3), ctx.extract_patches_batch(imgs, 16, 8))
    with pytest.raises(ValueError):
        ctx.extract_patches_batch(imgs.to(torch.float64), 16, 8)


# ------------------------------------------------------------------------------------------------ 2. the vote
KINDS = ("majority", "tie2_mean", "tie3", "tie_equal_means", "equal_rows", "grid", "coarse")


def crafted(kind, P, K, rng):
    """[P,K] fp32 probabilities on the 1/256 grid: every sum over <= 1000 rows is exact in fp32 and fp64."""
    p = np.zeros((P, K), np.float64)
    rows = np.arange(P)
    if kind == "majority":
        w = np.where(rows < (3 * P + 4) // 5, K - 1, rng.integers(0, K, P))
        p = rng.integers(0, 200, (P, K)) / 256.0
        p[rows, w] = rng.integers(201, 257, P) / 256.0
    elif kind == "tie2_mean":                                # classes a < b share the vote; b has the higher mean and wins
        a, b = (0, 1) if K == 2 else (1, K - 1)
        n = P // 2
        p[:n, a], p[n:2 * n, b] = 0.5, 0.75
    elif kind == "tie3":                                     # K >= 3: three classes share the vote, the middle one has the highest mean
        c = (0, 1, 2) if K >= 3 else (0, 1, 1)
        n = P // 3
        p[:n, c[0]], p[n:2 * n, c[1]], p[2 * n:3 * n, c[2]] = 0.5, 0.75, 0.625
    elif kind == "tie_equal_means":                          # equal votes and exactly equal means: the lower index wins
        a, b = (0, 1) if K == 2 else (1, K - 1)
        n = P // 2
        p[:n, b], p[n:2 * n, a] = 0.5, 0.5
    elif kind == "equal_rows":                               # equal entries inside a row: the first index takes the patch
        p[:] = (rng.integers(1, 256, P) / 256.0)[:, None]
        p[rows % 2 == 1, 0] = 0.0                            # odd rows: classes 1.. are equal maxima, class 1 takes them
    elif kind == "grid":
        p = rng.integers(0, 257, (P, K)) / 256.0
    elif kind == "coarse":
        p = rng.integers(0, 4, (P, K)) / 4.0
    return p.astype(np.float32)


def _vote_case(ctx, frames):
    """frames: list of [P,K] arrays of one shape -> device result checked against the restatements; returns the references."""
    F, (P, K) = len(frames), frames[0].shape
    cls, conf, votes = ctx.patch_vote(ctx.to_device(np.concatenate(frames)), F, P, raw=True)
    assert cls.dtype == torch.int32 and conf.dtype == torch.float32 and votes.dtype == torch.int32 and tuple(votes.shape) == (F, K)
    cls, conf, votes = cls.cpu().numpy(), conf.cpu().numpy(), votes.cpu().numpy()
    refs = [R.vote_ref(f) for f in frames]
    for i, f in enumerate(frames):
        assert cls[i] == refs[i][0], (i, P, K, cls[i], refs[i])
        assert np.array_equal(votes[i], refs[i][2])
        assert conf[i] == np.float32(R.vote_ref64(f)[1]), (i, P, K)
    return refs


@pytest.mark.parametrize("K", [2, 3, 5, 64])
@pytest.mark.parametrize("P", [1, 9, 63, 64, 65, 1000])
def test_patch_vote_on_crafted_probabilities(ctx, K, P):
    rng = np.random.default_rng(100 * K + P)
    frames = [crafted(kind, P, K, rng) for kind in KINDS]                      # F = 7, a different case per frame
    refs = _vote_case(ctx, frames)
    for kind, f in zip(KINDS, frames):                                           # F = 1
        _vote_case(ctx, [f])
    by = dict(zip(KINDS, refs))
    assert by["majority"][0] == K - 1
    if P % 2 == 0:                                                               # the crafted ties are what they claim to be
        a, b = (0, 1) if K == 2 else (1, K - 1)
        win, _, votes = by["tie2_mean"]
        assert votes[a] == votes[b] == P // 2 and win == b
        win, _, votes = by["tie_equal_means"]
        assert votes[a] == votes[b] == P // 2 and win == a
    if P % 3 == 0 and K >= 3:
        win, _, votes = by["tie3"]
        assert votes[0] == votes[1] == votes[2] == P // 3 and win == 1
    if K >= 3 and P >= 2:
        assert by["equal_rows"][2][0] == (P + 1) // 2 and by["equal_rows"][2][1] == P // 2


@pytest.mark.parametrize("P", [9, 63, 65, 1001, 2047])
def test_patch_vote_on_random_softmax_rows(ctx, P):
    """K = 2 and odd P: the vote cannot tie.  The device's confidence is the fp64 mean rounded once: within 1 fp32 ulp of float32(vote_ref64)
    (the two fp64 sums differ in order only), and within 2e-6 of the reference's fp32 mean (NumPy's pairwise fp32 sum of P <= 2048 values in
    [0,1]: at most about log2(P) 2^-24 relative)."""
    rng = np.random.default_rng(P)
    frames = []
    for _ in range(7):
        e = np.exp(rng.normal(size=(P, 2)) * 2.0)
        frames.append((e / e.sum(axis=1, keepdims=True)).astype(np.float32))
    cls, conf, votes = ctx.patch_vote(ctx.to_device(np.concatenate(frames)), 7, P)
    assert cls.dtype == np.int64 and conf.dtype == np.float64
    again = ctx.patch_vote(ctx.to_device(np.concatenate(frames)), 7, P)
    assert np.array_equal(conf, again[1])
    for i, f in enumerate(frames):
        win, c32, v = R.vote_ref(f)
        c64 = np.float32(R.vote_ref64(f)[1])
        print(f"P={P} frame {i}: device {conf[i]!r} ref64 {float(c64)!r} ref32 {c32!r}")
        assert cls[i] == win and np.array_equal(votes[i], v)
        assert abs(np.float32(conf[i]) - c64) <= np.spacing(c64)
        assert abs(conf[i] - c32) <= 2e-6


@pytest.mark.parametrize("K", [0, 65])
def test_patch_vote_refuses_other_class_counts(ctx, K):
    probs = torch.zeros((4, max(K, 1)), device=ctx.torch_device)
    cls, conf = torch.zeros(2, dtype=torch.int32, device=ctx.torch_device), torch.zeros(2, device=ctx.torch_device)
    assert ctx.lib.sr_patch_vote(ctx.h, probs.data_ptr(), 2, 2, K, cls.data_ptr(), conf.data_ptr(), None, ctx.stream()) == L.SR_ERR_INVALID
    if K:
        with pytest.raises(ValueError):
            ctx.patch_vote(torch.zeros((4, K), device=ctx.torch_device), 2, 2)


# ------------------------------------------------------------------------------------------------ 3. classify_defects_batch
@pytest.fixture(scope="module")
def clf32(ctx):
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    c = FineTunedVGG16()
    c.setup_model(input_shape=(32, 32, 3), num_classes=2)           # seeded init (seed 4000)
    return c


def test_classify_defects_batch_is_the_single_image_path(ctx, clf32):
    _, hr = make_pairs(5, 12, 12, 4, seed=31)                        # five 48 x 48 frames: 3 x 3 = 9 patches of 32 / 16, no tie possible
    frames = [hr[0], (hr[1] * 255).astype(np.uint8), hr[2], ctx.to_device(hr[3]), hr[4]]
    cls, conf = clf32.classify_defects_batch(frames)
    assert cls.dtype == np.int64 and conf.dtype == np.float64 and cls.shape == conf.shape == (5,)
    for i, f in enumerate(frames):
        one = clf32.classify_defects_method(f)
        host = f.cpu().numpy() if isinstance(f, torch.Tensor) else np.asarray(f)
        ora = M.classify_defects(host.astype(np.float32), clf32.weights, 32, 16, dtype=np.float64)
        print(f"frame {i}: batch ({cls[i]}, {conf[i]!r}) single {one} oracle {ora}")
        assert cls[i] == one[0] == ora[0]
        assert abs(conf[i] - one[1]) <= 2e-6 and abs(conf[i] - ora[1]) <= 1e-4
    rc, rp = clf32.classify_defects_batch(frames, raw=True)
    assert rc.is_cuda and rp.is_cuda and rc.dtype == torch.int32 and rp.dtype == torch.float32
    assert np.array_equal(rc.cpu().numpy(), cls) and np.array_equal(rp.cpu().numpy().astype(np.float64), conf)
    # stacks: all-uint8 (the kernel reads the bytes), all-float, a device stack
    u8 = (hr * 255).astype(np.uint8)
    for stack in (u8, hr, ctx.to_device(hr), ctx.to_device(u8)):
        c2, p2 = clf32.classify_defects_batch(stack)
        ones = [clf32.classify_defects_method(stack[i]) for i in range(5)]
        assert list(c2) == [o[0] for o in ones] and np.max(np.abs(p2 - np.array([o[1] for o in ones]))) <= 2e-6
    # a budget of three frames' patches: two chunks, the same bits
    try:
        clf32.patch_budget_bytes = 3 * 9 * 32 * 32 * 3 * 4
        rc2, rp2 = clf32.classify_defects_batch(frames, raw=True)
    finally:
        del clf32.patch_budget_bytes
    assert torch.equal(rc, rc2) and torch.equal(rp, rp2)
    with pytest.raises(ValueError):
        clf32.classify_defects_batch([hr[0], hr[1][:40]])
    with pytest.raises(ValueError):
        clf32.classify_defects_batch(hr[..., :2])


# ------------------------------------------------------------------------------------------------ 4. the stream with the vote on the device
def test_stream_vote_on_the_device_equals_the_host_vote(ctx):
    from sr355.pipeline import stream_sr_classify
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    from SRModels.defect_detection_models.VGG16_model import FineTunedVGG16
    g = ESRGAN(compute_dtype="f32")
    g.setup_model(scale_factor=4, growth_channels=8, num_rrdb_blocks=1)
    g.set_weights(g.weights)
    c = FineTunedVGG16()
    c.setup_model(input_shape=(96, 96, 3), num_classes=2)
    lr, _ = make_pairs(5, 40, 36, 4, seed=18)
    frames = [lr[0], (lr[1] * 255).astype(np.uint8), lr[2], ctx.to_device(lr[3]), lr[4]]
    kw = dict(patch_size_lr=24, stride=12, batch_size=64)
    host, hstats = stream_sr_classify(g, c, frames, sr_kwargs=kw)
    dev, dstats = stream_sr_classify(g, c, frames, sr_kwargs=kw, vote="device", keep_sr=True)
    assert [r["frame"] for r in dev] == [r["frame"] for r in host] == [0, 1, 2, 3, 4]
    assert sorted(dstats) == sorted(hstats) and dstats["frames"] == 5 and dstats["frames_per_s"] > 0
    for h, d in zip(host, dev):
        print(f"frame {h['frame']}: host ({h['class']}, {h['confidence']!r}) device ({d['class']}, {d['confidence']!r})")
        assert sorted(d) == sorted(h) + ["sr"] and isinstance(d["class"], int) and isinstance(d["confidence"], float)
        assert d["class"] == h["class"] and abs(d["confidence"] - h["confidence"]) <= 2e-6
    parts = [stream_sr_classify(g, c, frames, sr_kwargs=kw, rank=r, world=2, vote="device")[0] for r in range(2)]
    assert [x["frame"] for x in parts[0]] == [0, 1, 2] and [x["frame"] for x in parts[1]] == [3, 4]
    assert [(x["class"], x["confidence"]) for p_ in parts for x in p_] == [(r["class"], r["confidence"]) for r in dev]
    with pytest.raises(ValueError):
        stream_sr_classify(g, c, frames, sr_kwargs=kw, vote="gpu")


# ------------------------------------------------------------------------------------------------ 5. counts
def test_classification_counts_equal_numpy(ctx):
    rng = np.random.default_rng(257)
    A, N, K = 3, 257, 4
    y, preds = rng.integers(0, K, N), rng.integers(0, K, (A, N))
    conf = rng.random((A, N)).astype(np.float32)
    cm, sums = ctx.classification_counts(y, preds, conf, num_classes=K)
    assert cm.dtype == torch.int64 and sums.dtype == torch.float64 and tuple(cm.shape) == (A, K, K) and tuple(sums.shape) == (A, 2)
    cm_h, sums_h = cm.cpu().numpy(), sums.cpu().numpy()
    for a in range(A):
        assert np.array_equal(cm_h[a], R.confusion_ref(y, preds[a], K))
        want = np.array([conf[a].astype(np.float64).sum(), conf[a][preds[a] == y].astype(np.float64).sum()])
        assert np.all(np.abs(sums_h[a] - want) <= 1e-12 * np.abs(want)), (sums_h[a], want)
    # device labels, a second call: the same bits
    cm2, sums2 = ctx.classification_counts(ctx.to_device(y.astype(np.int32)), ctx.to_device(preds.astype(np.int32)), ctx.to_device(conf), num_classes=K)
    assert torch.equal(cm, cm2) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64))
    cm3, sums3 = ctx.classification_counts(y, preds, num_classes=K)            # no confidences: zero sums
    assert torch.equal(cm3, cm) and float(sums3.abs().sum()) == 0.0
    assert torch.equal(ctx.classification_counts(y, preds)[0], cm)              # K from the host labels
    with pytest.raises(ValueError):
        ctx.classification_counts(y, preds, num_classes=3)                      # host labels are validated
    with pytest.raises(ValueError):
        ctx.classification_counts(y, ctx.to_device(preds.astype(np.int32)))     # device labels need num_classes


# ------------------------------------------------------------------------------------------------ 6. end to end
@pytest.mark.parametrize("h,w,seed,counts", [(24, 24, 63, (1, 9)),       # LR 24 x 24, HR 48 x 48
                                              (32, 24, 64, (2, 12))])     # LR 32 x 24, HR 64 x 48: even patch counts, a vote may tie
def test_compare_sr_methods_end_to_end(ctx, clf32, h, w, seed, counts):
    from sr355.study import compare_sr_methods, resize_method
    N, H, W = 6, 2 * h, 2 * w
    lr, hr = make_pairs(N, h, w, 2, seed=seed)
    y = np.array([0, 1, 1, 0, 1, 0])
    methods = OrderedDict([("LR", None), ("HR", None), ("bicubic", resize_method("INTER_CUBIC", H, W)),
                           ("bilinear", resize_method("INTER_LINEAR", H, W))])
    out = compare_sr_methods(clf32, lr, hr, y, methods)
    names = list(methods)
    assert list(out["labels"]) == list(out["confidences"]) == names and sorted(out) == ["confidence", "confidences", "confusion", "labels", "report"]
    lr_d = ctx.to_device(lr)
    frames = {"LR": lr_d, "HR": ctx.to_device(hr), "bicubic": ctx.resize(lr_d, H, W, "INTER_CUBIC"), "bilinear": ctx.resize(lr_d, H, W, "INTER_LINEAR")}
    # an up-scaled frame is 48 x 48: 9 patches.  An LR frame is 24 x 24: the loader's padding rule (loading_methods.py:12-17) adds
    # max((32 - 24 % 16) % 16, 32 - 16) = 16 rows and columns, a 40 x 40 image with a single window.  Both counts are odd, so with two classes
    # no vote of that case can tie; the second case (LR 32 x 24: 2 windows, HR 64 x 48: 12) has even counts, where the near-tie rule below applies.
    count = {n: ctx.num_patches(int(frames[n].shape[1]), int(frames[n].shape[2]), 3, 32, 16) for n in names}
    assert count == {"LR": counts[0], "HR": counts[1], "bicubic": counts[1], "bilinear": counts[1]}
    near_ties = 0
    for name in names:
        lab, cf = out["labels"][name], out["confidences"][name]
        assert lab.dtype == np.int64 and cf.dtype == np.float64 and lab.shape == cf.shape == (N,)
        P = count[name]
        probs = clf32.model.predict(ctx.extract_patches_batch(frames[name], 32, 16), batch_size=128).cpu().numpy().reshape(N, P, 2)
        for i in range(N):
            one = clf32.classify_defects_method(frames[name][i])
            top, means = R.tied_means(probs[i])
            tie = len(top) > 1
            gap = float(np.min(np.diff(np.sort(means)))) if tie else np.inf
            print(f"{name} frame {i}: study ({lab[i]}, {cf[i]!r}) single {one} tie {tie} gap {gap!r}")
            if tie and gap < 1e-6:                                              # either tied class would be accepted; capped at zero below
                near_ties += 1
                assert lab[i] in top
                continue
            assert lab[i] == R.vote_ref(probs[i])[0] == one[0]
            assert abs(cf[i] - one[1]) <= 2e-6
    assert near_ties == 0                                                       # the cap for the committed seeds
    labels = [out["labels"][n] for n in names]
    confs = [out["confidences"][n] for n in names]
    assert np.array_equal(out["confusion"], np.stack([R.confusion_ref(y, l, 2) for l in labels])) and out["confusion"].dtype == np.int64
    assert R.same(out["report"], R.report_ref(y, names, labels), 1e-12)
    assert R.same(out["confidence"], R.confidence_ref(y, names, labels, confs), 1e-12)


def test_model_methods_feed_the_comparison(ctx, clf32):
    """model_method over the new SRCNNModel / EDSR super_resolve_images: every frame of the batch is the oracle's super-resolved frame within
    the 1e-5 the single-image wrappers are held to (tests/test_wrappers_gpu.py), and compare_sr_methods classifies what the methods return."""
    from sr355.study import compare_sr_methods, model_method
    from SRModels.deep_learning_models.EDSR_model import EDSR
    from SRModels.deep_learning_models.SRCNN_model import SRCNNModel
    lr, hr = make_pairs(3, 24, 24, 2, seed=91)
    s = SRCNNModel()
    s.setup_model(input_shape=(24, 24, 3))
    s.set_weights(s.weights)
    e = EDSR()
    e.setup_model(scale_factor=2, num_res_blocks=2)
    e.set_weights(e.weights)
    methods = OrderedDict([("SRCNN", model_method(s, hr_h=48, hr_w=48)), ("EDSR", model_method(e, patch_size_lr=16, stride=8)), ("HR", None)])
    lr_d = ctx.to_device(lr)
    out_s, out_e = methods["SRCNN"](lr_d), methods["EDSR"](lr_d)
    assert tuple(out_s.shape) == tuple(out_e.shape) == (3, 48, 48, 3) and out_s.is_cuda and out_e.is_cuda
    for i in range(3):
        assert np.max(np.abs(out_s[i].cpu().numpy() - M.srcnn_super_resolve(lr[i], s.weights, 48, 48, dtype=np.float64))) <= 1e-5
        assert np.max(np.abs(out_e[i].cpu().numpy() - M.edsr_super_resolve(lr[i], e.weights, 2, 16, 8, num_res_blocks=2, dtype=np.float64))) <= 1e-5
    with pytest.raises(RuntimeError):
        EDSR().super_resolve_images([lr_d[0]])
    y = np.array([1, 0, 1])
    out = compare_sr_methods(clf32, lr, hr, y, methods)
    for name, frames in (("SRCNN", out_s), ("EDSR", out_e), ("HR", ctx.to_device(hr))):
        for i in range(3):
            one = clf32.classify_defects_method(frames[i])               # 9 patches, two classes: no tie
            assert out["labels"][name][i] == one[0] and abs(out["confidences"][name][i] - one[1]) <= 2e-6
    assert np.array_equal(out["confusion"], np.stack([R.confusion_ref(y, out["labels"][n], 2) for n in methods]))
