"""The streamed dense-block kernel (csrc/dense_block_stream.hip, dense_block_stream<bf16,g8>): a whole dense block of the reference notebook's generator
(8 growth channels) as one kernel that streams the image's rows through a ring in LDS -- the patches the LDS-resident kernel cannot hold (48 x 48).

1. every conv of every block per element against an fp64 restatement fed with the DEVICE's own inputs (tests/dense_ref.py), at the shapes where a mechanism can
   go wrong: nothing but border, images shorter than the pipeline, ring wraps, both schedules (one phase per step up to W = 64, five beyond) on either side of
   their boundary, the widest ring;
2. where the LDS-resident kernel applies as well, the streamed kernel gives its bits, output and growth slices;
3. exact small integers: the growth convs' taps equal the layer-by-layer path's bit for bit, and the fp64 integers;
4. an image's result depends neither on the band count, nor on the batch, the workgroup, taps, nor on what the ring held before (NaNs included);
5. everything the route does not take still runs what it ran; the setter refuses the models the kernel cannot serve;
6. whole forwards against the CPU oracle, through Model and through the ESRGAN wrapper at super_resolve_image's default patch size.
Widths at the edges are read from sr_dense_block_stream_lds_bytes, not copied."""
import numpy as np
import pytest
import torch

import dense_ref as D
from oracle import models as M
from sr355 import Context, Model
from sr355 import _lib as L
from sr355.weights import bf16_rounded, init_weights

pytestmark = pytest.mark.gpu

STREAM = "dense_block_stream<bf16,g8>"
BLOCK = "dense_block_lds<bf16,g8>"
TILE_GROWTH = "conv_rows<bf16,k3,kg1,nt2>"            # a dense-block growth conv on the tile kernel
G = 8
NB = 2
# conv5's kernel and bias times 2^K5 for the conv5 check, as in test_dense_block_gpu.py: on plain random weights the skips hide 0.2 * conv5.  2^4 -- except on
# 1 x 1 images, where eight of conv5's nine taps see nothing but border (2^6).  The test asserts per block that the scaled conv term stands above the skips.
K5, K5_ONE_PIXEL = 4, 6


def ring(w, g=G):
    return Context.dense_block_stream_lds_bytes(g, w)


def widest():
    """The largest W the kernel takes."""
    w = 1
    while ring(w + 1) > 0:
        w += 1
    assert ring(w) > 0 and ring(w + 1) == -1
    return w


@pytest.fixture()
def fused_ctx(ctx):
    yield ctx
    ctx.set_fused(ctx.FUSED_ALL, 0)
    ctx.set_block_stream_bands(0)


_MODELS = {}


def model_of(ctx, key, mode, num_blocks=NB, growth=G, dtype="bf16", seed=5100):
    """key 'random': bf16-rounded seeded weights; ('conv5', k): the same with every dense block's conv5 (kernel and bias) times 2^k.  mode: sr_model_set_dense_block_stream's;
    None: a model the setter was never called on."""
    k = (key, num_blocks, growth, dtype, seed, mode is None)
    if k not in _MODELS:
        m = Model("esrgan_g", compute_dtype=dtype, scale_factor=2, num_blocks=num_blocks, growth_channels=growth, use_attention=False, ctx=ctx)
        w = bf16_rounded(init_weights(m.layer_shapes(), seed=seed))
        if key != "random":
            s = np.float32(2.0 ** key[1])
            w = {n: ((kb[0] * s, kb[1] * s) if n.endswith("_conv5") and "_dense" in n else kb) for n, kb in w.items()}
        m.set_weights(w)
        _MODELS[k] = (m, w)
    m, w = _MODELS[k]
    if mode is not None:
        m.set_dense_block_stream(mode)
    return m, w


def images(shape, seed):
    return D.rbf(np.random.default_rng(seed).uniform(-1, 1, tuple(shape) + (3,))).astype(np.float32)


def profiled(ctx, fn):
    ctx.profile_begin()
    out = fn()
    return out, {r["kernel"] for r in ctx.profile_end()}


BLOCKS = [f"rrdb_{b}_dense{d}" for b in range(NB) for d in (1, 2, 3)]
ALL_TAPS = ["initial_conv"] + [f"{n}_conv{k}" for n in BLOCKS for k in (1, 2, 3, 4, 5)]
GROWTH_TAPS = [f"{n}_conv{k}" for n in BLOCKS for k in (1, 2, 3, 4)]


# ------------------------------------------------------------------------------------------------ 1. every conv per element
# (B, H, W, workgroup cap, mode); W = "max": the largest W sr_dense_block_stream_lds_bytes accepts
CASES = [
    (3, 1, 1, 0, 2),         # nothing but border
    (2, 3, 17, 0, 2),        # shorter than the pipeline's skew, a partial second tile
    (2, 5, 31, 0, 2),
    (2, 9, 21, 1, 2),        # two images on one workgroup
    (1, 40, 5, 0, 2),        # many turns of the ring
    (2, 48, 48, 0, 1),       # the target, as the wrapper's option routes it
    (1, 14, 64, 0, 2),       # the widest image of the one-phase schedule: two tile groups per row, the second of one tile
    (1, 7, 65, 0, 2),        # the first of the five-phase schedule, a one-pixel fifth tile
    (1, 7, "max", 0, 2),     # on the edge of the LDS
    (1, 12, 96, 0, 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_conv_per_element(fused_ctx, case):
    ctx = fused_ctx
    B, H, W, cap, mode = case
    if W == "max":
        W = widest()
    x = images((B, H, W), B * 1000 + H * 10 + W)
    xd = ctx.to_device(x, torch.bfloat16)
    for key in ("random", ("conv5", K5_ONE_PIXEL if H * W == 1 else K5)):
        m, w = model_of(ctx, key, mode)
        ctx.set_fused(ctx.FUSED_ALL, cap)
        (_, taps), ran = profiled(ctx, lambda: m.forward_with_taps(xd, ALL_TAPS))
        assert STREAM in ran and BLOCK not in ran and not any(k.startswith(TILE_GROWTH) for k in ran), ran
        t = {n: v.cpu().numpy().astype(np.float64) for n, v in taps.items()}
        assert t["initial_conv"].shape == (B, H, W, 64) and all(t[n].shape == (B, H, W, G) for n in GROWTH_TAPS)
        for bi, name in enumerate(BLOCKS):
            d = int(name[-1])
            xin = t["initial_conv"] if bi == 0 else t[BLOCKS[bi - 1] + "_conv5"]
            c = [t[f"{name}_conv{k}"] for k in (1, 2, 3, 4)]
            so = None
            if d == 3:                                                        # the RRDB's input: initial_conv or the previous RRDB's output
                so = t["initial_conv"] if bi < 3 else t[BLOCKS[bi - 3] + "_conv5"]
            tag = f"{key} {case} {name}"
            if key == "random":
                feats = [xin]
                for k in (1, 2, 3, 4):
                    worst = D.assert_bf16_close(c[k - 1], D.growth_ref(feats, w, name, k), what=f"{tag}_conv{k}")
                    print(f"RATIO {STREAM} conv{k} {tag} {worst:.4f}")
                    feats.append(c[k - 1])
            else:
                ref = D.tail_ref(xin, *c, w, name, so)
                ct, sk = D.tail_terms(xin, *c, w, name, so)
                cm, sm = float(np.median(ct)), float(np.median(sk))
                print(f"MEDIANS {tag} |alpha conv5| {cm:.4g} |skips| {sm:.4g}")
                assert cm > sm > 0, (tag, cm, sm)                             # the scaled conv5 stands above the skips: a wrong conv5 cannot hide
                worst = D.assert_bf16_close(t[f"{name}_conv5"], ref, scale=max(1.0, D.rms(ref)), what=f"{tag}_conv5")
                print(f"RATIO {STREAM} conv5 {tag} {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 2. the resident kernel's bits
@pytest.mark.parametrize("case", [(5, 24, 24, 2), (4, 13, 21, 3), (3, 1, 1, 0)], ids=lambda c: "x".join(map(str, c)))
def test_bits_of_the_resident_kernel(fused_ctx, case):
    ctx = fused_ctx
    B, H, W, cap = case
    xd = ctx.to_device(images((B, H, W), 200 + H + W), torch.bfloat16)
    ctx.set_fused(ctx.FUSED_ALL, cap)
    m, _ = model_of(ctx, "random", 0)
    (y0, t0), ran0 = profiled(ctx, lambda: m.forward_with_taps(xd, GROWTH_TAPS))
    assert BLOCK in ran0 and STREAM not in ran0, ran0
    m, _ = model_of(ctx, "random", 2)
    (y2, t2), ran2 = profiled(ctx, lambda: m.forward_with_taps(xd, GROWTH_TAPS))
    assert STREAM in ran2 and BLOCK not in ran2, ran2
    assert torch.equal(y2, y0)
    for n in GROWTH_TAPS:
        assert torch.equal(t2[n], t0[n]), n
    assert torch.equal(m.forward(xd), y0)                                     # untapped as well


# ------------------------------------------------------------------------------------------------ 3. exact integers
@pytest.mark.parametrize("shape,mode", [((7, 11, 24), 2), ((2, 30, 48), 1)], ids=["7x11x24-mode2", "2x30x48-mode1"])
def test_growth_convs_exact_integers(fused_ctx, shape, mode):
    ctx = fused_ctx
    m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=1, growth_channels=G, use_attention=False, ctx=ctx, dense_block_stream=mode)
    shapes = m.layer_shapes()
    x = np.random.default_rng(D.EXACT_SEED).integers(-1, 2, size=shape + (3,)).astype(np.float32)
    name = "rrdb_0_dense1"
    for density in (0.06, 0.05, 0.04, 0.03, 0.02, 0.01):                      # the largest at which every sum of the first block's growth convs stays below 2^8
        w = D.exact_integer_weights(shapes, density, D.EXACT_SEED)
        feats = [D.conv(x, w["initial_conv"])]
        largest = float(np.abs(feats[0]).max())
        for k in (1, 2, 3, 4):
            largest = max(largest, float(np.abs(D.conv(D.cat(*feats), w[f"{name}_conv{k}"])).max()))      # the sums, before the ReLU
            feats.append(D.growth_ref(feats, w, name, k))
        if largest < 2 ** 8:
            break
    assert largest < 2 ** 8, "no density keeps the integers exact in bf16"
    assert all(np.array_equal(f, np.round(f)) for f in feats) and all(float(f.max()) > 0 for f in feats[1:])
    m.set_weights(w)                                                          # (the constructor's mode is set after every finalize)
    xd = ctx.to_device(x, torch.bfloat16)
    names = [f"{name}_conv{k}" for k in (1, 2, 3, 4)]
    ctx.set_fused(ctx.FUSED_ALL, 0)
    (_, fused), ran = profiled(ctx, lambda: m.forward_with_taps(xd, names))
    assert STREAM in ran and BLOCK not in ran, ran
    ctx.set_fused(0, 0)
    (_, plain), ran0 = profiled(ctx, lambda: m.forward_with_taps(xd, names))
    assert STREAM not in ran0 and BLOCK not in ran0, ran0
    for k in (1, 2, 3, 4):
        n = f"{name}_conv{k}"
        assert torch.equal(fused[n], plain[n]), n
        assert np.array_equal(fused[n].cpu().numpy().astype(np.float64), feats[k]), n


# ------------------------------------------------------------------------------------------------ 4. independence
# (13 x 48 still fits the resident kernel: mode 2 there)
@pytest.mark.parametrize("shape,mode", [((4, 13, 48), 2), ((2, 48, 48), 1)], ids=["4x13x48-mode2", "2x48x48-mode1"])
def test_an_image_does_not_depend_on_bands_batch_workgroup_taps_or_history(fused_ctx, shape, mode):
    ctx = fused_ctx
    B, H, W = shape
    m, _ = model_of(ctx, "random", mode)
    xd = ctx.to_device(images(shape, 61 + H), torch.bfloat16)
    small = ctx.to_device(images((2, 9, 31), 62), torch.bfloat16)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    y0, ran = profiled(ctx, lambda: m.forward(xd))                            # automatic bands
    assert STREAM in ran and BLOCK not in ran, ran
    assert bool(torch.isfinite(y0.float()).all())
    for bands in (1, 2, 3, 13):                                               # 13 at H = 13: every row on a seam, every band shorter than its halo
        ctx.set_block_stream_bands(bands)
        assert torch.equal(m.forward(xd), y0), bands
        ctx.set_fused(ctx.FUSED_ALL, 1)                                       # one workgroup runs every band of every image
        assert torch.equal(m.forward(xd), y0), bands
        ctx.set_fused(ctx.FUSED_ALL, 0)
    ctx.set_block_stream_bands(0)
    ctx.set_fused(ctx.FUSED_ALL, 1)
    assert torch.equal(m.forward(xd), y0)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    for i in range(B):
        assert torch.equal(m.forward(xd[i:i + 1]), y0[i:i + 1]), i
    yt, _ = m.forward_with_taps(xd, ALL_TAPS)
    assert torch.equal(yt, y0)
    ctx.set_block_stream_bands(3)                                             # growth slices are stored by the band that owns the row
    yt3, t3 = m.forward_with_taps(xd, GROWTH_TAPS)
    ctx.set_block_stream_bands(1)
    yt1, t1 = m.forward_with_taps(xd, GROWTH_TAPS)
    ctx.set_block_stream_bands(0)
    assert torch.equal(yt3, y0) and torch.equal(yt1, y0)
    for n in GROWTH_TAPS:
        assert torch.equal(t3[n], t1[n]), n
    yt4, _ = m.forward_with_taps(xd, ["rrdb_0_dense2_conv4"])
    assert torch.equal(yt4, y0)
    m.forward(small)                                                          # another shape in between: another ring over the same bytes
    assert torch.equal(m.forward(xd), y0)
    nan = torch.full_like(xd, float("nan"))
    m.forward(nan)                                                            # fills every ring with NaNs
    assert torch.equal(m.forward(xd), y0)


# ------------------------------------------------------------------------------------------------ 5. fallbacks
def test_mode_0_runs_what_a_model_without_the_option_runs(fused_ctx):
    ctx = fused_ctx
    xd = ctx.to_device(images((2, 48, 48), 71), torch.bfloat16)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    never, _ = model_of(ctx, "random", None)
    y_never, ran_never = profiled(ctx, lambda: never.forward(xd))
    m, _ = model_of(ctx, "random", 1)
    y1, ran1 = profiled(ctx, lambda: m.forward(xd))
    assert STREAM in ran1, ran1
    m, _ = model_of(ctx, "random", 0)
    y, ran = profiled(ctx, lambda: m.forward(xd))
    assert STREAM not in ran and STREAM not in ran_never and ran == ran_never, (ran, ran_never)
    assert torch.equal(y, y_never)


def test_mode_1_beyond_the_ring_runs_layer_by_layer(fused_ctx):
    ctx = fused_ctx
    W = widest() + 1
    assert ring(W) == -1
    m, w = model_of(ctx, "random", 1)
    H = 9
    assert Context.dense_block_lds_bytes(G, H, W) == -1                       # too large for the resident kernel as well
    x = images((1, H, W), 72)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    y, ran = profiled(ctx, lambda: m.forward(ctx.to_device(x, torch.bfloat16)))
    assert STREAM not in ran and BLOCK not in ran, ran
    ref = M.esrgan_g_forward(x, w, 2, NB, dtype=np.float64, attention=False, bf16_storage=True)
    e = D.rel_l2(y.float().cpu().numpy(), ref)
    print(f"REL_L2 fallback beyond the ring {e:.3e}")
    assert e <= 5e-3, e


def test_mode_1_keeps_the_resident_kernel_where_it_fits(fused_ctx):
    ctx = fused_ctx
    m, _ = model_of(ctx, "random", 1)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    _, ran = profiled(ctx, lambda: m.forward(ctx.to_device(images((2, 24, 24), 73), torch.bfloat16)))
    assert BLOCK in ran and STREAM not in ran, ran
    ctx.set_fused(ctx.FUSED_ALL & ~ctx.FUSED_TWO_UP, 0)                       # without the three mask bits neither kernel runs
    _, ran = profiled(ctx, lambda: m.forward(ctx.to_device(images((2, 48, 48), 74), torch.bfloat16)))
    assert BLOCK not in ran and STREAM not in ran, ran


@pytest.mark.parametrize("cfg", [dict(dtype="f32"), dict(growth=32)], ids=["f32", "growth-32"])
def test_the_setter_refuses_models_the_kernel_cannot_serve(fused_ctx, cfg):
    ctx = fused_ctx
    m = Model("esrgan_g", compute_dtype=cfg.get("dtype", "bf16"), scale_factor=2, num_blocks=1, growth_channels=cfg.get("growth", G), use_attention=False, ctx=ctx)
    for mode in (1, 2):
        assert ctx.lib.sr_model_set_dense_block_stream(m.h, mode) == L.SR_ERR_INVALID
        with pytest.raises(ValueError, match="8 growth channels"):
            m.set_dense_block_stream(mode)
    good, _ = model_of(ctx, "random", 0)
    assert ctx.lib.sr_model_set_dense_block_stream(good.h, 3) == L.SR_ERR_INVALID


# ------------------------------------------------------------------------------------------------ 6. whole forwards
def test_whole_forward_against_the_oracle(fused_ctx):
    ctx = fused_ctx
    m, w = model_of(ctx, "random", 1)
    x = images((3, 48, 48), 81)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    y, ran = profiled(ctx, lambda: m.forward(ctx.to_device(x, torch.bfloat16)))
    assert STREAM in ran, ran
    ref = M.esrgan_g_forward(x, w, 2, NB, dtype=np.float64, attention=False, bf16_storage=True)
    e = D.rel_l2(y.float().cpu().numpy(), ref)
    print(f"REL_L2 whole forward {e:.3e}")
    assert e <= 5e-3, e


def test_notebook_configuration_through_the_wrapper(fused_ctx):
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    from sr355.synth import make_pairs
    ctx = fused_ctx
    m = ESRGAN(compute_dtype="bf16", infer_dense_block="stream")
    m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1)      # the notebook's configuration, one RRDB
    w = bf16_rounded(m.weights)
    m.set_weights(w)
    lr, _ = make_pairs(1, 60, 80, 2, seed=9)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    (sr, _), ran = profiled(ctx, lambda: m.super_resolve_image(lr[0]))        # the defaults: patch_size_lr = 48, stride = 24
    assert STREAM in ran, ran
    ref = M.esrgan_super_resolve(lr[0], w, 2, 48, 24, num_rrdb=1, dtype=np.float64)
    assert sr.shape == (120, 160, 3)
    err = float(np.abs(sr - ref).max())
    print(f"MAXABS wrapper {err:.3e}")
    assert err <= 2e-2, err
