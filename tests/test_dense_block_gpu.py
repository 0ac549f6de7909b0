"""The LDS-resident dense-block kernel (csrc/dense_block.hip, dense_block_lds<bf16,g8>): a whole dense block of the reference notebook's generator
(8 growth channels) as one kernel per image.

1. every conv of every block per element against an fp64 restatement fed with the DEVICE's own inputs (tests/dense_ref.py): conv1 .. conv4 are all
   tappable on this route (the kernel then also writes its growth slices to memory), so nothing compounds and no allowance is needed;
2. exact small integers: the growth convs' taps equal the layer-by-layer path's bit for bit, and the fp64 integers;
3. an image's result depends neither on the batch, nor on the workgroup that ran it, nor on taps, nor on what the workgroup's LDS held before;
4. everything the route does not take still runs what it ran, and the kernel is absent from its profile;
5. whole forwards against the CPU oracle, through Model and through the ESRGAN wrapper in the notebook's configuration.
The boundary between 3. and 4. is read from sr_dense_block_lds_bytes, not copied."""
import numpy as np
import pytest
import torch

import dense_ref as D
from oracle import models as M
from sr355 import Context, Model
from sr355.weights import bf16_rounded, init_weights

pytestmark = pytest.mark.gpu

BLOCK = "dense_block_lds<bf16,g8>"
TILE_GROWTH = "conv_rows<bf16,k3,kg1,nt2>"            # a dense-block growth conv on the tile kernel
G = 8
NB = 2
# conv5's kernel and bias times 2^K5 for the conv5 check: on plain random weights the skips hide 0.2 * conv5.  2^4 -- except on 1 x 1 images, where eight of
# conv5's nine taps see nothing but border and the conv term is a third of its usual size: the CPU oracle puts median |alpha conv5| / median |skips| at
# 2.7 .. 2.9 over the six blocks of the other cases and at 0.6 for dense3 at 1 x 1 (0.7 with 2^5, 3.3 with 2^6).  The test asserts the condition per block.
K5, K5_ONE_PIXEL = 4, 6


def lds(h, w, g=G):
    return Context.dense_block_lds_bytes(g, h, w)


def widest(h):
    """The largest W the kernel takes at height h."""
    w = 1
    while lds(h, w + 1) > 0:
        w += 1
    assert lds(h, w) > 0 and lds(h, w + 1) == -1
    return w


@pytest.fixture()
def fused_ctx(ctx):
    yield ctx
    ctx.set_fused(ctx.FUSED_ALL, 0)


_MODELS = {}


def model_of(ctx, key, num_blocks=NB, growth=G, dtype="bf16", seed=5100):
    """key 'random': bf16-rounded seeded weights; ('conv5', k): the same with every dense block's conv5 (kernel and bias) times 2^k."""
    k = (key, num_blocks, growth, dtype, seed)
    if k not in _MODELS:
        m = Model("esrgan_g", compute_dtype=dtype, scale_factor=2, num_blocks=num_blocks, growth_channels=growth, use_attention=False, ctx=ctx)
        w = bf16_rounded(init_weights(m.layer_shapes(), seed=seed))
        if key != "random":
            s = np.float32(2.0 ** key[1])
            w = {n: ((kb[0] * s, kb[1] * s) if n.endswith("_conv5") and "_dense" in n else kb) for n, kb in w.items()}
        m.set_weights(w)
        _MODELS[k] = (m, w)
    return _MODELS[k]


def images(shape, seed):
    return D.rbf(np.random.default_rng(seed).uniform(-1, 1, tuple(shape) + (3,))).astype(np.float32)


def profiled(ctx, fn):
    ctx.profile_begin()
    out = fn()
    return out, {r["kernel"] for r in ctx.profile_end()}


def rel_l2(a, b):
    return D.rel_l2(a, b)


# ------------------------------------------------------------------------------------------------ 1. every conv per element
# (B, H, W, workgroup cap); W = None: the largest W sr_dense_block_lds_bytes accepts at that H
CASES = [
    (5, 24, 24, 2),      # the largest patch of the notebook, an odd batch, several images per workgroup
    (3, 1, 1, 0),        # nothing but border
    (4, 13, 21, 3),      # H W not a multiple of 16: a partly filled last tile
    (2, 5, 31, 0),       # W beyond 24
    (2, 31, 5, 0),       # H beyond 24
    (2, 24, None, 0),    # on the edge of the LDS
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_every_conv_per_element(fused_ctx, case):
    ctx = fused_ctx
    B, H, W, cap = case
    if W is None:
        W = widest(H)
    x = images((B, H, W), B * 1000 + H * 10 + W)
    xd = ctx.to_device(x, torch.bfloat16)
    blocks = [f"rrdb_{b}_dense{d}" for b in range(NB) for d in (1, 2, 3)]
    names = ["initial_conv"] + [f"{n}_conv{k}" for n in blocks for k in (1, 2, 3, 4, 5)]
    for key in ("random", ("conv5", K5_ONE_PIXEL if H * W == 1 else K5)):
        m, w = model_of(ctx, key)
        ctx.set_fused(ctx.FUSED_ALL, cap)
        (_, taps), ran = profiled(ctx, lambda: m.forward_with_taps(xd, names))
        assert BLOCK in ran and not any(k.startswith(TILE_GROWTH) for k in ran), ran
        t = {n: v.cpu().numpy().astype(np.float64) for n, v in taps.items()}
        assert t["initial_conv"].shape == (B, H, W, 64) and all(t[f"{n}_conv{k}"].shape == (B, H, W, G) for n in blocks for k in (1, 2, 3, 4))
        for bi, name in enumerate(blocks):
            d = int(name[-1])
            xin = t["initial_conv"] if bi == 0 else t[blocks[bi - 1] + "_conv5"]
            c = [t[f"{name}_conv{k}"] for k in (1, 2, 3, 4)]
            so = None
            if d == 3:                                                        # the RRDB's input: initial_conv or the previous RRDB's output
                so = t["initial_conv"] if bi < 3 else t[blocks[bi - 3] + "_conv5"]
            tag = f"{key} {case} {name}"
            if key == "random":
                feats = [xin]
                for k in (1, 2, 3, 4):
                    worst = D.assert_bf16_close(c[k - 1], D.growth_ref(feats, w, name, k), what=f"{tag}_conv{k}")
                    print(f"RATIO {BLOCK} conv{k} {tag} {worst:.4f}")
                    feats.append(c[k - 1])
            else:
                ref = D.tail_ref(xin, *c, w, name, so)
                ct, sk = D.tail_terms(xin, *c, w, name, so)
                cm, sm = float(np.median(ct)), float(np.median(sk))
                print(f"MEDIANS {tag} |alpha conv5| {cm:.4g} |skips| {sm:.4g}")
                assert cm > sm > 0, (tag, cm, sm)                             # the scaled conv5 stands above the skips: a wrong conv5 cannot hide
                # scale: the tensors grow with the scaled-up block outputs; the absolute term stands for fp32 accumulation, which scales with the data (dense_ref)
                worst = D.assert_bf16_close(t[f"{name}_conv5"], ref, scale=max(1.0, D.rms(ref)), what=f"{tag}_conv5")
                print(f"RATIO {BLOCK} conv5 {tag} {worst:.4f}")


# ------------------------------------------------------------------------------------------------ 2. exact integers
def test_growth_convs_exact_integers(fused_ctx):
    ctx = fused_ctx
    m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=1, growth_channels=G, use_attention=False, ctx=ctx)
    shapes = m.layer_shapes()
    x = np.random.default_rng(D.EXACT_SEED).integers(-1, 2, size=(7, 11, 24, 3)).astype(np.float32)
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
    m.set_weights(w)
    xd = ctx.to_device(x, torch.bfloat16)
    names = [f"{name}_conv{k}" for k in (1, 2, 3, 4)]
    ctx.set_fused(ctx.FUSED_ALL, 0)
    (_, fused), ran = profiled(ctx, lambda: m.forward_with_taps(xd, names))
    assert BLOCK in ran, ran
    ctx.set_fused(0, 0)
    (_, plain), ran0 = profiled(ctx, lambda: m.forward_with_taps(xd, names))
    assert BLOCK not in ran0, ran0
    for k in (1, 2, 3, 4):
        n = f"{name}_conv{k}"
        assert torch.equal(fused[n], plain[n]), n
        assert np.array_equal(fused[n].cpu().numpy().astype(np.float64), feats[k]), n


# ------------------------------------------------------------------------------------------------ 3. independence
def test_an_image_does_not_depend_on_batch_workgroup_taps_or_history(fused_ctx):
    ctx = fused_ctx
    m, _ = model_of(ctx, "random")
    xd = ctx.to_device(images((6, 24, 24), 61), torch.bfloat16)
    small = ctx.to_device(images((2, 9, 9), 62), torch.bfloat16)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    y0, ran = profiled(ctx, lambda: m.forward(xd))
    assert BLOCK in ran, ran
    ctx.set_fused(ctx.FUSED_ALL, 1)                                           # one workgroup runs all six images
    y1 = m.forward(xd)
    assert torch.equal(y1, y0)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    for i in range(6):
        assert torch.equal(m.forward(xd[i:i + 1]), y0[i:i + 1]), i
    names = ["initial_conv"] + [f"rrdb_{b}_dense{d}_conv{k}" for b in range(NB) for d in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
    yt, _ = m.forward_with_taps(xd, names)
    assert torch.equal(yt, y0)
    yt4, _ = m.forward_with_taps(xd, ["rrdb_0_dense2_conv4"])
    assert torch.equal(yt4, y0)
    m.forward(small)                                                          # a smaller image in between: another LDS image over the same bytes
    assert torch.equal(m.forward(xd), y0)


# ------------------------------------------------------------------------------------------------ 4. fallbacks
def fallback_cases():
    tile = Context.FUSED_ALL & ~Context.FUSED_TWO_UP
    return [
        ("first-rejected-width", dict(shape=(2, 24, None)), Context.FUSED_ALL),
        ("48x48", dict(shape=(1, 48, 48)), Context.FUSED_ALL),
        ("without-two-up-bits", dict(shape=(2, 24, 24)), tile),
        ("mask-0", dict(shape=(2, 24, 24)), 0),
        ("f32", dict(shape=(2, 24, 24), dtype="f32"), Context.FUSED_ALL),
        ("growth-16", dict(shape=(2, 24, 24), growth=16), Context.FUSED_ALL),
    ]


@pytest.mark.parametrize("name,cfg,mask", fallback_cases(), ids=[c[0] for c in fallback_cases()])
def test_fallbacks_run_what_they_ran(fused_ctx, name, cfg, mask):
    ctx = fused_ctx
    B, H, W = cfg["shape"]
    if W is None:
        W = widest(H) + 1
        assert lds(H, W) == -1
    growth, dtype = cfg.get("growth", G), cfg.get("dtype", "bf16")
    m, w = model_of(ctx, "random", growth=growth, dtype=dtype)
    x = images((B, H, W), 70 + H + W + growth)
    xd = ctx.to_device(x, torch.float32 if dtype == "f32" else torch.bfloat16)
    ctx.set_fused(mask, 0)
    y, ran = profiled(ctx, lambda: m.forward(xd))
    assert BLOCK not in ran, (name, ran)
    ref = M.esrgan_g_forward(x, w, 2, NB, dtype=np.float64, attention=False, bf16_storage=True)
    e = rel_l2(y.float().cpu().numpy(), ref)
    print(f"REL_L2 fallback {name} {e:.3e}")
    assert e <= 5e-3, (name, e)


# ------------------------------------------------------------------------------------------------ 5. whole forwards
def test_whole_forward_against_the_oracle(fused_ctx):
    ctx = fused_ctx
    m, w = model_of(ctx, "random")
    x = images((3, 24, 24), 81)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    y, ran = profiled(ctx, lambda: m.forward(ctx.to_device(x, torch.bfloat16)))
    assert BLOCK in ran, ran
    ref = M.esrgan_g_forward(x, w, 2, NB, dtype=np.float64, attention=False, bf16_storage=True)
    e = rel_l2(y.float().cpu().numpy(), ref)
    print(f"REL_L2 whole forward {e:.3e}")
    assert e <= 5e-3, e


def test_notebook_configuration_through_the_wrapper(fused_ctx):
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    from sr355.synth import make_pairs
    ctx = fused_ctx
    m = ESRGAN(compute_dtype="bf16")
    m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1)      # the notebook's configuration, one RRDB
    w = bf16_rounded(m.weights)
    m.set_weights(w)
    lr, _ = make_pairs(1, 30, 40, 2, seed=9)
    ctx.set_fused(ctx.FUSED_ALL, 0)
    (sr, _), ran = profiled(ctx, lambda: m.super_resolve_image(lr[0], patch_size_lr=24, stride=12))
    assert BLOCK in ran, ran
    ref = M.esrgan_super_resolve(lr[0], w, 2, 24, 12, num_rrdb=1, dtype=np.float64)
    assert sr.shape == (60, 80, 3)
    err = float(np.abs(sr - ref).max())
    print(f"MAXABS wrapper {err:.3e}")
    assert err <= 2e-2, err
