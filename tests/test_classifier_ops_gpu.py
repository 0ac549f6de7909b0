"""The kernels around the VGG conv stacks, per element against NumPy in fp64 (oracle.ops / oracle.models): the 2x2 max-pool (scalar kernel, bf16 x8
kernel, the pool in a conv's epilogue, each with and without cell-grid packing), global average pooling, _preprocess_vgg_input and the
Dense + ReLU / softmax head (csrc/imgops.hip, csrc/conv_rows.hip rows_pool2; VGG16_model.py:57-97, ESRGAN_model.py:379-408).

  A. the single ops through sr_spatial_op (fp32): signed data, odd sizes, empty outputs, exact-integer and random GAP, the channel order;
  B. the pools inside the VGG16 / VGG19 graphs, tapped op by op, at input sizes whose feature maps halve odd (MaxPooling2D floors), with the
     pool as its own kernel, in the conv's epilogue, and with block 5 packed into a cell grid;
  C. GAP -> Dense(ReLU) -> Dense(softmax) row by row from the tapped last pool, for 1, 2, 5 and 257 classes and logits beyond ln(FLT_MAX).

Not reachable from the ABI: the bf16 x8 pool kernel (and the pool in the conv epilogue) runs only inside a bf16 model, where its input is the
output of a ReLU, so its handling of negative values cannot be exercised here; the scalar kernel's is (section A, fp32)."""
import numpy as np
import pytest
import torch

from oracle import models as M
from oracle import ops as O
from sr355 import Model
from sr355 import _lib as L
from sr355.weights import bf16_rounded, init_weights, round_to_bf16

from tap_util import forward_tapped, host

pytestmark = pytest.mark.gpu

U = 2.0 ** -24          # unit round-off of fp32


@pytest.fixture(autouse=True)
def restore_fused(ctx):
    yield
    ctx.set_fused(ctx.FUSED_ALL, 0)


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# =====================================================================================================================================
# A. the single ops through sr_spatial_op
# =====================================================================================================================================

def _signed(shape, seed):
    """Signed data whose channel 0 is negative everywhere: every 2x2 window of that channel holds four negative values."""
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    x[..., 0] = -np.abs(x[..., 0]) - 0.5
    return x


# (4, 96, 96, 64): 589 824 outputs; (6, 194, 130, 64): 2 421 120 outputs, more than the 8192 x 256 threads the launch is capped at, so the
# grid-stride loop goes round twice (and 97 x 65 output pixels: odd both ways)
@pytest.mark.parametrize("shape", [(2, 8, 6, 5), (3, 9, 11, 5), (1, 2, 2, 1), (2, 3, 2, 8), (4, 96, 96, 64), (6, 194, 130, 64)])
def test_maxpool2_signed_and_odd(ctx, shape):
    x = _signed(shape, sum(shape))
    ref = O.maxpool2x2(x)
    assert ref.shape == (shape[0], shape[1] // 2, shape[2] // 2, shape[3]) and np.all(ref[..., 0] < 0)
    got = host(ctx.spatial_op(L.SP_MAXPOOL2, ctx.to_device(x)))
    assert got.shape == ref.shape and np.array_equal(got, ref)


@pytest.mark.parametrize("shape", [(1, 1, 4, 3), (1, 4, 1, 3)])
def test_maxpool2_empty_output_is_an_error_and_writes_nothing(ctx, shape):
    x = ctx.to_device(_signed(shape, 5))
    y = torch.full((64,), -7.5, dtype=torch.float32, device=ctx.torch_device)
    rc = ctx.lib.sr_spatial_op(ctx.h, L.SP_MAXPOOL2, x.data_ptr(), *shape, y.data_ptr(), ctx.stream())
    torch.cuda.synchronize()
    assert rc == L.SR_ERR_INVALID and "maxpool" in ctx.lib.sr_last_error(ctx.h).decode()
    assert bool((y == -7.5).all())
    with pytest.raises(ValueError):
        ctx.spatial_op(L.SP_MAXPOOL2, x)


GAP_SHAPES = [(2, 1, 1, 5), (3, 5, 7, 3), (2, 96, 96, 64), (2, 4, 5, 300), (3, 6, 7, 1)]     # HW = 1; odd; 9216 pixels; C > the block's 256 threads; C = 1


@pytest.mark.parametrize("shape", GAP_SHAPES)
def test_gap_exact_integers(ctx, shape):
    """Integers in [-8, 8]: every partial sum is an integer below 2^24, exact in fp32 in any order, so the one rounding left is the quotient's, and a
    correctly rounded fp32 division gives float32(sum / HW) bit for bit.  (The fp64 quotient rounded to fp32 is that value too: sum / HW with HW <
    2^14 is either an fp32 rounding tie exactly or at least 2^-38 relative away from one, far beyond fp64's 2^-53.)  A dropped or double-counted
    pixel changes the sum by an integer."""
    B, H, W, C = shape
    x = np.random.default_rng(H * W + C).integers(-8, 9, shape).astype(np.float32)
    s = x.astype(np.float64).reshape(B, H * W, C).sum(axis=1)
    ref = (s / (H * W)).astype(np.float32)
    got = host(ctx.spatial_op(L.SP_GAP, ctx.to_device(x)))
    assert got.shape == (B, C)
    assert np.array_equal(got, ref), (float(np.abs(got - ref).max()), np.argwhere(got != ref)[:5])


@pytest.mark.parametrize("shape", GAP_SHAPES)
def test_gap_random_within_the_sequential_sum_bound(ctx, shape):
    """Data in [100, 101] (no cancellation, every addition rounds) against fp64.  Bound per output: the first-order bound of a sequential fp32 sum
    of HW terms, HW 2^-24 mean|x|, plus the rounding of the quotient, 2^-24 |mean|, both evaluated in fp64 from the data.
    Measured on an MI355X, worst error / bound over the outputs: 0 at HW = 1, 0.082 at (3, 5, 7, 3), 0.0064 at (2, 96, 96, 64), 0.158 at
    (2, 4, 5, 300), 0.056 at (3, 6, 7, 1)."""
    B, H, W, C = shape
    x = np.random.default_rng(H + W + C).uniform(100.0, 101.0, shape).astype(np.float32)
    xd = x.astype(np.float64).reshape(B, H * W, C)
    ref = xd.mean(axis=1)
    bound = H * W * U * np.abs(xd).mean(axis=1) + U * np.abs(ref)
    got = host(ctx.spatial_op(L.SP_GAP, ctx.to_device(x))).astype(np.float64)
    ratio = float((np.abs(got - ref) / bound).max())
    print(f"gap random {shape}: worst error / bound = {ratio:.4f}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 48, 64, 3)])
def test_vgg_preprocess(ctx, shape):
    """(x + 1) * 127.5 - mean with the channels reversed: at most four fp32 roundings at magnitudes below 256 (the sum, the product, the rounded mean
    constant, the difference), 4 x 2^-17 < 2^-14."""
    x = np.random.default_rng(shape[1]).uniform(-1, 1, shape).astype(np.float32)
    x.reshape(-1, 3)[:3] = np.array([[-1, 0, 1], [0, 1, -1], [1, -1, 0]], np.float32)      # exactly -1, 0 and 1 in every channel
    got = host(ctx.spatial_op(L.SP_VGG_PREPROCESS, ctx.to_device(x)))
    ref = O.vgg19_preprocess(x)
    assert got.shape == ref.shape == shape
    assert np.abs(got - ref).max() <= 2.0 ** -14, float(np.abs(got - ref).max())


def test_vgg_preprocess_channel_order_and_rgb_only(ctx):
    red = np.empty((1, 3, 4, 3), np.float32)
    red[...] = np.array([1.0, -1.0, -1.0], np.float32)          # R = 255, G = B = 0 after the rescaling
    got = host(ctx.spatial_op(L.SP_VGG_PREPROCESS, ctx.to_device(red))).astype(np.float64)
    want = np.array([0.0 - 103.939, 0.0 - 116.779, 255.0 - 123.68])                         # B, G, R
    assert np.abs(got - want).max() <= 2.0 ** -14, got[0, 0, 0]
    with pytest.raises(ValueError, match="RGB"):
        ctx.spatial_op(L.SP_VGG_PREPROCESS, ctx.to_device(np.zeros((1, 3, 4, 4), np.float32)))
    with pytest.raises(ValueError, match="RGB"):
        ctx.spatial_op(L.SP_VGG_PREPROCESS, ctx.to_device(np.zeros((1, 3, 4, 1), np.float32)))


# =====================================================================================================================================
# B. the pools inside the graphs
# =====================================================================================================================================

# height x width of the input: 37 -> 18 -> 9 -> 4 -> 2 rows and 53 -> 26 -> 13 -> 6 -> 3 columns through the five blocks; 50 x 70 halves 25 and
# 35 and runs block 5 at 3 x 4; 33 x 47; 32 x 32 runs block 5 at 2 x 2, the smallest valid; 80 x 112 runs it at 5 x 7
SIZES = [(37, 53), (50, 70), (33, 47), (32, 32), (80, 112)]
BATCHES = [1, 2, 5]             # 5: the cell grid's last row is part-filled
SIZE_IDS = [f"{h}x{w}" for h, w in SIZES]


@pytest.fixture(scope="module")
def base_w():
    return init_weights(M.vgg16_classifier_layers(2), scheme="he_normal", seed=4200)


@pytest.fixture(scope="module")
def vgg_bf16(ctx, base_w):
    m = Model("vgg16", compute_dtype="bf16", num_classes=2, ctx=ctx)
    w = bf16_rounded(base_w)
    m.set_weights(w)
    return m, w


@pytest.fixture(scope="module")
def vgg_f32(ctx, base_w):
    m = Model("vgg16", compute_dtype="f32", num_classes=2, ctx=ctx)
    m.set_weights(base_w)
    return m, base_w


def image_batch(size, batch):
    """[0, 1) pixels that are bf16 values, so that both data types read the same numbers."""
    rng = np.random.default_rng(1000 * size[0] + 10 * size[1] + batch)
    return round_to_bf16(rng.uniform(0, 1, (batch, size[0], size[1], 3)).astype(np.float32))


def pool_ops(m, n_pools):
    """Indices of the graph's max-pool ops, each with a conv in front of it."""
    ops = m.ops()
    idx = [i for i, o in enumerate(ops) if o[0] == "maxpool"]
    assert len(idx) == n_pools
    for k, i in enumerate(idx):
        assert ops[i - 1][0].startswith(f"block{k + 1}_conv") and ops[i - 1][1] == ops[i][1] > 0, (ops[i - 1], ops[i])
    return idx


def kernels_of(ctx, fn):
    ctx.profile_begin()
    y = fn()
    torch.cuda.synchronize()
    return y, {r["kernel"]: r["launches"] for r in ctx.profile_end()}


_plain = {}


def plain_run(m, size, batch):
    """The bf16 classifier layer by layer (fusion mask 0), computed once per size and batch and left unchanged: the probabilities, every pool's
    tapped output, and whether each equals the NumPy floor max-pool of the tapped conv output in front of it."""
    key = (size, batch)
    if key not in _plain:
        ctx = m.ctx
        pools = pool_ops(m, 5)
        ctx.set_fused(0, 0)
        y, taps = forward_tapped(m, ctx.to_device(image_batch(size, batch), torch.bfloat16), pools + [i - 1 for i in pools])
        ctx.set_fused(ctx.FUSED_ALL, 0)
        conv = [host(taps[i - 1]) for i in pools]
        pool = [host(taps[i]) for i in pools]
        h, w = size
        shapes_ok, equal = [], []
        for c, p in zip(conv, pool):
            shapes_ok.append(c.shape[1:3] == (h, w) and p.shape[1:3] == (h // 2, w // 2))
            equal.append(p.shape == O.maxpool2x2(c).shape and np.array_equal(p, O.maxpool2x2(c)))
            h, w = h // 2, w // 2
        _plain[key] = {"y": y.clone(), "pool": pool, "shapes_ok": shapes_ok, "equal": equal,
                       "alive": [bool(np.isfinite(p).all() and (p > 0).any()) for p in pool]}
    return _plain[key]


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_vgg16_bf16_pools_layer_by_layer(ctx, vgg_bf16, size, batch):
    """Both tensors are fp32 copies of bf16 values and a maximum is exact: bit for bit, block by block."""
    r = plain_run(vgg_bf16[0], size, batch)
    assert all(r["shapes_ok"]), r["shapes_ok"]
    assert all(r["alive"]), r["alive"]                      # finite (the NaN the tap buffers started as is gone), and not all zeros
    assert all(r["equal"]), r["equal"]
    assert r["y"].shape == (batch, 2) and bool(torch.isfinite(r["y"].float()).all())


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_vgg16_bf16_pools_in_the_conv_epilogue(ctx, vgg_bf16, size, batch):
    """FUSED_POOL alone, the pools tapped (a tapped conv would opt out of the fusion): the fused kernel is the one that ran, and every pooled
    tensor and the probabilities are the layer-by-layer path's bit for bit."""
    m = vgg_bf16[0]
    r = plain_run(m, size, batch)
    pools = pool_ops(m, 5)
    xd = ctx.to_device(image_batch(size, batch), torch.bfloat16)
    ctx.set_fused(ctx.FUSED_POOL, 0)
    (y, taps), ks = kernels_of(ctx, lambda: forward_tapped(m, xd, pools))
    fused = {k: n for k, n in ks.items() if k.startswith("conv_rows_pool")}
    print(f"fused pools {size} x {batch}: {fused}")
    assert sum(fused.values()) == 5, ks                     # every block ends in a 3x3 conv to 64 couts or more over at least 2 x 2 pixels: all five fuse
    for k, i in enumerate(pools):
        got = host(taps[i])
        assert got.shape == r["pool"][k].shape and np.array_equal(got, r["pool"][k]), (k, float(np.nanmax(np.abs(got - r["pool"][k]))))
    assert torch.equal(y, r["y"])
    y2, ks2 = kernels_of(ctx, lambda: m.forward(xd))        # and without any tap
    assert any(k.startswith("conv_rows_pool") for k in ks2), ks2
    assert torch.equal(y2, r["y"])


def cell_masks(ctx):
    return {"cells": ctx.FUSED_CELLS, "cells+pool": ctx.FUSED_ALL & ~(ctx.FUSED_CONV_STREAM | ctx.FUSED_SRCNN_1X1)}


@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_vgg16_bf16_cell_packing_matches_the_plain_path(ctx, vgg_bf16, size, batch):
    """Any tap switches the cell grid off, so the outputs are compared: block 5 packed (without and with the fused pools) and mask 0 give the same
    probabilities bit for bit."""
    m = vgg_bf16[0]
    want = plain_run(m, size, batch)["y"]
    xd = ctx.to_device(image_batch(size, batch), torch.bfloat16)
    for name, mask in list(cell_masks(ctx).items()) + [("plain", 0)]:
        ctx.set_fused(mask, 0)
        y = m.forward(xd)
        assert torch.equal(y, want), (name, float((y.float() - want.float()).abs().max()))


@pytest.mark.parametrize("mask", ["cells", "cells+pool"])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_vgg16_bf16_cell_packing_small_batch_after_a_larger_one(ctx, vgg_bf16, size, mask):
    """Batch 2 after batch 5 on the same model: stale cells lie beside live ones, at odd cell sizes."""
    m = vgg_bf16[0]
    want5, want2 = plain_run(m, size, 5)["y"], plain_run(m, size, 2)["y"]
    ctx.set_fused(cell_masks(ctx)[mask], 0)
    y5 = m.forward(ctx.to_device(image_batch(size, 5), torch.bfloat16))
    y2 = m.forward(ctx.to_device(image_batch(size, 2), torch.bfloat16))
    assert torch.equal(y5, want5) and torch.equal(y2, want2)


@pytest.mark.parametrize("size", [(37, 53), (50, 70)], ids=["37x53", "50x70"])
def test_vgg16_f32_odd_sizes_against_fp64(ctx, vgg_f32, size):
    m, w = vgg_f32
    x = image_batch(size, 2)
    pools = pool_ops(m, 5)
    y, taps = forward_tapped(m, ctx.to_device(x), pools + [i - 1 for i in pools])
    ref = M.vgg16_classifier_forward(x, w, dtype=np.float64)
    got = host(y)
    assert got.shape == ref.shape == (2, 2)
    assert np.abs(got - ref).max() <= 1e-5, float(np.abs(got - ref).max())
    h, wd = size
    for i in pools:
        c, p = host(taps[i - 1]), host(taps[i])
        assert c.shape[1:3] == (h, wd) and p.shape[1:3] == (h // 2, wd // 2) and np.isfinite(p).all()
        assert np.array_equal(p, O.maxpool2x2(c))
        h, wd = h // 2, wd // 2
    assert torch.equal(m.forward(ctx.to_device(x)), y)      # the taps change nothing


@pytest.fixture(scope="module")
def vgg19(ctx):
    m = Model("vgg19_features", compute_dtype="f32", ctx=ctx)
    w = init_weights(m.layer_shapes(), scheme="he_normal", seed=6100)
    m.set_weights(w)
    return m, w


@pytest.mark.parametrize("shape", [(2, 37, 53, 3), (1, 33, 47, 3)])
def test_vgg19_features_f32_odd_sizes(ctx, vgg19, shape):
    m, w = vgg19
    x = np.random.default_rng(shape[1]).uniform(-1, 1, shape).astype(np.float32)
    ref = M.vgg19_features(O.vgg19_preprocess(x), w, dtype=np.float64)
    pools = pool_ops(m, 4)
    y, taps = forward_tapped(m, ctx.to_device(x), pools + [i - 1 for i in pools])
    got = host(y)
    assert got.shape == ref.shape == (shape[0], shape[1] // 16, shape[2] // 16, 512)
    assert rel_l2(got, ref) <= 2e-5, rel_l2(got, ref)
    for i in pools:
        assert np.array_equal(host(taps[i]), O.maxpool2x2(host(taps[i - 1])))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("size", [(31, 40), (40, 16)], ids=["31x40", "40x16"])
def test_vgg16_images_below_32_pixels_are_refused_cleanly(ctx, vgg_f32, vgg_bf16, size, dtype):
    """A side below 32 pixels leaves block 5's pool nothing to keep: the invalid-argument error, and no packed-layout state left behind -- a forward
    at 32 x 32 on the same model, whose block 5 was packed for a batch of 5 just before, is then correct."""
    m, w = vgg_f32 if dtype == "f32" else vgg_bf16
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    m.forward(ctx.to_device(image_batch((32, 32), 5), td))
    bad = ctx.to_device(image_batch(size, 3), td)
    out = torch.full((3, 2), -7.5, dtype=td, device=ctx.torch_device)
    with pytest.raises(ValueError, match="32"):
        m.forward(bad, out=out)
    torch.cuda.synchronize()
    assert bool((out == -7.5).all())
    x = image_batch((32, 32), 2)
    got = m.forward(ctx.to_device(x, td))
    ref = M.vgg16_classifier_forward(x, w, dtype=np.float64)
    assert np.abs(host(got) - ref).max() <= (1e-5 if dtype == "f32" else 3e-2)
    if dtype == "bf16":
        assert torch.equal(got, plain_run(m, (32, 32), 2)["y"])


# =====================================================================================================================================
# C. GAP -> Dense(ReLU) -> Dense(softmax), per element from the tapped last pool
# =====================================================================================================================================

HEAD_X = (70, 100)          # 70 -> 35 -> 17 -> 8 -> 4 -> 2 rows, 100 -> 50 -> 25 -> 12 -> 6 -> 3 columns: GAP over 2 x 3 pixels
HEAD_B = 3


def head_reference(pool, dense, pred):
    """fp64 GAP -> Dense(ReLU) -> Dense(softmax) of the tapped pool [B, h, w, 512], with a first-order bound on what fp32 arithmetic in that order
    may add: the sequential-sum bound n 2^-24 sum|terms| for the mean (plus the quotient's rounding) and for each dot product (the bias counted
    as one more term), the input's own bound carried through |W|, ReLU being 1-Lipschitz, and |dp| <= 2 p max|dlogit| through the softmax.
    -> (probabilities, logits, per-element bound on the probabilities)."""
    B = pool.shape[0]
    x = pool.astype(np.float64).reshape(B, -1, pool.shape[-1])
    hw = x.shape[1]
    (w1, b1), (w2, b2) = [(np.asarray(k, np.float64), np.asarray(b, np.float64)) for k, b in (dense, pred)]
    g = x.mean(axis=1)
    dg = hw * U * np.abs(x).mean(axis=1) + U * np.abs(g)
    a1 = g @ w1 + b1
    d1 = dg @ np.abs(w1) + (w1.shape[0] + 1) * U * (np.abs(g) @ np.abs(w1) + np.abs(b1))
    h = np.maximum(a1, 0.0)
    z = h @ w2 + b2
    dz = d1 @ np.abs(w2) + (w2.shape[0] + 1) * U * (h @ np.abs(w2) + np.abs(b2))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return p, z, 2.0 * p * dz.max(axis=1, keepdims=True)


_head_pool = {}


def head_pool(model_and_w, dtype):
    """The last pool of the module's classifier for the head cases' input, tapped once per data type (it does not depend on the head)."""
    if dtype not in _head_pool:
        m = model_and_w[0]
        td = torch.float32 if dtype == "f32" else torch.bfloat16
        _, taps = forward_tapped(m, m.ctx.to_device(image_batch(HEAD_X, HEAD_B), td), pool_ops(m, 5)[-1:])
        _head_pool[dtype] = host(next(iter(taps.values())))
    return _head_pool[dtype]


@pytest.mark.parametrize("logits", ["unit", "large"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("nc", [1, 2, 5, 257])
def test_classifier_head_per_element(ctx, vgg_f32, vgg_bf16, nc, dtype, logits):
    """Row by row against fp64 computed from the tapped last pool.  fp32: head_reference's bound + 1e-5 (test_vgg16_classifier_forward's fp32 bound,
    for expf and the division); bf16 compute with bf16 output: + 2^-9 of the value, half a bf16 ulp -- on each probability, and so on a row's sum.
    `large`: the predictions kernel scaled by a power of two until a reference logit exceeds 100 in magnitude (89 > ln(FLT_MAX): expf overflows
    without the max-subtraction).  A dropped term of a 512-term dot product is about 1 / (512^2 2^-24) = 64 times the bound.
    Measured on an MI355X, worst error / tolerance over a case's elements: fp32 at most 1e-4 in every case (worst error 2.0e-7 at unit logits
    against a bound of 8e-4 .. 2e-2; 6.2e-6 at 257 classes with large logits); bf16 output 0.098 / 0.115 / 0.142 at 2 / 5 / 257 classes with
    unit logits (the error is the output's rounding, up to 1.9e-3) and 0.0032 at 257 classes with large logits; 0 for one class.  The
    worst-case bound is loose: at large logits it exceeds 0.5, and what those cases pin is that the probabilities are finite and every row sums to one."""
    base_m, base = vgg_f32 if dtype == "f32" else vgg_bf16
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    rng = np.random.default_rng(7000 + nc)
    k2 = rng.normal(0.0, np.sqrt(2.0 / 256), (256, nc)).astype(np.float32)
    b2 = rng.uniform(-0.05, 0.05, nc).astype(np.float32)
    if dtype == "bf16":
        k2 = round_to_bf16(k2)
    if logits == "large":
        z0 = head_reference(head_pool((base_m, base), dtype), base["dense"], (k2, b2))[1]
        k2 = k2 * np.float32(2.0 ** np.ceil(np.log2(100.0 / np.abs(z0 - b2).max())))
    w = dict(base)
    w["predictions"] = (k2, b2)
    m = Model("vgg16", compute_dtype=dtype, num_classes=nc, ctx=ctx)
    assert m.layer_shapes() == M.vgg16_classifier_layers(nc)
    m.set_weights(w)
    last = pool_ops(m, 5)[-1]
    y, taps = forward_tapped(m, ctx.to_device(image_batch(HEAD_X, HEAD_B), td), [last])
    pool = host(taps[last])
    assert pool.shape == (HEAD_B, 2, 3, 512) and np.array_equal(pool, head_pool((base_m, base), dtype)) and (pool > 0).any()
    p, z, bound = head_reference(pool, w["dense"], w["predictions"])
    if logits == "large":
        assert np.abs(z).max(axis=1).max() > 89.0, float(np.abs(z).max())
    assert y.dtype == td and tuple(y.shape) == (HEAD_B, nc)
    got = host(y).astype(np.float64)
    out_round = 2.0 ** -9 if dtype == "bf16" else 0.0
    assert np.isfinite(got).all()
    assert np.abs(got.sum(axis=1) - 1.0).max() <= 1e-5 + out_round, got.sum(axis=1)
    if nc == 1:
        assert np.array_equal(got, np.ones((HEAD_B, 1)))
    err, tol = np.abs(got - p), bound + 1e-5 + out_round * p
    ratio = float((err / tol).max())
    print(f"head nc={nc} {dtype} {logits}: max|z| = {np.abs(z).max():.2f}, worst error = {err.max():.3e}, largest bound = {bound.max():.3e}, "
          f"worst error / tolerance = {ratio:.4f}")
    assert np.all(err <= tol), (float(err.max()), ratio)
