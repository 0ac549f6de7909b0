"""Every capped 1-D launch grid of csrc/ past its cap, element by element.

The host clamps these grids (grid_for, grid_n, cls_grid, met_grid, an inline std::min) and a grid-stride loop in the kernel covers the
rest; the other per-element tests stop at sizes where that loop's body runs once.  Each case here (tests/grid_caps.py) is the smallest
input whose thread count exceeds the cap, raggedly, so the loop goes round a second, shorter time.  Every op keeps the contract its
own per-element test states -- the helpers that state it are imported from those tests, not restated.  Outputs are written into
poisoned buffers where the entry point takes one; a failure names the first mismatching flat index and the round it belongs to.
"""
import functools

import numpy as np
import pytest
import torch

import classic_ref as CR
import crop_ref as CROP
import grid_caps as G
import metrics_ref as MR
import patch_dataset_ref as PR
import study_ref as SR
import test_backward_kernels_gpu as BK
import test_classic_gpu as CL
import test_image_ops_gpu as IO
import test_vgg_fit_device_gpu as VF
from oracle import ops as O
from sr355 import _lib as L
from sr355 import train as T

pytestmark = pytest.mark.gpu

Guarded = IO.Guarded


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def fail_at_first(case, bad, what, per_row=None):
    """bad: per-element mismatch flags in output order.  per_row: elements of one grid row (blockIdx.y) where the cap holds per row."""
    bad = np.asarray(bad).reshape(-1)
    if not bad.any():
        return
    i = int(np.argmax(bad))
    per_round = case.cap * case.per_thread
    j = i if per_row is None else i % per_row
    rounds = sorted({int(r) for r in (np.flatnonzero(bad) if per_row is None else np.flatnonzero(bad) % per_row) // per_round})
    pytest.fail(f"{case.id}, {what}: {int(bad.sum())} of {bad.size} elements differ; the first at flat index {i}"
                + ("" if per_row is None else f" (element {j} of its grid row)") + f", round {j // per_round} = index // {per_round}; rounds hit: {rounds}")


def assert_guard(gb, case, what):
    """The guard bytes are intact.  Elements never stored keep their NaN poison, which no comparison below takes for a result: it names them."""
    assert gb.untouched(), f"{case.id}, {what}: stores outside the output"


def guarded_copy(ctx, a, dtype):
    """A host array inside a Guarded buffer (for in-place kernels)."""
    gb = Guarded(ctx, a.size, dtype)
    gb.y.copy_(ctx.to_device(np.ascontiguousarray(a).reshape(-1)))
    return gb


# ================================================================================================ train_ops.hip
def test_adam_past_the_grid_cap(ctx):
    """Two steps on a bucket of cap + 257 floats, the second with grad_scale = 0.5: weights and both moments bit for bit sr355.train.Adam."""
    case = G.BY_ID["adam"]
    n = case.arg
    rng = np.random.default_rng(16)
    w0 = rng.standard_normal(n).astype(np.float32)
    split = lambda a: {"a": (a[:n - 257], a[n - 257:])}
    join = lambda d: np.concatenate([d["a"][0], d["a"][1]])
    ref = T.Adam(split(w0), 1e-4, epsilon=1e-7)
    wh = split(w0)

    class Opt:
        t, lr, b1, b2 = 0, 1e-4, 0.9, 0.999
    gw, gm, gv = guarded_copy(ctx, w0, "f32"), guarded_copy(ctx, np.zeros(n, np.float32), "f32"), guarded_copy(ctx, np.zeros(n, np.float32), "f32")
    for step, scale in enumerate((1.0, 0.5)):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 2, n)).astype(np.float32)
        wh = ref.apply(wh, split(g * np.float32(scale)))
        gd = ctx.to_device(g)                                              # held until the results are read: the launch is asynchronous
        ctx.adam_step(gw.y, gd, gm.y, gv.y, T._next_lr_t(Opt), 0.9, 0.999, 1e-7, grad_scale=scale)
        for name, gb, want in (("w", gw, join(wh)), ("m", gm, np.concatenate(ref.m["a"])), ("v", gv, np.concatenate(ref.v["a"]))):
            assert gb.untouched(), f"adam step {step}: stores outside {name}"
            fail_at_first(case, bits(host(gb.y)) != bits(want), f"{name} after step {step}")


@functools.lru_cache(maxsize=None)
def _elt_operands(n):
    """test_eltwise_boundary_operands' operand mix (all pairs of the boundary values, then random ones), tiled to n elements."""
    a, b = BK._boundary_operands(np.random.default_rng(77))
    assert n % len(a) != 0
    return np.resize(a, n), np.resize(b, n)                                # shared by the sixteen cases, which only read them


def _check_elt_rounds(case, op, a, b, got, what):
    """The contract of test_backward_kernels_gpu._check_elt on every element.  The operands repeat with the period of the boundary mix
    and the kernel treats every element alike, so the result repeats bit for bit too: that names the index when the contract fails."""
    period = len(BK._boundary_operands(np.random.default_rng(77))[0])
    fail_at_first(case, bits(got) != bits(np.resize(got[:period], got.size)), what + " (against the same operands of round 0)")
    BK._check_elt(op, a, b, got)


@pytest.mark.parametrize("op", BK.OPS)
def test_eltwise_past_the_grid_cap(ctx, op):
    case = G.BY_ID["eltwise"]
    a, b = _elt_operands(case.arg)
    two = op != L.ELT_CLIP01
    ad, bd = ctx.to_device(a), (ctx.to_device(b) if two else None)
    gb = Guarded(ctx, a.size, "f32")
    ctx.check(ctx.lib.sr_eltwise(ctx.h, int(op), ad.data_ptr(), bd.data_ptr() if two else None, float(BK.ALPHA), float(BK.BETA), gb.y.data_ptr(), a.size,
                                 ctx.stream()))
    assert_guard(gb, case, f"op {op}")
    _check_elt_rounds(case, op, a, b if two else np.zeros_like(b), host(gb.y), f"op {op}")


@pytest.mark.parametrize("op", BK.OPS)
def test_eltwise_view_past_the_grid_cap(ctx, op):
    """npix x 32 channels at channel offsets 5, 9 and 3 of buffers of 40, 48 and 36 channels; the output's other channels keep their sentinel."""
    case = G.BY_ID["eltwise_view"]
    npix, C = case.arg
    ca, cb, co = G.VIEW_BUFS
    a, b = _elt_operands(npix * C)
    shape = (1, 1, npix)
    ad = torch.full(shape + (ca,), 3.5, device=ctx.torch_device)
    bd = torch.full(shape + (cb,), -2.5, device=ctx.torch_device)
    od = torch.full(shape + (co,), -7.75, device=ctx.torch_device)
    ad[..., 5:5 + C] = ctx.to_device(a).view(shape + (C,))
    bd[..., 9:9 + C] = ctx.to_device(b).view(shape + (C,))
    two = op != L.ELT_CLIP01
    ctx.eltwise_view(op, ad, 5, bd if two else None, 9, od, 3, C, float(BK.ALPHA), float(BK.BETA))
    out = host(od)
    assert np.all(out[..., :3] == -7.75) and np.all(out[..., 3 + C:] == -7.75), "channels outside the view were written"
    _check_elt_rounds(case, op, a, b if two else np.zeros_like(b), np.ascontiguousarray(out[..., 3:3 + C]).reshape(-1), f"op {op}")


def test_space_to_depth_past_the_grid_cap(ctx):
    case = G.BY_ID["space_to_depth"]
    B, Hr, Wr, Cx = case.arg
    r = G.S2D_R
    want = np.random.default_rng(5).standard_normal((B, Hr // r, Wr // r, r * r * Cx)).astype(np.float32)
    x = O.depth_to_space(want, r)
    assert x.shape == case.arg and want.size == case.threads
    gb = Guarded(ctx, want.size, "f32")
    xd = ctx.to_device(x)                                                  # held until the result is read: the launch is asynchronous
    ctx.check(ctx.lib.sr_space_to_depth(ctx.h, xd.data_ptr(), B, Hr // r, Wr // r, Cx, r, gb.y.data_ptr(), ctx.stream()))
    assert_guard(gb, case, "y")
    fail_at_first(case, bits(host(gb.y)) != bits(want.reshape(-1)), "the exact inverse of depth_to_space")


def test_maxpool2_bwd_past_the_grid_cap(ctx):
    """Post-ReLU small integers (ties and all-zero windows everywhere, +0 and -0) on 4097 x 4096: the gradient goes to the first maximum in
    row-major order, the odd last row gets zero."""
    case = G.BY_ID["maxpool2_bwd"]
    shape = case.arg
    B, H, W, Cx = shape
    rng = np.random.default_rng(H * W)
    x = np.maximum(BK.ints(rng, shape, -2, 1), 0)
    x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, np.float32(0), np.float32(-0.0))
    dy = rng.standard_normal((B, H // 2, W // 2, Cx)).astype(np.float32)
    gb = Guarded(ctx, x.size, "f32")
    xd, dyd = ctx.to_device(x), ctx.to_device(dy)                          # named: a temporary dies before the next argument's upload, which takes its memory
    ctx.check(ctx.lib.sr_maxpool2_bwd(ctx.h, xd.data_ptr(), dyd.data_ptr(), B, H, W, Cx, gb.y.data_ptr(), ctx.stream()))
    assert_guard(gb, case, "dx")
    got = host(gb.y).reshape(shape)
    fail_at_first(case, got.astype(np.float64) != BK._maxpool_bwd_ref(x, dy), "dx")
    assert not np.any(got[:, -1])


def test_zero_insert2_past_the_grid_cap(ctx):
    case = G.BY_ID["zero_insert2"]
    B, H, W, Cx = case.arg
    ys, xs = BK._tf_stride2_centres(H), BK._tf_stride2_centres(W)
    g = np.random.default_rng(H + W).standard_normal((B, len(ys), len(xs), Cx)).astype(np.float32)
    want = np.zeros(case.arg, np.float32)
    want[:, ys[:, None], xs[None, :]] = g
    gb = Guarded(ctx, want.size, "f32")
    gd = ctx.to_device(g)                                                  # held until the result is read: the launch is asynchronous
    ctx.check(ctx.lib.sr_zero_insert2(ctx.h, gd.data_ptr(), B, H, W, Cx, gb.y.data_ptr(), ctx.stream()))
    assert_guard(gb, case, "out")
    fail_at_first(case, bits(host(gb.y)) != bits(want.reshape(-1)), "out")


# ================================================================================================ imgops.hip
def _resize_input(cid, dtype, shape):
    rng = np.random.default_rng(sum(ord(c) for c in cid))
    return rng.uniform(0, 1, shape).astype(np.float32) if dtype == "f32" else rng.integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("cid", [c[0] for c in G.RESIZE_CASES])
def test_resize_past_the_grid_cap(ctx, cid):
    """837 x 836 x 3 outputs: fp32 within 2e-6 of the oracle, uint8 bit for bit (the contracts of test_resize_per_element)."""
    case = G.BY_ID["resize_" + cid]
    dtype, shape, out, interp = case.arg
    x = _resize_input(cid, dtype, shape)
    got, untouched, written = IO.raw_resize(ctx, x, out, interp)
    assert untouched, "stores outside the output"
    if dtype == "f32":
        ref = O.cv_resize(x, out[0], out[1], interp)
        fail_at_first(case, ~(np.abs(got - ref) <= 2e-6), f"max |got - ref| = {np.nanmax(np.abs(got - ref)):.3e}")      # a NaN left in place counts
    else:
        fail_at_first(case, got != IO.u8_reference(x, out, interp), "uint8")
    assert written, "output elements never stored"


@pytest.mark.parametrize("cid", [c[0] for c in G.BICUBIC_CASES])
def test_bicubic_past_the_grid_cap(ctx, cid):
    """The per-pixel fp32 kernel and the uint8 kernel count output pixels: three images of 837 x 836.
    First run on an MI355X: the uint8 cases differed in 148 and 451 bytes, in round 0 -- a cubic weight one ulp off (fma contraction) rounds
    to another 11-bit integer at one output position in 837; bicubic_u8_kernel now rounds every operation of the weights on its own."""
    case = G.BY_ID["bicubic_" + cid]
    dtype, shape, out = case.arg
    if dtype == "f32":
        assert IO.T.bicubic_route(dtype, shape, out).kernel == "pixel"
    x = _resize_input(cid, dtype, shape)
    got, untouched, written = IO.raw_resize(ctx, x, out)
    assert untouched, "stores outside the output"
    if dtype == "f32":
        ref = O.bicubic_resize(x, out[0], out[1], dtype=np.float64)
        fail_at_first(case, ~(np.abs(got - ref) <= 2e-6), f"max |got - fp64| = {np.nanmax(np.abs(got - ref)):.3e}")
    else:
        fail_at_first(case, got != IO.u8_reference(x, out, None), "uint8")
    assert written, "output elements never stored"


def test_extract_patches_past_the_grid_cap(ctx):
    """bf16 and fp32 out, img * 2 - 1, reflect padding bottom and right: bit for bit (test_extract_patches_bf16_out's contract)."""
    case = G.BY_ID["extract_patches"]
    hw, p, s = case.arg
    img = np.random.default_rng(hw[0]).uniform(0, 1, (*hw, 3)).astype(np.float32)
    val = img * np.float32(2.0) + np.float32(-1.0)
    for out_dtype, v in (("bf16", O.round_bf16(val)), ("f32", val)):
        got, untouched, written = IO._raw_extract(ctx, img, p, s, 2.0, -1.0, out_dtype)
        assert untouched, out_dtype
        ref = O.extract_patches(O.add_padding(v, p, s), p, s)[0]
        assert got.shape == ref.shape and got.size == case.threads
        fail_at_first(case, bits(got) != bits(ref), out_dtype)
        assert written, out_dtype


@pytest.mark.parametrize("scale", sorted(G.OVERLAP_HW))
def test_overlap_add_past_the_grid_cap(ctx, scale):
    """Exact k/64 patches (bit for bit, from bf16 and fp32) and random bf16 patches beyond the clip on both sides (1e-6 of fp64)."""
    case = G.BY_ID[f"overlap_add_x{scale}"]
    hw, p, s, _ = case.arg
    n = ctx.num_patches(hw[0], hw[1], 3, p, s)
    padded = (hw[0] + O.pad_amount(hw[0], p, s), hw[1] + O.pad_amount(hw[1], p, s))
    pos = O.patch_positions(padded[0], padded[1], p, s)
    assert len(pos) == n
    rng = np.random.default_rng(hw[1] + 11 * scale)
    exact = (rng.integers(-96, 97, (n, p * scale, p * scale, 3)) / 64.0).astype(np.float32)
    ref64 = O.overlap_add(exact.astype(np.float64) * 0.5 + 0.5, pos, padded, hw, p, scale, dtype=np.float64)
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64) and ref.size == case.threads
    for in_dtype in ("bf16", "f32"):
        got, untouched, written = IO._raw_overlap_add(ctx, exact, in_dtype, hw, p, s, scale, 0.5, 0.5)
        assert untouched, in_dtype
        fail_at_first(case, bits(got) != bits(ref), f"exact patches from {in_dtype}")
        assert written, in_dtype
    rnd = O.round_bf16(rng.uniform(-1.4, 1.4, exact.shape).astype(np.float32))
    ref = O.overlap_add(rnd.astype(np.float64) * 0.5 + 0.5, pos, padded, hw, p, scale, dtype=np.float64)
    got, untouched, written = IO._raw_overlap_add(ctx, rnd, "bf16", hw, p, s, scale, 0.5, 0.5)
    assert untouched
    fail_at_first(case, ~(np.abs(got - ref) <= 1e-6), "random bf16 patches")
    assert written


def test_pick2_past_the_grid_cap(ctx):
    """SP_PICK2 on 1025 x 1025 x 8: the window centres of a stride-2 SAME conv, an exact gather."""
    case = G.BY_ID["pick2"]
    B, H, W, Cx = case.arg
    z = np.random.default_rng(H).standard_normal(case.arg).astype(np.float32)
    ys, xs = BK._tf_stride2_centres(H), BK._tf_stride2_centres(W)
    want = z[:, ys][:, :, xs]
    assert want.size == case.threads
    gb = Guarded(ctx, want.size, "f32")
    zd = ctx.to_device(z)                                                  # held until the result is read: the launch is asynchronous
    ctx.check(ctx.lib.sr_spatial_op(ctx.h, L.SP_PICK2, zd.data_ptr(), B, H, W, Cx, gb.y.data_ptr(), ctx.stream()))
    assert_guard(gb, case, "y")
    fail_at_first(case, bits(host(gb.y)) != bits(want.reshape(-1)), "the gather")


def test_vgg_preprocess_past_the_grid_cap(ctx):
    """SP_VGG_PREPROCESS on 837 x 836 x 3: within 2^-14 of the fp64 expression (test_vgg_preprocess's bound: four fp32 roundings below 256)."""
    case = G.BY_ID["vgg_preprocess"]
    B, H, W, Cx = case.arg
    x = np.random.default_rng(W).uniform(-1, 1, case.arg).astype(np.float32)
    gb = Guarded(ctx, x.size, "f32")
    xd = ctx.to_device(x)                                                  # held until the result is read: the launch is asynchronous
    ctx.check(ctx.lib.sr_spatial_op(ctx.h, L.SP_VGG_PREPROCESS, xd.data_ptr(), B, H, W, Cx, gb.y.data_ptr(), ctx.stream()))
    assert_guard(gb, case, "y")
    ref = O.vgg19_preprocess(x.astype(np.float64))
    fail_at_first(case, ~(np.abs(host(gb.y).reshape(case.arg) - ref) <= 2.0 ** -14), "against fp64")


def test_conv_input_padding_past_the_grid_cap(ctx):
    """A thin fp32 conv (3 -> 8 channels) on 725 x 725: sr_conv2d_dev pads the input to four channels per pixel first, 2 102 500 elements
    by convert_pad_kernel.  rel-L2 <= 1e-5 of the fp64 oracle (test_conv_routes_gpu.py's fp32 contract) on the whole output and on
    the part of the last output row whose windows hold pixels of the loop's second round alone."""
    case = G.BY_ID["convert_pad"]
    B, H, W, Cx = case.arg
    rng = np.random.default_rng(725)
    x = rng.standard_normal(case.arg).astype(np.float32)
    k = (rng.standard_normal((3, 3, Cx, 8)) / np.sqrt(27)).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, 8).astype(np.float32)
    got = host(ctx.conv2d_dev(ctx.to_device(x), ctx.to_device(k), ctx.to_device(b), 8))
    ref = O.conv2d(x, k, b, dtype=np.float64)
    assert BK.rel_l2(got, ref) <= 1e-5
    row, col = divmod(case.cap // 4, W)                                    # the first pixel the second round pads
    assert row == H - 2 and col + 2 < W // 2
    tail = (slice(None), slice(H - 1, H), slice(col + 2, W))               # outputs whose 3 x 3 windows hold second-round pixels only
    assert BK.rel_l2(got[tail], ref[tail]) <= 1e-5, f"the last output row from column {col + 2}: its input is round 1 of the padding"


def test_l1_past_the_grid_cap(ctx):
    """mean |a - b| over 812 700 elements against 1024 x 256 threads; within 1e-6 of fp64 (test_pixel_and_spectral_loss's bound)."""
    case = G.BY_ID["l1"]
    rng = np.random.default_rng(8)
    a = rng.uniform(-1, 1, case.arg).astype(np.float32)
    b = np.clip(a + 0.1 * rng.standard_normal(case.arg), -1, 1).astype(np.float32)
    b[-1] = a[-1]                                                          # the last image adds nothing ...
    b[-1, -40:] = -a[-1, -40:]                                             # ... except in its last rows: the tail of the last round
    ref = O.pixel_loss(a, b)
    got = float(ctx.l1(ctx.to_device(a), ctx.to_device(b)).item())
    print(f"l1: got {got!r}, fp64 {ref!r}")
    assert abs(got - ref) <= 1e-6, (got, ref)


def test_vgg16_bf16_pool_and_taps_past_the_grid_cap(ctx):
    """VGG16 in bf16 on one 1027 x 1026 image, layer by layer.  The input conversion's tap is the image itself (convert_pad_kernel and
    tap_copy_kernel, both several rounds); block 1's pool, eight channels per thread, is the floor max-pool of the tapped conv in front
    of it bit for bit, as in test_vgg16_bf16_pools_layer_by_layer.  The taps start out as NaN."""
    import test_classifier_ops_gpu as CO
    case = G.BY_ID["maxpool2_bf16x8"]
    m = CO.Model("vgg16", compute_dtype="bf16", num_classes=2, ctx=ctx)
    m.set_weights(CO.bf16_rounded(CO.init_weights(CO.M.vgg16_classifier_layers(2), scheme="he_normal", seed=4200)))
    pool1 = CO.pool_ops(m, 5)[0]
    ops = m.ops()
    assert ops[0][0] == "convert"
    x = CO.round_to_bf16(np.random.default_rng(1027).uniform(0, 1, case.arg).astype(np.float32))
    ctx.set_fused(0, 0)
    try:
        _, taps = CO.forward_tapped(m, ctx.to_device(x, torch.bfloat16), [0, pool1 - 1, pool1])
    finally:
        ctx.set_fused(ctx.FUSED_ALL, 0)
    m.release_workspace()
    t0 = host(taps[0])
    assert t0.shape[:3] == x.shape[:3] and t0.shape[3] >= 3
    fail_at_first(G.BY_ID["tap_copy"], np.ascontiguousarray(t0[..., :3]) != x, "the tapped input conversion against the image")
    assert not np.any(t0[..., 3:])
    conv, pool = host(taps[pool1 - 1]), host(taps[pool1])
    assert conv.shape == (1, 1027, 1026, 64) and pool.shape == (1, 513, 513, 64) and pool.size == case.threads * case.per_thread
    assert np.isfinite(conv).all() and (conv > 0).any()
    fail_at_first(case, bits(pool) != bits(O.maxpool2x2(conv)), "block 1's pool against the tapped conv")


@pytest.mark.parametrize("layout", sorted(G.ESRGAN_CASES))
def test_esrgan_bf16_layout_moves_past_the_grid_cap(ctx, layout):
    """The generator (one RRDB) in bf16 on a batch whose trunk has more than 8 x 2 097 152 values, in each layout of the dense blocks'
    buffers: the batch's output equals, bit for bit, the outputs of its chunks of 64 images, whose layout moves stay below the cap."""
    case = G.BY_ID["esrgan_" + layout]
    B, H, W = case.arg
    from sr355 import Model
    from sr355.weights import bf16_rounded, init_weights, round_to_bf16
    m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=1, growth_channels=32, use_attention=False, ctx=ctx)
    m.set_weights(bf16_rounded(init_weights(m.layer_shapes(), seed=3400)))
    x = round_to_bf16(np.random.default_rng(B + H).uniform(-1, 1, (B, H, W, 3)).astype(np.float32))
    xd = ctx.to_device(x, torch.bfloat16)
    ctx.set_fused(ctx.FUSED_ALL if layout == "two_up" else 0, 0)
    try:
        y = m.forward(xd).clone()
        chunks = torch.cat([m.forward(xd[i:i + 64].contiguous()).clone() for i in range(0, B, 64)])
    finally:
        ctx.set_fused(ctx.FUSED_ALL, 0)
    assert 64 * H * W * 8 < case.cap and tuple(y.shape) == (B, 2 * H, 2 * W, 3)
    yb, cb = host(y.view(torch.int16)), host(chunks.view(torch.int16))
    assert np.isfinite(host(y.float())).all()
    bad = (yb != cb).reshape(B, -1).any(1)
    # an image's output depends on that image's values alone; its trunk is elements [8 * 8 H W b, 8 * 8 H W (b + 1)) of the move
    assert not bad.any(), f"{case.id}: images {np.flatnonzero(bad)[:8]} .. differ from their chunk's; round = image * {H * W * 8} // {case.cap}"


# ================================================================================================ study.hip
@pytest.mark.parametrize("in_u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("route", ["quad", "scalar"])
def test_extract_patches_batch_past_the_grid_cap(ctx, route, in_u8):
    """Both kernels of sr_extract_patches_batch, uint8 and fp32 frames, against the NumPy reference frame by frame, bit for bit."""
    case = G.BY_ID["extract_batch_" + route]
    (F, H, W, Cn), p, s = case.arg
    assert (p * Cn % 4 == 0) == (route == "quad")
    rng = np.random.default_rng(H + p)
    frames = rng.integers(0, 256, (F, H, W, Cn)).astype(np.uint8) if in_u8 else rng.random((F, H, W, Cn)).astype(np.float32)
    got = ctx.extract_patches_batch(ctx.to_device(frames), p, s)
    ref = np.concatenate([SR.patches_ref(frames[f], p, s) for f in range(F)])
    assert tuple(got.shape) == ref.shape and ref.size == case.threads * case.per_thread
    fail_at_first(case, bits(host(got)) != bits(ref), "fp32 out")
    got = ctx.extract_patches_batch(ctx.to_device(frames), p, s, mul=2.0, add=-1.0, out_dtype=torch.bfloat16)
    ref16 = O.round_bf16(ref * np.float32(2.0) + np.float32(-1.0))
    fail_at_first(case, bits(host(got.float())) != bits(ref16), "bf16 out")


# ================================================================================================ patch_dataset.hip
def test_gather_patch_pairs_past_the_grid_cap(ctx):
    """228 pairs of 24 / 96: 2 232 576 pixels in one launch, uint8 stacks with reflect padding, against patch_dataset_ref.gather_side."""
    case = G.BY_ID["gather_patch_pairs"]
    B, patch, scale = case.arg
    rng = np.random.default_rng(228)
    N, h, w, pad = 5, 50, 61, (7, 11)
    lr = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    hr = rng.integers(0, 256, (N, h * scale, w * scale, 3), dtype=np.uint8)
    nwin = 300
    table = np.stack([rng.integers(0, N, nwin), rng.integers(0, h + pad[0] - patch + 1, nwin), rng.integers(0, w + pad[1] - patch + 1, nwin)], 1).astype(np.int32)
    table[:3, 1:] = (h + pad[0] - patch, w + pad[1] - patch)                 # the last window: reflected rows and columns
    order = rng.permutation(nwin).astype(np.int32)
    order[7] = 0
    off = 5
    hr_pad = (pad[0] * scale, pad[1] * scale)
    X, Y = ctx.gather_patch_pairs(dict(stack=ctx.to_device(lr), pad=pad, mul=2.0, add=-1.0), dict(stack=ctx.to_device(hr), pad=hr_pad, swap=True),
                                  ctx.to_device(table), ctx.to_device(order), off, B, patch, scale)
    rows = order[off:off + B]
    Xr = PR.gather_side(lr, table, rows, pad, patch, 1, False, 2.0, -1.0)
    Yr = PR.gather_side(hr, table, rows, hr_pad, patch * scale, scale, True)
    assert (Xr.size + Yr.size) == case.threads * 3
    # the launch numbers the LR pixels first, then the HR ones
    fail_at_first(case, np.concatenate([(bits(host(X)) != bits(Xr)).reshape(-1), (bits(host(Y)) != bits(Yr)).reshape(-1)]), "LR batch, then HR batch")


def test_gather_warp_patches_past_the_grid_cap(ctx):
    """One 513 x 512 patch per element: the identity gives the patch's own bits, the rotated, mirrored element is affine_warp of that
    patch bit for bit (affine_warp itself, below its own cap at this size, within 2e-5 of scipy)."""
    case = G.BY_ID["gather_warp_patches"]
    B, ph, pw = case.arg
    rng = np.random.default_rng(513)
    N, H, W = 2, ph + 3, pw + 5
    stack = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    table = np.array([[1, 2, 4], [0, 3, 1]], np.int32)
    order = np.array([1, 0, 1], np.int32)
    th = np.deg2rad(17.0)
    rot = np.stack([np.eye(2), np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])])
    off = np.array([[0.0, 0.0], [30.25, -41.5]])
    flip = np.array([False, True])
    params = ctx.warp_params(rot, off, flip)
    gb = Guarded(ctx, B * ph * pw * 3, "f32")
    y = ctx.gather_warp_patches(ctx.to_device(stack), ctx.to_device(table), ctx.to_device(order), 1, B, (ph, pw), params, out=gb.y.view(B, ph, pw, 3))
    assert_guard(gb, case, "y")
    rows = order[1:1 + B]
    patches = np.stack([PR.unit(stack)[table[k, 0], table[k, 1]:table[k, 1] + ph, table[k, 2]:table[k, 2] + pw] for k in rows])
    got = host(y)
    per = ph * pw * 3
    fail_at_first(case, bits(got[0]) != bits(patches[0]), "the identity element", per_row=per)
    warped = ctx.affine_warp(ctx.to_device(patches), np.arange(B), params)
    assert ph * pw * 3 // 4 < G.AFFINE_CAP                                   # that launch goes round once
    fail_at_first(case, bits(got) != bits(host(warped)), "against affine_warp of the patch", per_row=per)
    err = np.abs(got[1] - VF._ref_warp(patches[1], rot[1], off[1], True))
    fail_at_first(case, ~(err <= 2e-5), f"the rotated element against scipy, max {err.max():.3e}", per_row=per)


# ================================================================================================ head_train.hip
@pytest.mark.parametrize("cid", ["affine_warp_v4", "affine_warp_scalar"])
def test_affine_warp_past_the_grid_cap(ctx, cid):
    """The vectorised kernel (four elements per thread) on 592 x 592 x 3 and the scalar one on 513 x 513 x 1 (an odd count): an identity
    element bit for bit, a rotated and mirrored one within 2e-5 of scipy (test_affine_warp_matches_scipy's bound).
    First run on an MI355X: 5.4e-5 and 3.3e-5, in every round alike -- the compiler had contracted the products of warp_sample.h's
    double-float coordinate into the sums behind them; with contraction off there both cases pass (grid caps)."""
    case = G.BY_ID[cid]
    n, H, W, Cx = case.arg
    per = H * W * Cx
    assert (per % 4 == 0) == (cid == "affine_warp_v4")
    rng = np.random.default_rng(H)
    X = rng.uniform(0, 1, (2, H, W, Cx)).astype(np.float32)
    th = np.deg2rad(-11.0)
    rot = np.stack([np.eye(2), np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])])
    off = np.array([[0.0, 0.0], [-25.5, 60.125]])
    flip = np.array([False, True])
    idx = np.array([1, 0], np.int32)
    gb = Guarded(ctx, n * per, "f32")
    assert gb.y.data_ptr() % 16 == 0
    y = ctx.affine_warp(ctx.to_device(X), idx, ctx.warp_params(rot, off, flip), out=gb.y.view(n, H, W, Cx))
    assert_guard(gb, case, "y")
    got = host(y)
    fail_at_first(case, bits(got[0]) != bits(X[1]), "the identity element", per_row=per)
    err = np.abs(got[1] - VF._ref_warp(X[0], rot[1], off[1], True))
    fail_at_first(case, ~(err <= 2e-5), f"the rotated element against scipy, max {err.max():.3e}", per_row=per)


# ================================================================================================ crop.hip
CROP_DESIGNS = {"nested rings": lambda H, W: CROP.nested_rings(H, W, n=6, width=3, gap=4),
                "random 0.5": lambda H, W: np.random.default_rng(2).random((H, W)) < 0.5,
                "spiral": CROP.spiral}


@pytest.mark.parametrize("name", sorted(CROP_DESIGNS))
def test_object_boxes_past_the_mask_grid_cap(ctx, name):
    """513 x 512 frames (the design, its mirror image and upside down): gray, Otsu threshold, mask, labels and boxes exact against
    crop_ref, every output in a poisoned buffer, then the crop."""
    case = G.BY_ID["crop_mask"]
    B, H, W = case.arg
    m = CROP_DESIGNS[name](H, W)
    frames = CROP.frames_from_mask(np.stack([m, m[:, ::-1], m[::-1]]))
    ref = CROP.object_boxes(frames)
    x = ctx.to_device(frames)
    gg, gm = Guarded(ctx, B * H * W, "u8"), Guarded(ctx, B * H * W, "u8")
    boxes = torch.full((B, len(L.BOX_NAMES)), -77, dtype=torch.int32, device=ctx.torch_device)
    labels = torch.full((B, H, W), -77, dtype=torch.int32, device=ctx.torch_device)
    ctx.check(ctx.lib.sr_object_boxes(ctx.h, x.data_ptr(), B, H, W, boxes.data_ptr(), gg.y.data_ptr(), gm.y.data_ptr(), labels.data_ptr(), ctx.stream()))
    assert gg.untouched() and gm.untouched()
    per = H * W
    fail_at_first(case, host(gg.y) != ref["gray"].reshape(-1), "gray", per_row=per)
    assert np.array_equal(host(boxes)[:, 7], ref["boxes"][:, 7])
    fail_at_first(case, host(gm.y) != ref["mask"].reshape(-1), "mask", per_row=per)
    fail_at_first(case, host(labels) != ref["labels"], "labels", per_row=per)
    assert np.array_equal(host(boxes), ref["boxes"]), (host(boxes), ref["boxes"])
    crops = host(ctx.square_crop(x))
    assert np.array_equal(crops, CROP.square_crop(frames, ref["boxes"]))


def test_square_crop_rows_longer_than_the_workgroups_vectors(ctx):
    """1400 x 1500 frames: a row of the 1400-pixel square is 4200 bytes, more 16-byte vectors than the 256 threads copying it, at lefts
    that select the 16-, 4- and 1-byte copies."""
    rng = np.random.default_rng(14)
    frames = rng.integers(0, 256, (3, 1400, 1500, 3), dtype=np.uint8)
    x = ctx.to_device(frames)
    for lefts in ((16, 48, 64), (4, 20, 8), (3, 63, 1)):
        boxes = np.zeros((3, 8), np.int32)
        boxes[:, 5] = lefts
        got = host(ctx.square_crop(x, boxes))
        bad = got != CROP.square_crop(frames, boxes)
        assert not bad.any(), (lefts, "first mismatch at (frame, row, byte of the row)", np.unravel_index(int(np.argmax(bad)), (3, 1400, 4200)))


# ================================================================================================ classic.hip, metrics.hip
CLS_SPECIAL = sorted(set(G.images_crossed(G.CLS_CAP, G.CLS_HR * G.CLS_HR, G.CLS_NH) + G.images_crossed(G.CLS_CAP, G.CLS_LR * G.CLS_LR, G.CLS_NL) + [0]))


@functools.lru_cache(maxsize=None)
def _classic_batch():
    """294 pairs of 478 / 239 from six distinct gray_pairs: image 0 and the images inside which a round ends each have one of their
    own, the sixth fills the rest."""
    assert CLS_SPECIAL == [0, 73, 146, 220, 293]
    pairs = [CL.gray_pair(G.CLS_HR, G.CLS_HR, G.CLS_LR, G.CLS_LR, seed=500 + s) for s in range(6)]
    which = np.full(G.CLS_B, 5)
    which[CLS_SPECIAL] = np.arange(5)
    hr, lr = np.stack([pairs[k][0] for k in which]), np.stack([pairs[k][1] for k in which])
    return pairs, which, hr, lr                                            # shared by three tests, which only read them


def _u8_close_flags(got, ref):
    d = np.abs(got.astype(np.int64) - ref.astype(np.int64))
    return d, d > 1


def test_back_projection_batch_past_the_grid_cap(ctx):
    """Two iterations on the whole batch: ibp_init / ibp_hr cross the cap inside images 73, 146, 220 and 293, ibp_lr inside image 293.
    Those images and image 0 equal the single-image call bit for bit, and the single call meets test_back_projection's bounds."""
    pairs, which, hr, lr = _classic_batch()
    case = G.BY_ID["classic_hr"]
    B, H, h = G.CLS_B, G.CLS_HR, G.CLS_LR
    hd, ld = ctx.to_device(hr, torch.uint8), ctx.to_device(lr, torch.uint8)
    gy, ge = Guarded(ctx, B * H * H, "u8"), Guarded(ctx, B * H * H, "f32")
    ctx.check(ctx.lib.sr_back_projection(ctx.h, hd.data_ptr(), ld.data_ptr(), B, H, H, h, h, 2, gy.y.data_ptr(), ge.y.data_ptr(), ctx.stream()))
    assert gy.untouched() and ge.untouched()
    y, est = host(gy.y).reshape(B, H, H), host(ge.y).reshape(B, H, H)
    single = {}
    for k in range(6):
        y1, e1 = ctx.back_projection(ctx.to_device(pairs[k][0][None], torch.uint8), ctx.to_device(pairs[k][1][None], torch.uint8), 2, raw=True)
        single[k] = (host(y1)[0], host(e1)[0])
    # every image of the batch against the single call of its pair: flat indices of the whole launch
    fail_at_first(case, bits(est) != bits(np.stack([single[k][1] for k in which])), "estimate, batch against single calls")
    fail_at_first(case, y != np.stack([single[k][0] for k in which]), "uint8 result, batch against single calls")
    for k, i in enumerate(CLS_SPECIAL):
        ref_u8, ref_est = CR.back_projection(pairs[k][0], pairs[k][1], 2)
        assert np.max(np.abs(est[i] - ref_est)) <= 1e-3, i
        CL.assert_u8_close(y[i], ref_u8)


def test_edge_guided_batch_past_the_grid_cap(ctx):
    """sobel_mag crosses the cap inside LR image 293, egi_hr inside HR images 73, 146, 220 and 293."""
    pairs, which, _, lr = _classic_batch()
    case = G.BY_ID["classic_hr"]
    B, H, h = G.CLS_B, G.CLS_HR, G.CLS_LR
    ld = ctx.to_device(lr, torch.uint8)
    gy, ge = Guarded(ctx, B * H * H, "u8"), Guarded(ctx, B * H * H, "f32")
    ctx.check(ctx.lib.sr_edge_guided(ctx.h, ld.data_ptr(), B, h, h, H, H, 0.3, gy.y.data_ptr(), ge.y.data_ptr(), ctx.stream()))
    assert gy.untouched() and ge.untouched()
    y, up_e = host(gy.y).reshape(B, H, H), host(ge.y).reshape(B, H, H)
    single = {}
    for k in range(6):
        y1, e1 = ctx.edge_guided(ctx.to_device(pairs[k][1][None], torch.uint8), H, H, raw=True)
        single[k] = (host(y1)[0], host(e1)[0])
    fail_at_first(case, bits(up_e) != bits(np.stack([single[k][1] for k in which])), "up-sized edges, batch against single calls")
    fail_at_first(case, y != np.stack([single[k][0] for k in which]), "uint8 result, batch against single calls")
    for k, i in enumerate(CLS_SPECIAL):
        ref_u8, ref_up_e = CR.edge_guided(pairs[k][1], H, H)
        assert np.max(np.abs(up_e[i] - ref_up_e)) <= 1e-4, i
        CL.assert_u8_close(y[i], ref_u8)


def test_freq_extrapolate_batch_past_the_grid_cap(ctx):
    """4200 images of 64 x 64 widened to fp64 by one capped launch, extrapolated to 72 x 72: |A_H X A_W^T| within 1e-9 of the largest
    value (test_freq_extrapolate's bound), every image."""
    case = G.BY_ID["u8_to_f64"]
    B, h, w = case.arg
    H = W = 72
    x = np.random.default_rng(64).integers(0, 256, (B, h, w), dtype=np.uint8)
    got = host(ctx.freq_extrapolate(ctx.to_device(x, torch.uint8), H, W))
    # classic_ref.freq_extrapolate_fft for the whole batch at once; the operator form the contract names on the first image, the last and
    # the one inside which the round ends (the two forms agree to 1e-12 of the largest value, asserted)
    pad = np.zeros((B, H, W), complex)
    r0, c0 = H // 2 - h // 2, W // 2 - w // 2
    pad[:, r0:r0 + h, c0:c0 + w] = np.fft.fftshift(np.fft.fft2(x.astype(np.float64)), axes=(-2, -1))
    ref = np.abs(np.fft.ifft2(np.fft.ifftshift(pad, axes=(-2, -1))))
    for b in (0, G.images_crossed(case.cap, h * w, case.threads)[0], B - 1):
        assert np.max(np.abs(ref[b] - CR.freq_extrapolate(x[b], H, W))) <= 1e-12 * np.max(ref)
    bad = ~(np.abs(got - ref) <= 1e-9 * np.max(ref))
    if bad.any():                                                          # name the image; its 4096 inputs are elements [4096 b, 4096 (b + 1)) of the launch
        b = int(np.argmax(bad.reshape(B, -1).any(1)))
        pytest.fail(f"{case.id}: image {b} differs; its inputs are flat indices {b * h * w} .., round {b * h * w // case.cap} = index // {case.cap}")


def test_noise_sigma_batch_past_the_grid_cap(ctx):
    """16 385 images of 61 x 61: 32 x 32 detail coefficients each, 16 778 240 in one launch of db2_hh_abs_kernel; the round ends inside
    image 16 383.  That image, the last one and image 0 are distinct, a fourth image fills the rest; every sigma within 1e-12 of
    classic_ref.noise_sigma (test_noise_sigma_odd_and_even_counts's bound)."""
    case = G.BY_ID["noise_sigma"]
    B, h, w = case.arg
    per = ((h + 3) // 2) * ((w + 3) // 2)
    special = sorted(set(G.images_crossed(case.cap, per, case.threads) + [0, B - 1]))
    assert special == [0, B - 2, B - 1]
    imgs = [CL.gray_pair(2 * h, 2 * w, h, w, seed=900 + s)[1] for s in range(4)]
    which = np.full(B, 3)
    which[special] = np.arange(3)
    x = np.stack(imgs)[which]
    sig = host(ctx.noise_sigma(ctx.to_device(x, torch.uint8)))
    ref = np.array([CR.noise_sigma(im) for im in imgs])[which]
    bad = ~(np.abs(sig - ref) <= 1e-12 * ref)
    assert not bad.any(), f"{case.id}: images {np.flatnonzero(bad)[:8]} .. differ; round = image * {per} // {case.cap}"


def test_eda_dct_chunk_past_the_grid_cap(ctx):
    """sr_eda_pair_stats with a caller's DCT buffer on 2048 pairs of 64 x 64: one chunk of 4096 gray images, 2^24 values, 256 more than
    gray_to_f64_kernel's grid holds.  Every image's DCT within 1e-9 of the largest coefficient of eda_ref.dct2 (test_eda_gpu.py's bound).
    Run twice, the second time with the batch reversed, so that values an earlier call left in the work buffer cannot pass for the tail."""
    import eda_ref as ER
    case = G.BY_ID["eda_dct"]
    B, H, W = case.arg
    rng = np.random.default_rng(2048)
    lr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    hr = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    Ch, CwT = ER.dct_operator(H), ER.dct_operator(W).T
    for flip in (False, True):
        a, b = (lr[::-1].copy(), hr[::-1].copy()) if flip else (lr, hr)
        _, raw = ctx.eda_pair_stats(ctx.to_device(a, torch.uint8), ctx.to_device(b, torch.uint8), raw=True)
        got = host(raw["dct"])
        gray = np.stack([ER.gray_u8(a), ER.gray_u8(b)], 1).astype(np.float64)            # [B, 2, H, W]: lr and hr interleaved, as the device holds them
        ref = Ch @ gray @ CwT
        assert np.max(np.abs(ref[3, 1] - ER.dct2(ER.gray_u8(b[3])))) <= 1e-12 * np.abs(ref[3, 1]).max()
        bad = ~(np.abs(got - ref) <= 1e-9 * np.abs(ref).max(axis=(1, 2, 3), keepdims=True))
        if bad.any():
            full = bad.reshape(-1)
            fail_at_first(case, full, f"dct, batch {'reversed' if flip else 'as drawn'}")


def test_rgb2gray_past_the_grid_cap(ctx):
    """294 frames of 478 x 478 x 3 (four pixels per thread: 16 793 574 threads), the channels three different arrangements of the classic
    batch's HR images; bit for bit the integer expression, with the aligned kernel and -- output one byte off -- the unaligned one."""
    case = G.BY_ID["rgb2gray"]
    pairs, which, _, _ = _classic_batch()
    six = np.stack([np.stack([p[0], p[0][::-1, ::-1], p[0].T], -1) for p in pairs])
    ref6 = MR.rgb2gray_u8(six)
    x = ctx.to_device(six[which], torch.uint8)
    n = G.CLS_NH
    assert x.shape == case.arg and x.data_ptr() % 4 == 0
    for shift, what in ((0, "aligned"), (1, "output one byte off")):
        gb = Guarded(ctx, n + 4, "u8")
        y = gb.y[shift:shift + n]
        assert (y.data_ptr() % 4 == 0) == (shift == 0)
        ctx.check(ctx.lib.sr_rgb2gray_u8(ctx.h, x.data_ptr(), G.CLS_B, G.CLS_HR, G.CLS_HR, y.data_ptr(), ctx.stream()))
        assert gb.untouched(), what
        out = host(gb.y)
        assert np.all(out[:shift] == IO.U8_POISON) and np.all(out[shift + n:] == IO.U8_POISON), what
        got = out[shift:shift + n].reshape(G.CLS_B, -1)
        for c0 in range(0, G.CLS_B, 49):                                   # in chunks of 49 frames
            sl = slice(c0, c0 + 49)
            bad = got[sl] != ref6[which[sl]].reshape(len(which[sl]), -1)
            if bad.any():
                full = np.zeros(n, bool)
                full[c0 * G.CLS_HR ** 2:c0 * G.CLS_HR ** 2 + bad.size] = bad.reshape(-1)
                fail_at_first(case, full, what)


# ================================================================================================ conv.hip
@pytest.mark.parametrize("rot", [False, True], ids=["plain", "rot"])
def test_conv2d_dev_packs_a_512_to_512_kernel(ctx, rot):
    """pack_weights_f32_kernel on 3 x 3 x 512 x 512 (2 359 296 packed values, the grid capped at 4096 x 256): sr_conv2d_dev equals the
    host-packed sr_conv2d bit for bit (test_conv2d_dev_matches_host_packed_conv's contract) and the fp64 convolution."""
    case = G.BY_ID["pack_weights_f32"]
    K, _, cin, cout = case.arg
    rng = np.random.default_rng(512 + rot)
    x = rng.standard_normal((1, 4, 4, 512)).astype(np.float32)
    k = (rng.standard_normal(case.arg) / np.sqrt(K * K * cin)).astype(np.float32)
    b = None if rot else rng.uniform(-0.1, 0.1, cout).astype(np.float32)
    xd, kd = ctx.to_device(x), ctx.to_device(k)
    keff = T._rot(k) if rot else k
    want = ctx.conv2d(xd, keff, b)
    got = ctx.conv2d_dev(xd, kd, None if b is None else ctx.to_device(b), 512, rot=rot)
    assert torch.equal(got, want), int((got != want).sum())
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    ref = sum(np.einsum("bhwi,io->bhwo", xp[:, i:i + 4, j:j + 4], keff[i, j].astype(np.float64)) for i in range(3) for j in range(3))
    if b is not None:
        ref = ref + b
    assert BK.rel_l2(host(got), ref) <= 1e-5                               # the fp32 conv contract of test_conv_routes_gpu.py
