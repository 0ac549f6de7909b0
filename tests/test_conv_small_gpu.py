"""sr_conv3x3_small_bf16 (csrc/conv_small.hip) through the C ABI: per element against fp64 recomputed from the device's own stored inputs
(tests/vgg_mixed_ref.py), bit for bit against sr_conv2d_dev_bf16 where every partial sum is exact, and the properties a batch-spanning tile could break: no
image reads another, an image's bits depend on nothing but the image."""
import functools

import numpy as np
import pytest
import torch

import vgg_mixed_ref as R
from sr355 import _lib as L

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@functools.lru_cache(maxsize=None)
def reference(shape, rot):
    """The operands and the linear fp64 value of one (shape, rot), computed once for the eight cases that share it."""
    x, w, b, mask = R.conv_operands(shape, rot)
    v, bound = R.conv_small_ref(x, w, b, rot, "linear")
    return x, w, b, mask, v, bound


@functools.lru_cache(maxsize=None)
def on_device(shape, rot):
    from sr355 import Context
    ctx = Context.get(0)
    x, w, b, mask, _, _ = reference(shape, rot)
    return tuple(ctx.to_device(a) for a in (x, w, b, mask))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("act", ["linear", "relu"])
@pytest.mark.parametrize("rot", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("shape", R.SHAPES, ids=R.shape_id)
def test_every_element_against_fp64(ctx, shape, rot, act, masked):
    """2^-8 |v| + (9 Cin + 2) 2^-24 S per element; at most 1e-2 of the non-zero elements off the once-rounded reference, by one step.  With a mask: +0 (the
    bits) exactly where mask <= 0, the unmasked call's bits elsewhere, and the bits of the unmasked call followed by sr_relu_bwd_bf16 everywhere."""
    _, _, _, mask, v, bound = reference(shape, rot)
    xd, wd, bd, md = on_device(shape, rot)
    cout = shape[4]
    if act == "relu":
        v = torch.relu(v)
    plain = ctx.conv3x3_small_bf16(xd, wd, bd, cout, rot=rot, act=act)
    if not masked:
        R.check_conv(f"{R.shape_id(shape)} rot={int(rot)} {act}", R.t64(plain), v, bound)
        return
    got = ctx.conv3x3_small_bf16(xd, wd, bd, cout, rot=rot, act=act, mask=md)
    assert np.array_equal(R.bf16_bits(got), R.bf16_bits(ctx.relu_bwd_bf16(plain, md)))
    keep = R.positive_bits(mask)
    assert 0.3 < float(keep.double().mean()) < 0.7
    gb = torch.from_numpy(R.bf16_bits(got).astype(np.int32))
    assert bool((gb[~keep] == 0).all()), "a masked element is not +0"
    zero = torch.zeros(()).double()
    R.check_conv(f"{R.shape_id(shape)} rot={int(rot)} {act} masked", R.t64(got), torch.where(keep, v, zero), torch.where(keep, bound, zero))


def small_integers(shape, rot, seed):
    B, H, W, cin, cout = shape
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-3, 4, (B, H, W, cin)).astype(np.float32)).to(BF16)
    w = rng.integers(-2, 3, (3, 3, cout, cin) if rot else (3, 3, cin, cout)).astype(np.float32)
    b = rng.integers(-4, 5, cout).astype(np.float32)
    return x, w, b


@pytest.mark.parametrize("rot", [False, True], ids=["fwd", "dgrad"])
@pytest.mark.parametrize("shape", [(5, 3, 3, 512, 512), (2, 12, 12, 128, 256), (3, 5, 7, 96, 64), (7, 1, 1, 64, 32)], ids=R.shape_id)
def test_small_integers_give_the_bits_of_conv2d_dev_bf16(ctx, shape, rot):
    """|x| <= 3, |w| <= 2, |b| <= 4: every partial sum is an integer below 9 * 512 * 6 + 4 < 2^24, exact in fp32 in any order, so the two kernels differ in
    nothing but the order and must agree to the bit -- and with the integer fp64 value rounded once."""
    x, w, b = small_integers(shape, rot, 17)
    xd, wd, bd = ctx.to_device(x), ctx.to_device(w), ctx.to_device(b)
    for act in ("linear", "relu"):
        got = ctx.conv3x3_small_bf16(xd, wd, bd, shape[4], rot=rot, act=act)
        want = ctx.conv2d_dev_bf16(xd, wd, bd, shape[4], rot=rot, act=act)
        assert np.array_equal(R.bf16_bits(got), R.bf16_bits(want)), act
        v, _ = R.conv_small_ref(x, w, b, rot, act)
        assert torch.equal(R.t64(got), R.rb(v)), act


@pytest.mark.parametrize("shape", [(5, 3, 3, 512, 512), (3, 5, 7, 96, 64), (7, 1, 1, 64, 32)], ids=R.shape_id)
def test_a_nan_image_stays_in_its_image(ctx, shape):
    """One image of NaN and Inf among finite ones: the tile that holds it holds its neighbours' pixels too.  Every other image's output is finite and, to the
    bit, what it is beside a finite image."""
    x, w, b, _ = R.conv_operands(shape, False, seed=1)
    bad = x.clone()
    k = shape[0] // 2
    bad[k] = float("nan")
    bad[k, ..., ::2] = float("inf")
    bad[k, ..., 1::4] = float("-inf")
    wd, bd = ctx.to_device(w), ctx.to_device(b)
    clean = ctx.conv3x3_small_bf16(ctx.to_device(x), wd, bd, shape[4])
    dirty = ctx.conv3x3_small_bf16(ctx.to_device(bad), wd, bd, shape[4])
    others = [i for i in range(shape[0]) if i != k]
    assert bool(torch.isfinite(dirty[others].float()).all())
    assert np.array_equal(R.bf16_bits(dirty[others].contiguous()), R.bf16_bits(clean[others].contiguous()))
    assert not bool(torch.isfinite(dirty[k].float()).all())                         # the planted image did run


@pytest.mark.parametrize("shape", [(5, 3, 3, 512, 512), (3, 6, 6, 512, 512), (3, 5, 7, 96, 64)], ids=R.shape_id)
def test_an_images_bits_depend_on_the_image_alone(ctx, shape):
    """Not on B, not on its place in the batch (another column of the MFMA tile, another tile), not on what the LDS held before: a batch of NaNs runs first in
    the same process; then the batch, its images one at a time, and the batch reversed behind an extra image."""
    x, w, b, _ = R.conv_operands(shape, True, seed=2)
    cout = shape[4]
    wd, bd = ctx.to_device(w), ctx.to_device(b)
    nan = ctx.to_device(torch.full(x.shape, float("nan")).to(BF16))
    assert bool(torch.isnan(ctx.conv3x3_small_bf16(nan, wd, bd, cout, rot=True).float()).all())
    whole = R.bf16_bits(ctx.conv3x3_small_bf16(ctx.to_device(x), wd, bd, cout, rot=True))
    for i in range(shape[0]):
        one = ctx.conv3x3_small_bf16(ctx.to_device(x[i:i + 1].contiguous()), wd, bd, cout, rot=True)
        assert np.array_equal(R.bf16_bits(one)[0], whole[i]), i
    rev = torch.cat([x[:1], x.flip(0)]).contiguous()
    back = R.bf16_bits(ctx.conv3x3_small_bf16(ctx.to_device(rev), wd, bd, cout, rot=True))
    assert np.array_equal(back[1:][::-1], whole)


def test_a_packed_handle_gives_the_same_bits_and_outlives_the_per_step_lists(ctx):
    shape = (3, 6, 6, 512, 512)
    for rot in (False, True):
        xd, wd, bd, _ = on_device(shape, rot)
        want = R.bf16_bits(ctx.conv3x3_small_bf16(xd, wd, bd, 512, rot=rot, act="relu"))
        handle = ctx.conv3x3_small_pack(wd, rot=rot)
        assert handle.numel() * 2 == ctx.lib.sr_conv3x3_small_pack_bytes(512, 512) == 9 * 512 * 512 * 2
        ctx.conv_prepack_bf16(None)                                                  # the per-step list is forgotten: the handle is no part of it
        ctx.conv3x3_small_bf16(xd, wd, bd, 512, rot=not rot)                         # another kernel passes through the context's own pack arena
        got = ctx.conv3x3_small_bf16(xd, None, bd, 512, act="relu", packed=handle)
        assert np.array_equal(R.bf16_bits(got), want)


def test_rejected_shapes_launch_nothing(ctx):
    lib, S = ctx.lib, ctx.stream
    y = torch.full((2 * 13 * 13 * 64,), 7.0, dtype=BF16, device=ctx.torch_device)
    x = torch.zeros((2 * 13 * 13 * 64,), dtype=BF16, device=ctx.torch_device)
    w = torch.zeros((9 * 64 * 64,), dtype=torch.float32, device=ctx.torch_device)
    call = lambda B, H, W, cin, cout, act=L.ACT_LINEAR: lib.sr_conv3x3_small_bf16(ctx.h, x.data_ptr(), B, H, W, cin, w.data_ptr(), None, None, cout, 0, act, None,
                                                                                 y.data_ptr(), S())
    assert call(2, 12, 12, 48, 64) == L.SR_ERR_INVALID                              # Cin = 48: a chunk and a half
    assert b"multiples of 32" in lib.sr_last_error(ctx.h)
    assert call(2, 12, 12, 64, 48) == L.SR_ERR_INVALID
    assert call(2, 13, 13, 64, 64) == L.SR_ERR_INVALID                              # 169 pixels
    assert b"144" in lib.sr_last_error(ctx.h)
    assert call(2, 1, 145, 64, 64) == L.SR_ERR_INVALID
    assert call(0, 12, 12, 64, 64) == L.SR_ERR_INVALID
    assert call(2, 12, 12, 64, 64, L.ACT_LRELU) == L.SR_ERR_INVALID
    assert lib.sr_conv3x3_small_pack_bytes(48, 64) == 0 and lib.sr_conv3x3_small_pack_bytes(64, 0) == 0
    assert lib.sr_conv3x3_small_pack_bf16(ctx.h, w.data_ptr(), 48, 64, 0, y.data_ptr(), S()) == L.SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert call(2, 12, 12, 64, 64) == L.SR_OK                                       # the largest image the kernel takes
    torch.cuda.synchronize()
    assert bool((y[:2 * 144 * 64] == 0.0).all()) and bool((y[2 * 144 * 64:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- the branch's other kernels
def bf(rng, shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(BF16)


def pool_input(shape, seed):
    """N(0,1) with every tie the rule has to decide: an all-zero window, a window of -0 and +0, two equal maxima, equal maxima on the diagonal, an all-negative
    window, and the special bit patterns."""
    x = bf(np.random.default_rng(seed), shape)
    x[0, 0:2, 0:2, 0] = 0.0
    x[0, 0:2, 0:2, 1] = torch.tensor([[-0.0, 0.0], [0.0, -0.0]]).to(BF16)
    x[0, 0:2, 0:2, 2] = torch.tensor([[0.5, 2.0], [2.0, 1.0]]).to(BF16)
    x[0, 0:2, 0:2, 3] = torch.tensor([[3.0, 1.0], [1.0, 3.0]]).to(BF16)
    x[0, 0:2, 0:2, 4] = torch.tensor([[-3.0, -1.0], [-1.0, -2.0]]).to(BF16)
    if shape[3] >= 16:
        x.view(torch.int16)[0, 0, 0, 8:16] = torch.tensor(R.SPECIAL_BITS, dtype=torch.int16)
    return x


@pytest.mark.parametrize("shape", [(2, 3, 3, 16), (3, 7, 5, 24), (2, 12, 12, 64), (1, 2, 2, 8)], ids=R.shape_id)
def test_pools_are_selects_with_the_first_winner_rule(ctx, shape):
    """3 x 3 -> 1 x 1 and 7 x 5 -> 3 x 2 drop a row and a column.  Forward: the bits of the window's maximum.  Backward: dy's bits at the first winner where it
    is positive, +0 everywhere else -- both against the restated reference, bit for bit (NaN windows aside, which the reference does not define)."""
    x = pool_input(shape, 3)
    finite = ~torch.isnan(x.float())
    xs = torch.where(finite, x, torch.zeros((), dtype=BF16))                        # the reference's view; the device gets the same values
    xd = ctx.to_device(xs)
    y = ctx.maxpool2_bf16(xd)
    assert tuple(y.shape) == (shape[0], shape[1] // 2, shape[2] // 2, shape[3])
    assert torch.equal(R.t64(y), R.pool64(R.t64(xs)))
    dy = bf(np.random.default_rng(4), tuple(y.shape))
    dx = ctx.maxpool2_bwd_bf16(xd, ctx.to_device(dy))
    want = R.pool_bwd64(R.t64(xs), R.t64(dy))
    assert torch.equal(R.t64(dx), want)
    db = torch.from_numpy(R.bf16_bits(dx).astype(np.int32))
    assert bool((db[want == 0] == 0).all()), "a zero of the gradient is not +0"
    routed = int((want != 0).sum())
    assert 0 < routed <= y.numel()
    with pytest.raises(ValueError, match="multiple of 8"):
        ctx.maxpool2_bf16(ctx.to_device(bf(np.random.default_rng(5), (1, 4, 4, 12))))
    with pytest.raises(ValueError, match="at least 2 x 2"):
        ctx.maxpool2_bf16(ctx.to_device(bf(np.random.default_rng(5), (1, 1, 4, 8))))


def test_pool_backward_is_the_fp32_pool_backward_then_the_relu_select(ctx):
    """On values bf16 holds exactly, sr_maxpool2_bwd (fp32) followed by the select x > 0 is the same routing."""
    x = pool_input((2, 7, 5, 16), 6)
    x = torch.where(torch.isnan(x.float()), torch.zeros((), dtype=BF16), x)
    dy = bf(np.random.default_rng(7), (2, 3, 2, 16))
    xd, dyd = ctx.to_device(x), ctx.to_device(dy)
    got = ctx.maxpool2_bwd_bf16(xd, dyd)
    ref = ctx.maxpool2_bwd(xd.float(), dyd.float())
    ref = torch.where(xd.float() > 0, ref, torch.zeros((), device=ref.device))
    assert torch.equal(got.float(), ref)


def test_preprocess_pair_against_the_fp32_kernel_and_the_restated_reference(ctx):
    """hi = bf16(v) and lo = bf16(v - hi) of the very v SR_SP_VGG_PREPROCESS stores in fp32, fake first; hi + lo reproduces that v to 2^-16 |v| and the fp64 value
    to 2^-16 |v| + 2^-15 (v is evaluated in fp32 at magnitudes up to 255: three roundings of at most 2^-17 .. 2^-16).  The backward: 127.5 x the flipped channels."""
    hr, fake = R.images(3, 10, 21)
    hr[0, 0, 0] = [-1.0, 0.0, 1.0]
    fake[0, 0, 0] = [1.0, -1.0, 0.25]
    hd, fd = ctx.to_device(hr), ctx.to_device(fake)
    out = ctx.vgg_preprocess_bf16(fd, hd)
    assert tuple(out.shape) == (6, 10, 10, 6) and out.dtype == BF16
    v32 = torch.cat([ctx.spatial_op(L.SP_VGG_PREPROCESS, fd), ctx.spatial_op(L.SP_VGG_PREPROCESS, hd)])
    hi = v32.to(BF16)
    lo = (v32 - hi.float()).to(BF16)
    assert torch.equal(out[..., :3].view(torch.int16), hi.view(torch.int16)) and torch.equal(out[..., 3:].view(torch.int16), lo.view(torch.int16))
    o64, v32_64 = R.t64(out), R.t64(v32)
    assert float(((o64[..., :3] + o64[..., 3:] - v32_64).abs() - 2.0 ** -16 * v32_64.abs()).max()) <= 0.0
    v = R.preprocess64(torch.cat([R.t64(fake), R.t64(hr)]))
    assert float(((o64[..., :3] + o64[..., 3:] - v).abs() - 2.0 ** -16 * v.abs()).max()) <= 2.0 ** -15
    assert float((o64[..., :3] - v).abs().max()) > 2.0 ** -4                          # bf16 alone is coarse here: the pair is what makes the entry exact
    ref = R.hi_lo(v)
    print(f"preprocess: {float((o64 != ref).double().mean()):.2e} of the pair's elements differ from the fp64 restatement (fp32 v on the other side of a bf16 boundary)")
    dv = bf(np.random.default_rng(22), (3, 10, 10, 3), 1e-3)
    d = ctx.vgg_preprocess_bwd(ctx.to_device(dv))
    assert d.dtype == torch.float32 and torch.equal(d.cpu(), np.float32(127.5) * dv.float().flip(-1))


@pytest.mark.parametrize("shape", [(4, 3, 3, 512), (2, 1, 1, 512), (6, 5, 7, 40), (2, 24, 24, 512)], ids=R.shape_id)
def test_mse_grad_against_the_restated_reference(ctx, shape):
    """perc = mean((ff - fr)^2) summed in fp64: within fp32's rounding of the fp64 value; dff bit for bit bf16(fp32(2 / n) * fp32(ff - fr)) where ff > 0, +0 elsewhere
    (the special bit patterns among ff).  (6,5,7,40): 4200 elements per half, 17 workgroups of partial sums; (2,24,24,512): 294 912, past the cap of 1024
    workgroups x 256 elements, so that every thread takes a second round."""
    assert shape != (2, 24, 24, 512) or shape[1] * shape[2] * shape[3] > 1024 * 256
    rng = np.random.default_rng(31)
    feats = torch.relu(bf(rng, shape).float()).to(BF16)
    feats.view(torch.int16)[0, 0, 0, :8] = torch.tensor(R.SPECIAL_BITS[:6] + [0x0000, 0x007F], dtype=torch.int16)      # (no NaN: the loss would be NaN)
    feats[0, 0, 0, 4:6] = torch.tensor([3.0, -2.0]).to(BF16)                                                           # (nor an infinity)
    perc, dff = ctx.mse_grad_bf16(ctx.to_device(feats))
    p_ref, d_ref = R.mse_grad_ref(R.t64(feats))
    assert abs(float(perc) - float(p_ref)) <= 2.0 ** -24 * float(p_ref)
    assert tuple(dff.shape) == (shape[0] // 2,) + shape[1:] and torch.equal(R.t64(dff), d_ref)
    keep = R.positive_bits(feats[:shape[0] // 2])
    db = torch.from_numpy(R.bf16_bits(dff).astype(np.int32))
    assert bool((db[~keep] == 0).all()) and 0.2 < float(keep.double().mean()) < 0.8
    again = ctx.mse_grad_bf16(ctx.to_device(feats))
    assert float(again[0]) == float(perc) and torch.equal(again[1].view(torch.int16), dff.view(torch.int16))
