"""The device pieces of bf16 mixed-precision training, one at a time (include/sr355.h: sr_conv2d_wgrad_bf16, sr_conv2d_dev_bf16, sr_conv_prepack_bf16,
sr_mse_clip_grad_bf16, sr_relu_bwd_bf16, sr_space_to_depth_bf16), against fp64 on the same bf16 values (tests/edsr_mixed_ref.py) or, for the conv,
bit for bit against sr_conv2d with the same weights as host arrays."""
import numpy as np
import pytest
import torch

import edsr_mixed_ref as R
from sr355 import _lib as L
from sr355 import train as T

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16

# csrc/wgrad_bf16.hip: an 8 x 16-pixel tile per step, at most 64 pixel splits per (32-cin block, 32-cout block) pair.  (4, 41, 81): 4 * 6 * 6 = 144 tiles
# > 2 * 64, so with one channel-block pair every workgroup walks 3 tiles (48 splits), ragged on both edges.
WB_TH, WB_TW, WB_MAX_SPLIT = 8, 16, 64
SPLIT_CAP_SHAPE = (4, 41, 81, 32, 32)
assert 4 * -(-41 // WB_TH) * -(-81 // WB_TW) > 2 * WB_MAX_SPLIT

WGRAD_SHAPES = [(2, 37, 53, 32, 32), (3, 1, 50, 16, 24), (3, 45, 1, 24, 16), (5, 1, 1, 8, 16), (4, 24, 24, 3, 64), (4, 24, 24, 64, 3), (2, 19, 29, 37, 45),
                (2, 19, 29, 40, 48), (16, 24, 24, 64, 64), SPLIT_CAP_SHAPE]


def f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def wgrad_operands(shape, rng, integers):
    """bf16 device x (channel-padded to 8 with planted non-zero padding when Cin = 3) and dy, and their fp64 values."""
    B, H, W, Cin, Cout = shape
    cx = 8 if Cin == 3 else Cin
    if integers:
        x, dy = rng.integers(-2, 3, (B, H, W, cx)).astype(np.float32), rng.integers(-2, 3, (B, H, W, Cout)).astype(np.float32)
    else:
        x, dy = rng.standard_normal((B, H, W, cx)).astype(np.float32), rng.standard_normal((B, H, W, Cout)).astype(np.float32)
    if cx != Cin:
        x[..., Cin:] = 3.0                                           # must not count
    xb, dyb = torch.from_numpy(x).to(BF16), torch.from_numpy(dy).to(BF16)
    return xb, dyb, xb.double()[..., :Cin], dyb.double()


@pytest.fixture(scope="module")
def wgrad_random_refs():
    """fp64 references of the random cases, computed once per shape."""
    cache = {}

    def get(shape):
        if shape not in cache:
            xb, dyb, x64, dy64 = wgrad_operands(shape, np.random.default_rng(sum(shape)), integers=False)
            cache[shape] = (xb, dyb) + R.wgrad64(x64, dy64)
        return cache[shape]
    return get


def check_wgrad_integers(ctx, shape, scale):
    xb, dyb, x64, dy64 = wgrad_operands(shape, np.random.default_rng(7 + sum(shape)), integers=True)
    dw, db = ctx.conv2d_wgrad_bf16(ctx.to_device(xb), ctx.to_device(dyb), 3, scale=scale, cin=shape[3])
    rw, rbias = R.wgrad64(x64, dy64, scale)
    assert float(rw.abs().max()) < 2 ** 24
    if shape[1:3] == (1, 1):                                         # one pixel: only the centre tap can be non-zero
        assert float(dw.cpu().reshape(9, -1)[[0, 1, 2, 3, 5, 6, 7, 8]].abs().max()) == 0.0
    assert np.array_equal(f32_bits(dw), f32_bits(rw.float())) and np.array_equal(f32_bits(db), f32_bits(rbias.float()))


@pytest.mark.parametrize("shape", WGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_wgrad_bf16_exact_on_integers(ctx, shape):
    """Inputs in {-2..2}: every product and every partial sum is an integer below 2^24 (at most 4 * 16 * 24 * 24 pixels = 36 864), so fp32 accumulation
    in any order is exact and dw, db must be the fp64 reference bit for bit."""
    check_wgrad_integers(ctx, shape, 1.0)


@pytest.mark.parametrize("shape", [(2, 37, 53, 32, 32), (4, 24, 24, 3, 64), SPLIT_CAP_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_wgrad_bf16_scale_half_stays_exact(ctx, shape):
    """scale = 0.5 on the finished integer sums: a power of two, still exact."""
    check_wgrad_integers(ctx, shape, 0.5)


@pytest.mark.parametrize("shape", WGRAD_SHAPES + [(16, 48, 48, 64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_wgrad_bf16_random_against_fp64(ctx, shape, wgrad_random_refs):
    """Standard-normal data rounded to bf16: rel-L2 <= 2e-6 against fp64 on the rounded operands -- the bound tests/test_backward_kernels_gpu.py holds the
    fp32 kernel to; here the products are exact and only the fp32 summation rounds.  Two runs give the same bits (no atomics)."""
    xb, dyb, rw, rbias = wgrad_random_refs(shape)
    xd, dyd = ctx.to_device(xb), ctx.to_device(dyb)
    dw, db = ctx.conv2d_wgrad_bf16(xd, dyd, 3, cin=shape[3])
    dw2, db2 = ctx.conv2d_wgrad_bf16(xd, dyd, 3, cin=shape[3])
    ew, eb = R.rel_l2(dw, rw), R.rel_l2(db, rbias)
    print(f"wgrad_bf16 {shape}: rel-L2 dw {ew:.3e} db {eb:.3e}")
    assert np.array_equal(f32_bits(dw), f32_bits(dw2)) and np.array_equal(f32_bits(db), f32_bits(db2))
    assert ew <= 2e-6 and eb <= 2e-6


# ---------------------------------------------------------------------------------------------------------------- conv
CONV_CASES = {  # name: (Cin, Cout, size, kwargs, number of skips)
    "head_relu": (3, 64, 24, dict(act="relu"), 0),
    "block_alpha_skip": (64, 64, 24, dict(alpha=0.1), 1),
    "block_alpha_two_skips": (64, 64, 24, dict(alpha=0.1), 2),
    "up_d2s2": (64, 256, 24, dict(d2s=2), 0),
    "up_d2s3": (64, 576, 12, dict(d2s=3), 0),
    "rgb": (64, 3, 48, dict(), 0),
}


def conv_case(ctx, name, B=2):
    cin, cout, n, kw, nskip = CONV_CASES[name]
    rng = np.random.default_rng(len(name) + cin + cout)
    w = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = None if name == "rgb" else rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    x = ctx.to_device(torch.from_numpy(rng.standard_normal((B, n, n, cin)).astype(np.float32)).to(BF16))
    r = kw.get("d2s", 1)
    skips = [ctx.to_device(torch.from_numpy(rng.standard_normal((B, n * r, n * r, cout // (r * r))).astype(np.float32)).to(BF16)) for _ in range(nskip)]
    kw = dict(kw)
    for i, s in enumerate(skips, 1):
        kw[f"skip{i}"], kw[f"beta{i}"] = s, 1.0
    return x, w, b, kw


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv2d_dev_bf16_is_conv2d_bit_for_bit(ctx, name):
    """Device weights (fp32, rounded by the device pack kernel) against the same weights as host arrays (rounded by the host packer): the packed images
    agree and the kernel is the same, so the bits are.  Prepacked and not prepacked give the same bits too."""
    x, w, b, kw = conv_case(ctx, name)
    wd, bd = ctx.to_device(w), None if b is None else ctx.to_device(b)
    want = ctx.conv2d(x, w, b, **kw)
    got = ctx.conv2d_dev_bf16(x, wd, bd, w.shape[3], **kw)
    assert got.dtype == BF16 and got.shape == want.shape
    assert np.array_equal(R.bf16_bits(got), R.bf16_bits(want))
    try:
        ctx.conv_prepack_bf16(ctx.pack_list([(wd, bd, False)]))
        packed = ctx.conv2d_dev_bf16(x, wd, bd, w.shape[3], **kw)
    finally:
        ctx.conv_prepack_bf16(None)
    assert np.array_equal(R.bf16_bits(packed), R.bf16_bits(want))


@pytest.mark.parametrize("name", ["head_relu", "block_alpha_skip", "up_d2s2", "rgb"])
def test_conv2d_dev_bf16_rot_is_conv2d_on_the_rotated_kernel(ctx, name):
    """rot=True on the layer's forward kernel [3,3,Cin,Cout]: the input-gradient conv of a [.., Cout] gradient, bit for bit ctx.conv2d on _rot(w)."""
    cin, cout, n, _, _ = CONV_CASES[name]
    rng = np.random.default_rng(90 + cin + cout)
    w = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    dy = ctx.to_device(torch.from_numpy(rng.standard_normal((2, n, n, cout)).astype(np.float32)).to(BF16))
    wd = ctx.to_device(w)
    want = ctx.conv2d(dy, T._rot(w), None, alpha=0.1)
    got = ctx.conv2d_dev_bf16(dy, wd, None, cin, rot=True, alpha=0.1)
    assert np.array_equal(R.bf16_bits(got), R.bf16_bits(want))
    try:
        ctx.conv_prepack_bf16(ctx.pack_list([(wd, None, True)]))
        packed = ctx.conv2d_dev_bf16(dy, wd, None, cin, rot=True, alpha=0.1)
    finally:
        ctx.conv_prepack_bf16(None)
    assert np.array_equal(R.bf16_bits(packed), R.bf16_bits(want))


def test_prepack_lists_of_both_dtypes_hold_the_same_weight_and_follow_it(ctx):
    """The same (w, bias, K, Cin, Cout, rot) on the fp32 list and on the bf16 list: each conv finds its own image.  After the weight buffer is
    overwritten and the prepack repeated, the results follow the new weights."""
    rng = np.random.default_rng(3)
    w0, w1 = [(rng.standard_normal((3, 3, 64, 64)) * 0.06).astype(np.float32) for _ in range(2)]
    b = rng.uniform(-0.05, 0.05, 64).astype(np.float32)
    x32 = ctx.to_device(rng.standard_normal((2, 24, 24, 64)).astype(np.float32))
    x16 = x32.to(BF16)
    wd, bd = ctx.to_device(w0.copy()), ctx.to_device(b)
    pl = ctx.pack_list([(wd, bd, False)])
    try:
        for w in (w0, w1):
            wd.copy_(ctx.to_device(w))
            ctx.conv_prepack(pl)
            ctx.conv_prepack_bf16(pl)
            got16, got32 = ctx.conv2d_dev_bf16(x16, wd, bd, 64), ctx.conv2d_dev(x32, wd, bd, 64)
            assert np.array_equal(R.bf16_bits(got16), R.bf16_bits(ctx.conv2d(x16, w, b)))
            assert np.array_equal(f32_bits(got32), f32_bits(ctx.conv2d(x32, w, b)))
        stale = ctx.conv2d_dev_bf16(x16, wd, bd, 64)                  # forgetting the fp32 list leaves the bf16 list alone
        ctx.conv_prepack(None)
        assert np.array_equal(R.bf16_bits(ctx.conv2d_dev_bf16(x16, wd, bd, 64)), R.bf16_bits(stale))
    finally:
        ctx.conv_prepack(None)
        ctx.conv_prepack_bf16(None)


# ---------------------------------------------------------------------------------------------------------------- loss
MSE_MAX_BLOCKS = 1024          # csrc/wgrad_bf16.hip: 256 threads per block, grid-stride above 1024 blocks


def bf16_neighbours(v):
    b = torch.tensor([v], dtype=torch.float32).to(BF16).view(torch.int16)
    return [(b + d).view(BF16).float().item() for d in (-1, 0, 1)]


@pytest.mark.parametrize("n", [7, 16 * 48 * 48 * 3, MSE_MAX_BLOCKS * 256 + 3])
def test_mse_clip_grad_bf16(ctx, n):
    """pre at and around 0 and 1 (the values, their bf16 neighbours, both zeros, far outside), then random; t fp32, not representable in bf16.  dpre is
    bitwise fp32 2 / n * (y - t) in NumPy's order rounded to nearest even, 0 outside [0, 1]; the loss is within n 2^-24 relative of the fp64 mean (the
    kernel sums exact fp64 squares; the fp32 result rounds once); y = clip(pre); two runs give the same bits."""
    rng = np.random.default_rng(n)
    tiny = torch.tensor([0x0001, -0x7FFF], dtype=torch.int16).view(BF16).float().tolist()          # the bf16 neighbours of zero: +- 2^-133
    special = [0.0, -0.0, 1.0] + tiny + bf16_neighbours(1.0) + [7.5, -3.0, 1e30, -1e30]
    special = special[:n] if n < len(special) else special
    pre = np.concatenate([np.asarray(special, np.float32), rng.uniform(-0.3, 1.3, n - len(special)).astype(np.float32)])
    pre16 = torch.from_numpy(pre).to(BF16)
    t = (rng.uniform(0, 1, n).astype(np.float32) + np.float32(2.0 ** -12)).astype(np.float32)
    assert not np.array_equal(torch.from_numpy(t).to(BF16).float().numpy(), t)
    pd, td = ctx.to_device(pre16), ctx.to_device(t)
    y, loss, dpre = ctx.mse_clip_grad_bf16(pd, td)
    y2, loss2, dpre2 = ctx.mse_clip_grad_bf16(pd, td)
    want = R.dpre_bits_ref(pre16.double(), t)
    assert np.array_equal(R.bf16_bits(dpre), R.bf16_bits(want))
    p64 = pre16.double().numpy()
    y64 = np.clip(p64, 0.0, 1.0)
    assert np.array_equal(y.cpu().numpy(), y64.astype(np.float32))
    mean64 = float(np.mean((y64 - t.astype(np.float64)) ** 2))
    got = float(loss.cpu()[0])
    print(f"mse_clip_grad n={n}: loss {got!r} fp64 {mean64!r} rel {abs(got - mean64) / mean64:.2e}")
    assert abs(got - mean64) <= n * 2.0 ** -24 * mean64
    assert np.array_equal(f32_bits(loss), f32_bits(loss2)) and np.array_equal(R.bf16_bits(dpre), R.bf16_bits(dpre2)) and torch.equal(y, y2)


# ---------------------------------------------------------------------------------------------------------------- selects and permutations
def test_relu_bwd_bf16_is_a_select(ctx):
    """y covers +0, -0, the smallest positive bf16 (a subnormal), its negative, ordinary values of both signs, infinities; dy arbitrary bit patterns."""
    rng = np.random.default_rng(5)
    ybits = np.concatenate([np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x0080, 0x8080, 0x3F80, 0xBF80, 0x7F80, 0xFF80], np.uint16),
                            torch.from_numpy(rng.standard_normal(70001).astype(np.float32)).to(BF16).view(torch.int16).numpy().view(np.uint16)])
    dybits = torch.from_numpy(rng.standard_normal(len(ybits)).astype(np.float32)).to(BF16).view(torch.int16).numpy().view(np.uint16)
    y = ctx.to_device(torch.from_numpy(ybits.view(np.int16)).view(BF16))
    dy = ctx.to_device(torch.from_numpy(dybits.view(np.int16)).view(BF16))
    out = ctx.relu_bwd_bf16(dy, y)
    yv = torch.from_numpy(ybits.view(np.int16)).view(BF16).double().numpy()
    want = np.where(yv > 0, dybits, np.uint16(0))
    assert list(yv[:4] > 0) == [False, False, True, False]
    assert np.array_equal(R.bf16_bits(out).view(np.uint16), want)


@pytest.mark.parametrize("r", [2, 3])
@pytest.mark.parametrize("C", [3, 64])
def test_space_to_depth_bf16_is_the_fp32_permutation(ctx, r, C):
    rng = np.random.default_rng(r * 100 + C)
    x = torch.from_numpy(rng.standard_normal((3, 5 * r, 7 * r, C)).astype(np.float32)).to(BF16)
    got = ctx.space_to_depth_bf16(ctx.to_device(x), r)
    assert got.shape == (3, 5, 7, r * r * C)
    assert np.array_equal(R.bf16_bits(got), R.bf16_bits(R.s2d(x, r).contiguous()))
    assert np.array_equal(R.bf16_bits(got), R.bf16_bits(ctx.space_to_depth(ctx.to_device(x.float()), r).to(BF16)))


# ---------------------------------------------------------------------------------------------------------------- error paths
def test_error_paths_return_without_a_launch(ctx):
    x16 = ctx.to_device(torch.zeros((1, 4, 4, 8), dtype=BF16))
    x32 = ctx.to_device(np.zeros((1, 4, 4, 8), np.float32))
    w = ctx.to_device(np.zeros((3, 3, 8, 8), np.float32))
    dw, db = ctx.empty((3, 3, 8, 8)), ctx.empty((8,))
    lib, h, st = ctx.lib, ctx.h, ctx.stream()
    # the library: null pointers and K != 3
    assert lib.sr_conv2d_wgrad_bf16(h, None, 8, x16.data_ptr(), 8, 1, 4, 4, 8, 8, 3, 1.0, dw.data_ptr(), None, st) == L.SR_ERR_INVALID
    assert lib.sr_conv2d_wgrad_bf16(h, x16.data_ptr(), 8, x16.data_ptr(), 8, 1, 4, 4, 8, 8, 3, 1.0, None, None, st) == L.SR_ERR_INVALID
    for k in (1, 5):
        assert lib.sr_conv2d_wgrad_bf16(h, x16.data_ptr(), 8, x16.data_ptr(), 8, 1, 4, 4, 8, 8, k, 1.0, dw.data_ptr(), db.data_ptr(), st) == L.SR_ERR_INVALID
    assert lib.sr_conv2d_wgrad_bf16(h, x16.data_ptr(), 4, x16.data_ptr(), 8, 1, 4, 4, 8, 8, 3, 1.0, dw.data_ptr(), db.data_ptr(), st) == L.SR_ERR_INVALID   # stride < Cin
    assert lib.sr_conv2d_dev_bf16(h, None, 1, 4, 4, 8, w.data_ptr(), None, 3, 8, 0, 0, 1.0, None, 0.0, None, 0.0, 0, 1, x16.data_ptr(), st) == L.SR_ERR_INVALID
    assert lib.sr_conv2d_dev_bf16(h, x16.data_ptr(), 1, 4, 4, 8, None, None, 3, 8, 0, 0, 1.0, None, 0.0, None, 0.0, 0, 1, x16.data_ptr(), st) == L.SR_ERR_INVALID
    assert lib.sr_conv_prepack_bf16(h, None, 2, st) == L.SR_ERR_INVALID
    assert lib.sr_relu_bwd_bf16(h, x16.data_ptr(), None, x16.data_ptr(), 128, st) == L.SR_ERR_INVALID
    assert lib.sr_space_to_depth_bf16(h, None, 1, 2, 2, 8, 2, x16.data_ptr(), st) == L.SR_ERR_INVALID
    assert lib.sr_mse_clip_grad_bf16(h, x16.data_ptr(), None, 128, dw.data_ptr(), x16.data_ptr(), None, st) == L.SR_ERR_INVALID
    assert lib.sr_mse_clip_grad_bf16(h, x16.data_ptr(), x32.data_ptr(), 0, dw.data_ptr(), x16.data_ptr(), None, st) == L.SR_ERR_INVALID
    # the wrappers: fp32 tensors where bf16 is expected, a kernel size other than 3
    with pytest.raises(ValueError, match="dtype"):
        ctx.conv2d_dev_bf16(x32, w, None, 8)
    with pytest.raises(ValueError, match="dtype"):
        ctx.conv2d_wgrad_bf16(x32, x16)
    with pytest.raises(ValueError, match="dtype"):
        ctx.conv2d_wgrad_bf16(x16, x32)
    with pytest.raises(ValueError, match="3x3"):
        ctx.conv2d_wgrad_bf16(x16, x16, 5)
    with pytest.raises(ValueError, match="dtype"):
        ctx.relu_bwd_bf16(x32, x16)
    with pytest.raises(ValueError, match="dtype"):
        ctx.space_to_depth_bf16(x32, 2)
    with pytest.raises(ValueError, match="dtype"):
        ctx.mse_clip_grad_bf16(x32, x32)
    with pytest.raises(ValueError, match="dtype"):
        ctx.mse_clip_grad_bf16(x16, x16)
    with pytest.raises(ValueError, match="contiguous"):
        ctx.relu_bwd_bf16(x16.permute(0, 2, 1, 3), x16.permute(0, 2, 1, 3))
