"""The training backward kernels (csrc/train_ops.hip, the spectral loss of csrc/imgops.hip) one at a time against fp64 references, at the
trainers' shapes and at the edges where their index arithmetic can go wrong.

Every kernel gets two kinds of case:
  * exact integers: inputs in {-2..2} (or other small integers), so that every fp32 sum the kernel forms is an exact integer below 2^24 and
    the device result must be BITWISE the fp64 reference -- this pins tiles, halos, pixel splits, channel offsets and tie rules;
  * random data against the fp64 reference by rel-L2, at the bounds test_train_gpu.py uses (2e-6 for wgrad, 1e-5 for dgrad).  Where a new
    bound is needed it is derived next to the assert.

The regimes of the kernels are forced by the shapes whatever the CU count:
  * wgrad_partial_kernel (K = 1 / 5 / 9) splits its P = B*H*W pixels into slices of 2048, at most 64: P > 2048 gives several slices,
    P > 131072 reaches the cap (a slice then holds more than 2048 pixels);
  * wgrad3_tile_kernel runs ntile = B * ceil(H/8) * ceil(W/24) tiles over at most 64 pixel splits: ntile > 64 forces tiles_per_wg >= 2.
"""
import ctypes

import numpy as np
import pytest
import torch

from sr355 import _lib as L

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, size=shape).astype(np.float32)


def host(t):
    return t.cpu().numpy()


def wgrad_ref(x, dy, K):
    """fp64 kernel and bias gradient of a K x K SAME stride-1 conv: dW[ky,kx] = sum over pixels of x(shifted by the tap)^T dy."""
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    B, H, W, Cin = x.shape
    Cout = dy.shape[3]
    p = (K - 1) // 2
    xp = np.pad(x, ((0, 0), (p, p), (p, p), (0, 0)))
    d2 = dy.reshape(-1, Cout)
    dw = np.empty((K, K, Cin, Cout))
    for ky in range(K):
        for kx in range(K):
            dw[ky, kx] = xp[:, ky:ky + H, kx:kx + W, :].reshape(-1, Cin).T @ d2
    return dw, d2.sum(0)


def dgrad_ref(dz, w):
    """fp64 input gradient of a K x K SAME stride-1 conv with HWIO kernel w [K,K,Cin,Cout]: dX[q] = sum over taps of dZ[q - tap + p] W[tap]^T."""
    dz, w = np.asarray(dz, np.float64), np.asarray(w, np.float64)
    B, H, W, _ = dz.shape
    K = w.shape[0]
    p = (K - 1) // 2
    zp = np.pad(dz, ((0, 0), (p, p), (p, p), (0, 0)))
    dx = np.zeros((B, H, W, w.shape[2]))
    for ky in range(K):
        for kx in range(K):
            dx += zp[:, 2 * p - ky:2 * p - ky + H, 2 * p - kx:2 * p - kx + W, :] @ w[ky, kx].T
    return dx


def check_wgrad_exact(ctx, x, dy, K):
    dw, db = ctx.conv2d_wgrad(ctx.to_device(x), ctx.to_device(dy), K)
    rw, rb = wgrad_ref(x, dy, K)
    assert np.abs(rw).max() < 2 ** 24 and np.abs(rb).max() < 2 ** 24
    dw, db = host(dw).astype(np.float64), host(db).astype(np.float64)
    assert np.array_equal(dw, rw), (np.argwhere(dw != rw)[:5], np.abs(dw - rw).max())
    assert np.array_equal(db, rb), np.abs(db - rb).max()


def check_wgrad_random(ctx, x, dy, K):
    dw, db = ctx.conv2d_wgrad(ctx.to_device(x), ctx.to_device(dy), K)
    rw, rb = wgrad_ref(x, dy, K)
    assert rel_l2(host(dw), rw) <= 2e-6, rel_l2(host(dw), rw)
    assert rel_l2(host(db), rb) <= 2e-6, rel_l2(host(db), rb)


# ---- wgrad, per-tap kernel (K = 1 / 5 / 9: SRCNN 9-1-5) ----

PER_TAP = [
    (16, 24, 24, 3, 64, 9),       # SRCNN fit: batch 16 of 24 x 24 patches, P = 9216 -> five slices of 2048 pixels
    (16, 24, 24, 64, 32, 1),
    (16, 24, 24, 32, 3, 5),
    (4, 192, 192, 32, 32, 1),     # P = 147456 > 64 * 2048: the 64-slice cap, 2304 pixels per slice
]


@pytest.mark.parametrize("case", PER_TAP)
def test_wgrad_per_tap_kernel_exact_integers(ctx, case):
    B, H, W, Cin, Cout, K = case
    rng = np.random.default_rng(sum(case))
    check_wgrad_exact(ctx, ints(rng, (B, H, W, Cin)), ints(rng, (B, H, W, Cout)), K)


@pytest.mark.parametrize("case", PER_TAP)
def test_wgrad_per_tap_kernel_random(ctx, case):
    B, H, W, Cin, Cout, K = case
    rng = np.random.default_rng(sum(case) + 1)
    check_wgrad_random(ctx, rng.standard_normal((B, H, W, Cin)).astype(np.float32), rng.standard_normal((B, H, W, Cout)).astype(np.float32), K)


# ---- wgrad, 3x3 tile kernel (wgrad3_tile_kernel + wgrad_finish_kernel) ----

TILE3 = [
    (2, 37, 53, 32, 32),          # ragged H and W: partial 8 x 24 tiles on both edges
    (3, 1, 50, 16, 24),           # H = 1: only the centre row of taps sees data
    (3, 45, 1, 24, 16),           # W = 1
    (4, 24, 24, 3, 64),           # Cin = 3 (initial_conv): the scalar staging path for x
    (4, 24, 24, 64, 3),           # Cout = 3 (the generator's RGB conv): scalar staging for dy
    (2, 19, 29, 37, 45),          # Cin, Cout not multiples of 4: both operands scalar, ragged channel blocks
    (2, 19, 29, 36, 44),          # multiples of 4, not of 32: vector staging, ragged channel blocks
    (4, 96, 96, 64, 64),          # discriminator-like: ntile = 4 * 12 * 4 = 192 > 64 -> tiles_per_wg >= 3
]


@pytest.mark.parametrize("case", TILE3)
def test_wgrad3_tile_kernel_exact_integers(ctx, case):
    B, H, W, Cin, Cout = case
    rng = np.random.default_rng(sum(case))
    x, dy = ints(rng, (B, H, W, Cin)), ints(rng, (B, H, W, Cout))
    check_wgrad_exact(ctx, x, dy, 3)
    # two runs, the same bits (the splits are summed in a fixed order, no atomics) -- on random data, where the order would show
    xr, dyr = ctx.to_device(rng.standard_normal(x.shape).astype(np.float32)), ctx.to_device(rng.standard_normal(dy.shape).astype(np.float32))
    a, ab = ctx.conv2d_wgrad(xr, dyr, 3)
    b, bb = ctx.conv2d_wgrad(xr, dyr, 3)
    assert torch.equal(a, b) and torch.equal(ab, bb)


@pytest.mark.parametrize("case", TILE3)
def test_wgrad3_tile_kernel_random(ctx, case):
    B, H, W, Cin, Cout = case
    rng = np.random.default_rng(sum(case) + 1)
    check_wgrad_random(ctx, rng.standard_normal((B, H, W, Cin)).astype(np.float32), rng.standard_normal((B, H, W, Cout)).astype(np.float32), 3)


def test_wgrad3_one_pixel_images_only_the_centre_tap(ctx):
    """A 1 x 1 image: every tap but the centre reads the zero halo, so those eight taps must be exactly 0."""
    rng = np.random.default_rng(11)
    x, dy = rng.standard_normal((5, 1, 1, 8)).astype(np.float32), rng.standard_normal((5, 1, 1, 12)).astype(np.float32)
    dw, db = ctx.conv2d_wgrad(ctx.to_device(x), ctx.to_device(dy), 3)
    dw = host(dw)
    off = np.ones((3, 3), bool)
    off[1, 1] = False
    assert not np.any(dw[off]) and np.count_nonzero(dw[1, 1]) == dw[1, 1].size
    rw, rb = wgrad_ref(x, dy, 3)
    assert rel_l2(dw, rw) <= 2e-6 and rel_l2(host(db), rb) <= 2e-6


# ---- wgrad on channel-range views, as the dense-block backward calls it (gan_train.Tape.dense_block) ----

def _dense_views(g):
    """(C0, Ct, [(x channel count, dy channel count)]): conv5 reads all of F = [x | f1..f4] against dz5 (C0 channels), growth conv k reads
    the prefix cin = C0 + (k-1) g against dz (g channels)."""
    C0 = 64
    Ct = C0 + 4 * g
    return C0, Ct, [(Ct, C0)] + [(C0 + (k - 1) * g, g) for k in range(4, 0, -1)]


@pytest.mark.parametrize("g", [8, 32])
@pytest.mark.parametrize("exact", [True, False])
def test_wgrad_views_replay_the_dense_block(ctx, g, exact):
    B, H, W = 3, 24, 24
    C0, Ct, uses = _dense_views(g)
    rng = np.random.default_rng(g + exact)
    gen = (lambda s: ints(rng, s)) if exact else (lambda s: rng.standard_normal(s).astype(np.float32))
    F = gen((B, H, W, Ct))
    Fd = ctx.to_device(F)
    for cin, cout in uses:
        dz = gen((B, H, W, cout))
        dzd = ctx.to_device(dz)
        dw, db = ctx.conv2d_wgrad_view(Fd, 0, cin, dzd, 0, cout, 3)
        cw, cb = ctx.conv2d_wgrad(ctx.to_device(F[..., :cin].copy()), dzd, 3)
        assert torch.equal(dw, cw) and torch.equal(db, cb), (cin, cout)             # the view reads exactly what the dense copy holds
        rw, rb = wgrad_ref(F[..., :cin], dz, 3)
        if exact:
            assert np.array_equal(host(dw).astype(np.float64), rw) and np.array_equal(host(db).astype(np.float64), rb), (cin, cout)
        else:
            assert rel_l2(host(dw), rw) <= 2e-6 and rel_l2(host(db), rb) <= 2e-6, (cin, cout, rel_l2(host(dw), rw))


def test_wgrad_views_at_odd_channel_offsets(ctx):
    """x at channel offset 1 of a 40-channel buffer, dy at offset 3 of a 20-channel one: unaligned pointers, the scalar staging path."""
    rng = np.random.default_rng(5)
    xb, db_ = ints(rng, (2, 17, 29, 40)), ints(rng, (2, 17, 29, 20))
    dw, dbias = ctx.conv2d_wgrad_view(ctx.to_device(xb), 1, 35, ctx.to_device(db_), 3, 13, 3)
    cw, cb = ctx.conv2d_wgrad(ctx.to_device(xb[..., 1:36].copy()), ctx.to_device(db_[..., 3:16].copy()), 3)
    assert torch.equal(dw, cw) and torch.equal(dbias, cb)
    rw, rb = wgrad_ref(xb[..., 1:36], db_[..., 3:16], 3)
    assert np.array_equal(host(dw).astype(np.float64), rw) and np.array_equal(host(dbias).astype(np.float64), rb)
    xr, dr = rng.standard_normal((2, 17, 29, 40)).astype(np.float32), rng.standard_normal((2, 17, 29, 20)).astype(np.float32)
    dw, dbias = ctx.conv2d_wgrad_view(ctx.to_device(xr), 1, 35, ctx.to_device(dr), 3, 13, 3)
    rw, rb = wgrad_ref(xr[..., 1:36], dr[..., 3:16], 3)
    assert rel_l2(host(dw), rw) <= 2e-6 and rel_l2(host(dbias), rb) <= 2e-6


@pytest.mark.parametrize("k", [1, 5])
def test_wgrad_views_need_a_3x3_kernel(ctx, k):
    F = ctx.to_device(np.zeros((1, 4, 4, 16), np.float32))
    dz = ctx.to_device(np.zeros((1, 4, 4, 8), np.float32))
    with pytest.raises(ValueError):
        ctx.conv2d_wgrad_view(F, 0, 12, dz, 0, 8, k)
    with pytest.raises(ValueError):
        ctx.conv2d_wgrad_view(F, 4, 12, dz, 0, 8, k)


# ---- the dense block's in-place input-gradient accumulation: G[..., :cin] += conv(dz, rot(k)) ----

@pytest.mark.parametrize("g", [16, 32])
@pytest.mark.parametrize("exact", [True, False])
def test_dgrad_accumulates_in_place_into_the_prefix(ctx, g, exact):
    """Replays gan_train's backward loop for k = 4..1 on one buffer G: conv2d_dev_view(dz, rot=True, skip = the output range itself).  The
    channels at and past cin hold non-integer sentinels and must come back bitwise unchanged after every step.  (The trainer takes this path
    for growth widths that are whole 16-channel chunks of the fp32 conv; narrower ones are refused, see below.)"""
    B, H, W = 2, 19, 29
    C0 = 64
    Ct = C0 + 4 * g
    rng = np.random.default_rng(100 + g + exact)
    gen = (lambda s: ints(rng, s)) if exact else (lambda s: rng.standard_normal(s).astype(np.float32))
    G = gen((B, H, W, Ct))
    G[..., C0 + 3 * g:] = rng.standard_normal((B, H, W, g)).astype(np.float32) + 0.375        # slice 4: never written by these steps
    Gd = ctx.to_device(G)
    for k in range(4, 0, -1):
        cin = C0 + (k - 1) * g
        kk = gen((3, 3, cin, g)) if exact else (rng.standard_normal((3, 3, cin, g)) / np.sqrt(9 * g)).astype(np.float32)
        dz = gen((B, H, W, g))
        before = Gd.clone()
        ctx.conv2d_dev_view(ctx.to_device(dz), 0, g, ctx.to_device(kk), None, cin, Gd, 0, rot=True, skip_buf=Gd, skip_coff=0, beta1=1.0)
        assert torch.equal(Gd[..., cin:], before[..., cin:]), k
        prev = host(before[..., :cin]).astype(np.float64)
        want = prev + dgrad_ref(dz, kk)
        got = host(Gd[..., :cin]).astype(np.float64)
        if exact:
            assert np.abs(want).max() < 2 ** 24
            assert np.array_equal(got, want), (k, np.abs(got - want).max())
        else:
            # the dgrad bound on the increment; the sum with the skip rounds once more, by at most half an ulp of the result
            assert rel_l2(got - prev, want - prev) <= 1e-5, (k, rel_l2(got - prev, want - prev))
            assert rel_l2(got, want) <= 1e-5, (k, rel_l2(got, want))


def test_dgrad_view_refuses_a_growth_width_of_8(ctx):
    """growth 8 is no whole 16-channel chunk: conv2d_dev_view refuses it (the trainer runs such blocks conv by conv) and writes nothing."""
    rng = np.random.default_rng(8)
    G = ctx.to_device(rng.standard_normal((2, 5, 7, 96)).astype(np.float32))
    before = G.clone()
    kk = ctx.to_device(np.ones((3, 3, 88, 8), np.float32))
    with pytest.raises(ValueError):
        ctx.conv2d_dev_view(ctx.to_device(np.ones((2, 5, 7, 8), np.float32)), 0, 8, kk, None, 88, G, 0, rot=True, skip_buf=G, skip_coff=0, beta1=1.0)
    torch.cuda.synchronize()
    assert torch.equal(G, before)


# ---- element-wise ops ----

OPS = [L.ELT_AXPBY, L.ELT_RELU_BWD, L.ELT_LRELU_BWD, L.ELT_CLIP01_BWD, L.ELT_MUL, L.ELT_TANH_BWD, L.ELT_CLIP01, L.ELT_SIGN_DIFF]
ONE_OPERAND = (L.ELT_AXPBY, L.ELT_CLIP01)
ALPHA, BETA = np.float32(0.375), np.float32(-1.25)


def _boundary_operands(rng):
    """All pairs of boundary values (+-0, 0 and 1 exactly and their neighbours, +-1 for tanh, a == b), then random values."""
    f = np.float32
    vals = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(f(1), f(2)), np.nextafter(f(1), f(0)), 0.5, 2.0, -2.0, 1e-30, -3.25, 7.0], np.float32)
    a, b = np.meshgrid(vals, vals, indexing="ij")
    ra = rng.standard_normal(2000).astype(np.float32) * 2
    rb = rng.standard_normal(2000).astype(np.float32) * 2
    rb[::7] = ra[::7]                                              # a == b
    return np.concatenate([a.ravel(), ra]), np.concatenate([b.ravel(), rb])


def _check_elt(op, a, b, got):
    """Select ops and single products must be bitwise NumPy's fp32 result; AXPBY and TANH_BWD may be contracted into an fma, so they are held
    to the fp64 value within the two roundings an fp32 evaluation makes (2 * 2^-24 of the magnitudes involved)."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if op == L.ELT_AXPBY:
        ref = ALPHA * a64 + BETA * b64
        assert np.all(np.abs(got - ref) <= 2.0 ** -23 * (np.abs(ALPHA * a64) + np.abs(BETA * b64)))
        return
    if op == L.ELT_TANH_BWD:
        ref = a64 * (1 - b64 * b64)
        assert np.all(np.abs(got - ref) <= 2.0 ** -22 * np.abs(a64) * (1 + b64 * b64))
        assert np.all(got[np.abs(b) == 1] == 0)                    # 1 - b^2 is exactly 0 at b = +-1 with or without an fma
        return
    if op == L.ELT_CLIP01:
        want = np.minimum(np.maximum(a, np.float32(0)), np.float32(1))
        z = a == 0                                                 # fmax(-0, 0) may be either zero: the value, not the sign, is pinned there
        assert np.array_equal(got[z], np.zeros(int(z.sum()), np.float32))
        assert np.array_equal(got[~z].view(np.int32), want[~z].view(np.int32))
        return
    want = {
        L.ELT_RELU_BWD: np.where(b > 0, a, np.float32(0)),
        L.ELT_LRELU_BWD: np.where(b > 0, a, np.float32(0.2) * a),
        L.ELT_CLIP01_BWD: np.where((b >= 0) & (b <= 1), a, np.float32(0)),
        L.ELT_MUL: (ALPHA * a) * b,
        L.ELT_SIGN_DIFF: ALPHA * np.where(a > b, np.float32(1), np.where(a < b, np.float32(-1), np.float32(0))),
    }[op].astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (op, np.argwhere(got.view(np.int32) != want.view(np.int32))[:5])


@pytest.mark.parametrize("op", OPS)
def test_eltwise_boundary_operands(ctx, op):
    a, b = _boundary_operands(np.random.default_rng(op))
    bd = None if op == L.ELT_CLIP01 else ctx.to_device(b)
    got = host(ctx.eltwise(op, ctx.to_device(a), bd, float(ALPHA), float(BETA)))
    _check_elt(op, a, np.zeros_like(b) if bd is None else b, got)


@pytest.mark.parametrize("op", OPS)
def test_eltwise_view_keeps_to_its_channel_range(ctx, op):
    a, b = _boundary_operands(np.random.default_rng(50 + op))
    C = 5
    npix = len(a) // (2 * C) * 2
    a, b = a[:npix * C], b[:npix * C]                               # the boundary pairs come first and stay
    shape = (2, 1, npix // 2)
    rng = np.random.default_rng(op)
    abuf = rng.standard_normal(shape + (9,)).astype(np.float32)
    bbuf = rng.standard_normal(shape + (6,)).astype(np.float32)
    obuf = np.full(shape + (12,), -7.75, np.float32)               # o_cs = 12 > C: sentinels around the range [4, 9)
    abuf[..., 2:2 + C] = a.reshape(shape + (C,))
    bbuf[..., 1:1 + C] = b.reshape(shape + (C,))
    ad, bd, od = ctx.to_device(abuf), ctx.to_device(bbuf), ctx.to_device(obuf)
    two = op != L.ELT_CLIP01
    ctx.eltwise_view(op, ad, 2, bd if two else None, 1, od, 4, C, float(ALPHA), float(BETA))
    out = host(od)
    assert np.array_equal(out[..., :4], obuf[..., :4]) and np.array_equal(out[..., 4 + C:], obuf[..., 4 + C:])
    assert np.array_equal(host(ad), abuf) and np.array_equal(host(bd), bbuf)
    _check_elt(op, a, b if two else np.zeros_like(b), out[..., 4:4 + C].reshape(-1))
    # out aliasing a: the same range read and written in place
    ctx.eltwise_view(op, ad, 2, bd if two else None, 1, ad, 2, C, float(ALPHA), float(BETA))
    res = host(ad)
    assert np.array_equal(res[..., :2], abuf[..., :2]) and np.array_equal(res[..., 2 + C:], abuf[..., 2 + C:])
    assert np.array_equal(res[..., 2:2 + C].view(np.int32), out[..., 4:4 + C].view(np.int32))


def test_eltwise_error_paths(ctx):
    a = ctx.to_device(np.ones((2, 3, 4, 8), np.float32))
    b = ctx.to_device(np.ones((2, 3, 4, 8), np.float32))
    o = ctx.empty((2, 3, 4, 8))
    for bad in (-1, L.ELT_SIGN_DIFF + 1):
        with pytest.raises(ValueError):
            ctx.eltwise(bad, a, b)
        with pytest.raises(ValueError):
            ctx.eltwise_view(bad, a, 0, b, 0, o, 0, 8)
    for op in OPS:
        if op not in ONE_OPERAND:
            with pytest.raises(ValueError):
                ctx.eltwise(op, a)
            with pytest.raises(ValueError):
                ctx.eltwise_view(op, a, 0, None, 0, o, 0, 8)
    with pytest.raises(ValueError):
        ctx.eltwise_view(L.ELT_AXPBY, a, 1, None, 0, o, 0, 8)         # [1, 9) is outside the 8 channels
    # the C entry point checks the width itself: a 4-channel-wide view asked for 8 channels (the buffer is large enough either way)
    narrow = L.View(a.data_ptr(), 4, 0)
    wide = L.View(o.data_ptr(), 8, 0)
    rc = ctx.lib.sr_eltwise_views(ctx.h, L.ELT_AXPBY, ctypes.byref(narrow), None, 1.0, 0.0, ctypes.byref(wide), 12, 8, ctx.stream())
    assert rc == L.SR_ERR_INVALID
    rc = ctx.lib.sr_eltwise_views(ctx.h, L.ELT_AXPBY, ctypes.byref(wide), None, 1.0, 0.0, ctypes.byref(narrow), 12, 8, ctx.stream())
    assert rc == L.SR_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(a, torch.ones_like(a))


# ---- row softmax and its backward (the training attention: 576 tokens at 24 x 24, 2304 at 48 x 48) ----

def _softmax_rows(rng, rows, cols):
    s = (3 * rng.standard_normal((rows, cols))).astype(np.float32)
    q = rows // 5
    s[:q] += np.float32(80)                                        # large offsets: exp(s - max) must not see them
    s[q:2 * q] -= np.float32(80)
    s[2 * q:3 * q] = 0
    hot = rng.integers(0, cols, size=q)
    s[2 * q + np.arange(q), hot] = 60                              # one-hot rows: the others get exp(-60), still a normal fp32 number
    s[3 * q:3 * q + 2] = 5                                         # all-equal rows: exactly 1/cols
    return s


@pytest.mark.parametrize("cols", [1, 255, 256, 257, 576, 2304])
def test_softmax_rows_and_backward(ctx, cols):
    rows = 16 * 576 if cols == 576 else (512 if cols == 2304 else 1000)
    rng = np.random.default_rng(cols)
    s = _softmax_rows(rng, rows, cols)
    p = host(ctx.softmax_rows_(ctx.to_device(s)))
    s64 = s.astype(np.float64)
    e = np.exp(s64 - s64.max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    # bound, relative per element: the subtraction s - max rounds at most once (|s - max| <= ~30 outside the exact cases: 30 * 2^-24 = 1.8e-6),
    # expf ~2 ulp, the row sum of positive terms <= (9 sequential + 8 tree levels) ulp, the reciprocal and the product 2 ulp: ~3e-6 < 1e-5
    assert np.all(np.abs(p - ref) <= 1e-5 * ref), float((np.abs(p - ref) / ref).max())
    if cols == 1:
        assert np.all(p == 1)
    dp = rng.standard_normal((rows, cols)).astype(np.float32)
    dp[:rows // 7] = 0
    dp[np.arange(rows // 7), rng.integers(0, cols, size=rows // 7)] = 1          # one-hot upstream gradients
    ds = host(ctx.softmax_bwd(ctx.to_device(p), ctx.to_device(dp)))
    p64, dp64 = p.astype(np.float64), dp.astype(np.float64)
    dot = (p64 * dp64).sum(1, keepdims=True)
    ref = p64 * (dp64 - dot)
    # bound: the dot product's products and sums cost <= (1 + 9 + 8) ulp of sum p |dp|, dp - dot 1 ulp of |dp| + |dot|, the product 1 ulp:
    # ~20 * 2^-24 = 1.2e-6 of p (|dp| + sum p |dp|) per element
    scale = p64 * (np.abs(dp64) + (p64 * np.abs(dp64)).sum(1, keepdims=True))
    assert np.all(np.abs(ds - ref) <= 1e-5 * scale), float((np.abs(ds - ref) / np.maximum(scale, 1e-300)).max())
    if cols == 1:
        assert np.all(ds == 0)


# ---- spectral loss: mean | |fft2(a)| - |fft2(b)| | over (W, C) and its gradient ----

def _spectral_ref(a, b):
    at = torch.tensor(a.astype(np.float64), requires_grad=True)
    fa = torch.fft.fft2(at.to(torch.complex128))
    fb = torch.fft.fft2(torch.tensor(b.astype(np.float64)).to(torch.complex128))
    loss = torch.mean(torch.abs(torch.abs(fa) - torch.abs(fb)))
    loss.backward()
    return loss.item(), at.grad.numpy(), torch.abs(fa).detach().numpy(), torch.abs(fb).numpy()


@pytest.mark.parametrize("shape", [(16, 96, 96, 3), (4, 16, 1, 3), (4, 16, 2, 3), (4, 16, 3, 3), (4, 16, 7, 3), (2, 9, 97, 3), (4, 16, 192, 3)])
def test_spectral_l1_and_gradient(ctx, shape):
    rng = np.random.default_rng(shape[2])
    a = rng.uniform(-1, 1, shape).astype(np.float32)
    b = rng.uniform(-1, 1, shape).astype(np.float32)
    ad, bd = ctx.to_device(a), ctx.to_device(b)
    loss, grad, ma, mb = _spectral_ref(a, b)
    # forward: each bin's magnitude carries ~sqrt(W) * 2^-24 relative error from the direct W-point sums in fp32 (< 1e-6 at W = 192)
    assert abs(float(ctx.spectral_l1(ad, bd).item()) - loss) <= 1e-5 * loss
    got = host(ctx.spectral_l1_bwd(ad, bd, 0.75))
    # The gradient is sgn(|Fa| - |Fb|) * Fa / |Fa| per bin: where |Fa| and |Fb| are closer than the fp32 error of the magnitudes (~2^-24 sqrt(W)
    # of their row's scale, < 1e-6) the sign is a coin toss, and where |Fa| is tiny the phase is.  Rows (each row's gradient depends on that row
    # only) with a bin within 1e-4 of a tie, or with |Fa| below 3e-3 of the row's scale (a phase error < 1e-3 on that one bin), are left out --
    # a few per cent of them; the rest must agree to rel-L2 1e-5: the forward and inverse DFT in fp32 with fp32 twiddles cost ~2^-24 (sqrt(W)
    # + a few), < 2e-6 at W = 192.
    rows = ma.reshape(-1, shape[2] * 3)
    rms = np.sqrt((rows ** 2).mean(1))
    margin = np.abs(rows - mb.reshape(rows.shape)).min(1) / rms
    keep = (margin >= 1e-4) & (rows.min(1) >= 3e-3 * rms)
    assert keep.mean() >= 0.8, keep.mean()
    g2, r2 = got.reshape(len(keep), -1)[keep], 0.75 * grad.reshape(len(keep), -1)[keep]
    assert rel_l2(g2, r2) <= 1e-5, rel_l2(g2, r2)
    assert np.all(np.isfinite(got))
    # a == b: every sign is 0, so the gradient is exactly 0 (and the loss too)
    assert float(ctx.spectral_l1(ad, ad).item()) == 0.0
    z = host(ctx.spectral_l1_bwd(ad, ctx.to_device(a.copy()), 1.0))
    assert not np.any(z)


# ---- MaxPooling2D(2, 2) backward ----

def _maxpool_bwd_ref(x, dy):
    """torch's CPU max_pool2d backward in fp64 (NCHW-contiguous input): the gradient goes to the first maximum of the window in row-major order."""
    xt = torch.tensor(x.astype(np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    torch.nn.functional.max_pool2d(xt, 2).backward(torch.tensor(dy.astype(np.float64)).permute(0, 3, 1, 2).contiguous())
    return xt.grad.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("shape", [(2, 8, 6, 5), (3, 9, 11, 5), (2, 7, 8, 3), (1, 3, 5, 2), (4, 96, 96, 64)])
def test_maxpool2_bwd_ties_and_odd_edges(ctx, shape):
    B, H, W, C = shape
    rng = np.random.default_rng(H * W)
    x = np.maximum(ints(rng, shape, -2, 1), 0)                     # post-ReLU small integers: all-zero windows and ties everywhere
    x[x == 0] = np.where(rng.random(int((x == 0).sum())) < 0.5, np.float32(0), np.float32(-0.0))
    if H >= 2 and W >= 4:
        x[0, 0:2, 0:2, 0] = [[3, 3], [1, 0]]                       # equal maxima at window positions 0 and 1
        x[0, 0:2, 2:4, 0] = [[3, 1], [3, 0]]                       # 0 and 2
        if C > 1:
            x[0, 0:2, 0:2, 1] = [[1, 3], [0, 3]]                   # 1 and 3
            x[0, 0:2, 2:4, 1] = [[2, 2], [2, 2]]                   # all four
    dy = rng.standard_normal((B, H // 2, W // 2, C)).astype(np.float32)
    got = host(ctx.maxpool2_bwd(ctx.to_device(x), ctx.to_device(dy)))
    ref = _maxpool_bwd_ref(x, dy)
    assert np.array_equal(got.astype(np.float64), ref), np.argwhere(got != ref)[:5]
    if H % 2:
        assert not np.any(got[:, -1])
    if W % 2:
        assert not np.any(got[:, :, -1])
    # random values (no ties) as well
    xr = rng.standard_normal(shape).astype(np.float32)
    assert np.array_equal(host(ctx.maxpool2_bwd(ctx.to_device(xr), ctx.to_device(dy))).astype(np.float64), _maxpool_bwd_ref(xr, dy))


# ---- the stride-2 pick (SP_PICK2) and its adjoint zero_insert2 ----

def _tf_stride2_centres(n, k=3):
    """Input positions of the window centres of a TF Conv2D(k, strides=2, padding='SAME') along an axis of length n."""
    out = -(-n // 2)
    pad_top = max((out - 1) * 2 + k - n, 0) // 2
    return 2 * np.arange(out) - pad_top + (k - 1) // 2


@pytest.mark.parametrize("hw", [(8, 6), (7, 5), (8, 5), (7, 6), (1, 1), (2, 1), (1, 2), (96, 97)])
def test_pick2_and_zero_insert2_positions(ctx, hw):
    H, W = hw
    rng = np.random.default_rng(H * 100 + W)
    ys, xs = _tf_stride2_centres(H), _tf_stride2_centres(W)
    z = rng.standard_normal((3, H, W, 4)).astype(np.float32)
    pick = host(ctx.spatial_op(L.SP_PICK2, ctx.to_device(z)))
    assert np.array_equal(pick, z[:, ys][:, :, xs])
    g = rng.standard_normal(pick.shape).astype(np.float32)
    back = host(ctx.zero_insert2(ctx.to_device(g), H, W))
    want = np.zeros_like(z)
    want[:, ys[:, None], xs[None, :]] = g
    assert np.array_equal(back, want)


# ---- sr_matmul at the 2304-token products ----

BIG_MM = [(1, 2304, 2304, 8), (1, 2304, 32, 2304)]          # (batch, M, N, K): s = g f^T at 48 x 48 tokens, and o = beta h


@pytest.mark.parametrize("ta,tb", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("shape", BIG_MM)
def test_matmul_2304_tokens(ctx, shape, ta, tb):
    B, M, N, K = shape
    rng = np.random.default_rng(M + N + K + 2 * ta + tb)
    for exact in (True, False):
        gen = (lambda s: ints(rng, s)) if exact else (lambda s: rng.standard_normal(s).astype(np.float32))
        a = gen((B, K, M) if ta else (B, M, K))
        b = gen((B, N, K) if tb else (B, K, N))
        got = host(ctx.matmul(ctx.to_device(a), ctx.to_device(b), trans_a=ta, trans_b=tb, alpha=0.5))
        A = a.transpose(0, 2, 1) if ta else a
        Bm = b.transpose(0, 2, 1) if tb else b
        ref = 0.5 * np.matmul(A.astype(np.float64), Bm.astype(np.float64))
        assert got.shape == ref.shape == (B, M, N)
        if exact:                                                  # |sums| <= 4 K < 2^24, alpha a power of two
            assert np.array_equal(got.astype(np.float64), ref)
        else:
            assert np.abs(got - ref).max() <= 2e-6 * np.sqrt(K) * max(1.0, np.abs(ref).max())
