"""The device pieces of the bf16 RRDB trunk, one at a time (include/sr355.h: sr_conv2d_dev_views_bf16, sr_conv2d_wgrad_group_bf16, sr_eltwise_views_bf16):
against the same ops on contiguous copies of the same values (bit for bit where the same kernel runs) and against fp64 (tests/esrgan_mixed_ref.py)."""
import numpy as np
import pytest
import torch

import esrgan_mixed_ref as R
from sr355 import _lib as L

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN_BITS = 0x7FD5                       # a quiet NaN with a payload: planted in every channel no view covers


def f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def bf(rng, shape, scale=1.0):
    return torch.from_numpy((scale * rng.standard_normal(shape)).astype(np.float32)).to(BF16)


def plant(t, lo, hi):
    t.view(torch.int16)[..., lo:hi] = NAN_BITS
    return t


def planted_ok(t, lo, hi):
    return bool((t.view(torch.int16)[..., lo:hi] == NAN_BITS).all())


# ---------------------------------------------------------------------------------------------------------------- views conv
def conv_case(ctx, name, hw):
    """-> (run(): the views call, returns the output view; ref(): the contiguous call; v, bound: unrounded fp64 value and fp32 bound; planted(): the untouched
    channels still carry their pattern)."""
    H, W = hw
    B = 2
    rng = np.random.default_rng({"growth": 1, "conv5_folded": 2, "dgrad_inplace": 3}[name] + H)
    if name == "growth":                                        # conv 3 of a dense block: reads F[..., :96], writes F[..., 96:128] with ReLU
        w = (rng.standard_normal((3, 3, 96, 32)) * np.sqrt(2.0 / (9 * 96))).astype(np.float32)
        b = rng.uniform(-0.05, 0.05, 32).astype(np.float32)
        F = ctx.to_device(plant(bf(rng, (B, H, W, 192)), 96, 192))
        wd, bd = ctx.to_device(w), ctx.to_device(b)
        xc = F[..., :96].contiguous()

        def run():
            ctx.conv2d_dev_view_bf16(F, 0, 96, wd, bd, 32, F, 96, act="relu")
            return F[..., 96:128]
        ref = lambda: ctx.conv2d_dev_bf16(xc, wd, bd, 32, act="relu")
        kk = R.rb(R.t64(w))
        v = torch.relu(R.conv64(R.t64(xc), kk, R.t64(b)))
        bound = R.conv_bound(R.t64(xc), kk, R.t64(b))
        planted = lambda: planted_ok(F, 128, 192)
    elif name == "conv5_folded":                                # an RRDB's third block: 0.04 * conv5(F) + 0.2 * x + r_in into slice 0 of the next F
        w = (rng.standard_normal((3, 3, 192, 64)) * np.sqrt(2.0 / (9 * 192))).astype(np.float32)
        b = rng.uniform(-0.05, 0.05, 64).astype(np.float32)
        F = ctx.to_device(bf(rng, (B, H, W, 192)))
        Rin = ctx.to_device(plant(bf(rng, (B, H, W, 192)), 64, 192))
        Nx = ctx.to_device(plant(bf(rng, (B, H, W, 192)), 0, 192))
        wd, bd = ctx.to_device(w), ctx.to_device(b)
        xs, rs = F[..., :64].contiguous(), Rin[..., :64].contiguous()

        def run():
            ctx.conv2d_dev_view_bf16(F, 0, 192, wd, bd, 64, Nx, 0, alpha=0.04, skip1=(F, 0), beta1=0.2, skip2=(Rin, 0), beta2=1.0)
            return Nx[..., :64]
        ref = lambda: ctx.conv2d_dev_bf16(F, wd, bd, 64, alpha=0.04, skip1=xs, beta1=0.2, skip2=rs, beta2=1.0)
        kk = R.rb(R.t64(w))
        sk = (0.2 * R.t64(xs), R.t64(rs))
        v = 0.04 * R.conv64(R.t64(F), kk, R.t64(b)) + sk[0] + sk[1]
        bound = R.conv_bound(R.t64(F), kk, R.t64(b), 0.04, sk)
        planted = lambda: planted_ok(Nx, 64, 192) and planted_ok(Rin, 64, 192)
    else:                                                       # conv 4's input gradient: G[..., :128] += dgrad(dz_4), dz_4 a slice of the dz buffer
        w = (rng.standard_normal((3, 3, 128, 32)) * np.sqrt(2.0 / (9 * 128))).astype(np.float32)
        dz = ctx.to_device(plant(plant(bf(rng, (B, H, W, 128)), 0, 32), 64, 128))
        Gb = ctx.to_device(plant(bf(rng, (B, H, W, 192)), 128, 192))
        wd = ctx.to_device(w)
        xc, g0 = dz[..., 32:64].contiguous(), Gb[..., :128].contiguous()

        def run():
            ctx.conv2d_dev_view_bf16(dz, 32, 32, wd, None, 128, Gb, 0, rot=True, skip1=(Gb, 0), beta1=1.0)
            return Gb[..., :128]
        ref = lambda: ctx.conv2d_dev_bf16(xc, wd, None, 128, rot=True, skip1=g0, beta1=1.0)
        kk = R.rot(R.rb(R.t64(w)))
        v = R.conv64(R.t64(xc), kk) + R.t64(g0)
        bound = R.conv_bound(R.t64(xc), kk, None, 1.0, (R.t64(g0),))
        planted = lambda: planted_ok(Gb, 128, 192) and planted_ok(dz, 0, 32) and planted_ok(dz, 64, 128)
    return run, ref, v, bound, planted


@pytest.mark.parametrize("hw", [(12, 12), (9, 20)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", ["growth", "conv5_folded", "dgrad_inplace"])
def test_conv_views_bf16(ctx, name, hw):
    """The three epilogues the trunk uses, on channel ranges, against sr_conv2d_dev_bf16 on contiguous copies: bit for bit where conv_routes names the same
    kernel variant for both calls, and always within 2^-8 |v| + (9 Cin + 2) 2^-24 S of the unrounded fp64 value.  Channels no view covers carry a NaN
    pattern: it must stay where it is and must not reach the output."""
    run, ref, v, bound, planted = conv_case(ctx, name, hw)
    ctx.conv_routes(True)
    want = ref()
    r_ref = ctx.conv_routes(True)
    got = run().contiguous()
    r_got = ctx.conv_routes(False)
    print(f"{name} {hw}: route of the contiguous call {r_ref}, of the views call {r_got}")
    assert len(r_ref) == 1 and len(r_got) == 1 and "bf16" in r_got[0]
    assert planted(), "a channel outside every view was written"
    g64 = R.t64(got)
    assert bool(torch.isfinite(g64).all()), "a channel outside every read view reached the output"
    excess = float(((g64 - v).abs() - (2.0 ** -8 * v.abs() + bound)).max())
    print(f"{name} {hw}: worst |got - v| - bound {excess:.3e}")
    assert excess <= 0.0
    if name == "growth" and hw == (12, 12):
        assert r_ref == r_got
    if r_ref == r_got:
        assert np.array_equal(R.bf16_bits(got), R.bf16_bits(want))


def test_conv_views_bf16_refuses_what_it_cannot_address(ctx):
    rng = np.random.default_rng(0)
    F = ctx.to_device(bf(rng, (2, 12, 12, 192)))
    before = R.bf16_bits(F).copy()
    w48 = ctx.to_device(rng.standard_normal((3, 3, 48, 32)).astype(np.float32))
    w32 = ctx.to_device(rng.standard_normal((3, 3, 32, 32)).astype(np.float32))
    ctx.conv_routes(True)
    with pytest.raises(ValueError, match="32-channel chunks"):
        ctx.conv2d_dev_view_bf16(F, 0, 48, w48, None, 32, F, 96)                  # Cin 48: one chunk and a half
    with pytest.raises(ValueError, match="multiples of 8"):
        ctx.conv2d_dev_view_bf16(F, 4, 32, w32, None, 32, F, 96)                  # a view that starts 8 bytes into a pixel
    with pytest.raises(ValueError, match="multiples of 8"):
        ctx.conv2d_dev_view_bf16(F, 0, 32, w32, None, 32, F, 100)
    assert ctx.conv_routes(False) == []                                           # nothing was launched
    torch.cuda.synchronize()
    assert np.array_equal(R.bf16_bits(F), before)


# ---------------------------------------------------------------------------------------------------------------- grouped weight gradient
C0, G = 64, 32
PAIRS = [2 * 1, 3 * 1, 4 * 1, 5 * 1, 6 * 2]                     # (32-cin blocks) x (32-cout blocks) of a G = 32 dense block's five layers
PLANT = 12345.0


def block_operands(ctx, B, H, W, seed):
    rng = np.random.default_rng(seed)
    F, dz, dY = (ctx.to_device(bf(rng, (B, H, W, c))) for c in (C0 + 4 * G, 4 * G, C0))
    return F, dz, dY


def block_jobs(F, dz, dY, flat):
    """The five jobs of a dense block, dw / db views of one flat tensor, 8 planted floats between consecutive arrays -> (jobs, [(x, dy, scale, dw, db)])."""
    jobs, parts, o = [], [], 8
    for k in range(1, 6):
        cin, cout = (C0 + (k - 1) * G, G) if k < 5 else (C0 + 4 * G, C0)
        dw = flat[o:o + 9 * cin * cout].view(3, 3, cin, cout)
        o += 9 * cin * cout + 8
        db = flat[o:o + cout]
        o += cout + 8
        scale = 1.0 if k < 5 else 0.2
        dyb, dyo = (dz, (k - 1) * G) if k < 5 else (dY, 0)
        jobs.append((F, 0, cin, dyb, dyo, cout, scale, dw, db))
        parts.append((F[..., :cin].contiguous(), dyb[..., dyo:dyo + cout].contiguous(), scale, dw, db))
    assert o <= flat.numel()
    return jobs, parts


def flat_bucket(ctx):
    n = 8 + sum(9 * (C0 + (k - 1) * G) * G + G + 16 for k in range(1, 5)) + 9 * (C0 + 4 * G) * C0 + C0 + 16
    return torch.full((n,), PLANT, dtype=torch.float32, device=ctx.torch_device)


def untouched(flat, parts):
    """Every element of the flat tensor outside the jobs' arrays still carries the planted value."""
    keep = torch.ones_like(flat, dtype=torch.bool)
    for _, _, _, dw, db in parts:
        for a in (dw, db):
            if a is not None:
                o = a.storage_offset() - flat.storage_offset()
                keep[o:o + a.numel()] = False
    return bool((flat[keep] == PLANT).all()) and int(keep.sum()) >= 8 * 11


def test_wgrad_group_small_is_the_single_launches_bit_for_bit(ctx):
    """B = 2, 12 x 12: 4 tiles.  The single launches split the pixels 4 ways, and so does the group (its 26 pairs still leave ceil(1.5 CUs / 26) >= 4): every
    workgroup owns one tile in both, so both add the same partial tiles in the same order."""
    cu = ctx.cu_count()
    ntile = 2 * 2 * 1
    for pairs in PAIRS + [sum(PAIRS)]:
        assert min((3 * cu // 2 + pairs - 1) // pairs, 64) >= ntile, (cu, pairs)
    assert sum(PAIRS) == 26
    F, dz, dY = block_operands(ctx, 2, 12, 12, 1)
    flat = flat_bucket(ctx)
    jobs, parts = block_jobs(F, dz, dY, flat)
    ctx.conv2d_wgrad_group_bf16(jobs)
    assert untouched(flat, parts)
    for x, dy, scale, dw, db in parts:
        rw, rbias = ctx.conv2d_wgrad_bf16(x, dy, 3, scale=scale)
        assert np.array_equal(f32_bits(dw), f32_bits(rw)) and np.array_equal(f32_bits(db), f32_bits(rbias)), tuple(dw.shape)


def test_wgrad_group_many_tiles_against_fp64(ctx):
    """B = 6, 20 x 40: 54 tiles, several per workgroup, ragged on the right and at the bottom.  rel-L2 <= 2e-6 against fp64 on the stored operands (the bar
    of tests/test_edsr_mixed_gpu.py); a second run gives the same bits; one job alone gives sr_conv2d_wgrad_bf16's bits."""
    F, dz, dY = block_operands(ctx, 6, 20, 40, 2)
    flat = flat_bucket(ctx)
    jobs, parts = block_jobs(F, dz, dY, flat)
    ctx.conv2d_wgrad_group_bf16(jobs)
    first = f32_bits(flat).copy()
    assert untouched(flat, parts)
    for x, dy, scale, dw, db in parts:
        rw, rbias = R.wgrad64(R.t64(x), R.t64(dy), scale)
        ew, eb = R.rel_l2(dw, rw), R.rel_l2(db, rbias)
        print(f"wgrad group {tuple(dw.shape)}: rel-L2 dw {ew:.3e} db {eb:.3e}")
        assert ew <= 2e-6 and eb <= 2e-6
    flat.fill_(PLANT)
    ctx.conv2d_wgrad_group_bf16(jobs)
    assert np.array_equal(f32_bits(flat), first)
    # one job alone: the third layer, on the views and through the single-layer entry point on contiguous copies
    x, dy, scale, dw, db = parts[2]
    flat.fill_(PLANT)
    ctx.conv2d_wgrad_group_bf16([jobs[2]])
    rw, rbias = ctx.conv2d_wgrad_bf16(x, dy, 3, scale=scale)
    assert np.array_equal(f32_bits(dw), f32_bits(rw)) and np.array_equal(f32_bits(db), f32_bits(rbias))
    assert untouched(flat, [parts[2]])


def test_wgrad_group_scalar_staging_path(ctx):
    """A view that starts 8 bytes into a pixel, channel counts that are no multiples of 8, no bias gradient: the element-wise staging path."""
    rng = np.random.default_rng(3)
    xb, dyb = ctx.to_device(bf(rng, (2, 12, 12, 48))), ctx.to_device(bf(rng, (2, 12, 12, 24)))
    flat = torch.full((8 + 9 * 40 * 24 + 8,), PLANT, dtype=torch.float32, device=ctx.torch_device)
    dw = flat[8:8 + 9 * 40 * 24].view(3, 3, 40, 24)
    ctx.conv2d_wgrad_group_bf16([(xb, 4, 40, dyb, 0, 24, 1.0, dw, None)])
    rw, _ = R.wgrad64(R.t64(xb[..., 4:44]), R.t64(dyb))
    e = R.rel_l2(dw, rw)
    print(f"wgrad group scalar path: rel-L2 dw {e:.3e}")
    assert e <= 2e-6
    assert bool((flat[:8] == PLANT).all()) and bool((flat[-8:] == PLANT).all())


def test_wgrad_group_refuses_empty_and_oversized_groups(ctx):
    F, dz, dY = block_operands(ctx, 2, 12, 12, 4)
    flat = flat_bucket(ctx)
    jobs, _ = block_jobs(F, dz, dY, flat)
    with pytest.raises(ValueError, match="1 to 8 jobs"):
        ctx.conv2d_wgrad_group_bf16((jobs + jobs)[:9])
    arr = (L.WgradJob * 1)()
    assert ctx.lib.sr_conv2d_wgrad_group_bf16(ctx.h, arr, 0, 2, 12, 12, ctx.stream()) == L.SR_ERR_INVALID
    assert ctx.lib.sr_conv2d_wgrad_group_bf16(ctx.h, None, 1, 2, 12, 12, ctx.stream()) == L.SR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((flat == PLANT).all())                                              # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- element-wise on views
def test_relu_bwd_views_is_a_select_on_bits(ctx):
    rng = np.random.default_rng(5)
    Gb, F = bf(rng, (2, 9, 20, 192)), bf(rng, (2, 9, 20, 192))
    Fb = F.view(torch.int16)
    Fb[0, 0, :8, 96] = torch.tensor([0x0000, -0x8000, 0x0001, -0x7FFF, 0x7F80, -0x0080, 0x7FC0, 0x007F], dtype=torch.int16)   # +0 -0 +/-subnormal +/-inf NaN subnormal
    out = plant(bf(rng, (2, 9, 20, 128)), 0, 128)
    Gd, Fd, od = ctx.to_device(Gb), ctx.to_device(F), ctx.to_device(out)
    ctx.eltwise_view_bf16(L.ELT_RELU_BWD, Gd, 96, Fd, 96, od, 32, 32)
    fb = Fb[..., 96:128].int()
    pos = (fb > 0) & (fb <= 0x7F80)                                                # sign clear, not zero, not NaN
    want = torch.where(pos, Gb.view(torch.int16)[..., 96:128], torch.zeros((), dtype=torch.int16))
    assert np.array_equal(R.bf16_bits(od[..., 32:64].contiguous()), want.numpy())
    assert planted_ok(od, 0, 32) and planted_ok(od, 64, 128)


def test_relu_bwd_views_past_the_grid_cap(ctx):
    """65 535 workgroups of 256 threads: 18 M elements make every thread take a second round."""
    n = 1500
    assert n * n * 8 > 65535 * 256
    gen = torch.Generator(device=ctx.torch_device).manual_seed(6)
    a = torch.randn((1, n, n, 8), generator=gen, device=ctx.torch_device).to(BF16)
    b = torch.randn((1, n, n, 8), generator=gen, device=ctx.torch_device).to(BF16)
    out = torch.empty_like(a)
    ctx.eltwise_view_bf16(L.ELT_RELU_BWD, a, 0, b, 0, out, 0, 8)
    assert torch.equal(out.view(torch.int16), torch.where(b > 0, a, torch.zeros((), dtype=BF16, device=a.device)).view(torch.int16))


@pytest.mark.parametrize("coef", [(1.0, 1.0), (0.5, 2.0)])
def test_axpby_views_rounds_once(ctx, coef):
    """alpha * a + beta * b with power-of-two coefficients: the products are exact.  The sum of two values of 8 significant bits either fits fp32's 24 bits
    (exponents at most 15 apart: exact) or its smaller term is below 2^-8 of a bf16 step of the larger, so the fp32 sum lies far from every bf16 rounding
    boundary: bf16(fp32 sum) is the correctly rounded sum -- element for element rb of the fp64 value."""
    rng = np.random.default_rng(7)
    a, b = bf(rng, (2, 9, 20, 64)), bf(rng, (2, 9, 20, 192), scale=0.03)
    out = plant(bf(rng, (2, 9, 20, 128)), 0, 128)
    ad, bd, od = ctx.to_device(a), ctx.to_device(b), ctx.to_device(out)
    ctx.eltwise_view_bf16(L.ELT_AXPBY, ad, 0, bd, 64, od, 64, 64, *coef)
    want = R.rb(coef[0] * a.double() + coef[1] * b.double()[..., 64:128])
    assert torch.equal(R.t64(od[..., 64:128]), want)
    assert planted_ok(od, 0, 64)
    with pytest.raises(ValueError):
        ctx.eltwise_view_bf16(L.ELT_LRELU_BWD, ad, 0, ad, 0, od, 0, 64)
