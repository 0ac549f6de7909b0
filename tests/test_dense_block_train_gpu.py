"""Training a G = 8 dense block on the LDS-resident kernels (csrc/dense_block_train.hip), on the GPU:
1. the device packer against its NumPy restatement and against the inference kernel's own packing;
2. the forward on NHWC buffers, every growth slice and the block output per element against fp64 on the device's own stored inputs;
3. the backward, teacher-forced stage by stage through the kernel's stage dump; planted NaNs; exact integers;
4. an image's bits do not depend on the batch, the workgroup cap, the stage dump or what the LDS held before;
5. the grouped weight-gradient kernel at the block's channel counts;
6. the trainer end to end (pixel_step's gradient, train_step beside the fp32 trainer);
7. the public interface.
References: tests/dense_block_train_ref.py.  The per-element bar is 3.26's (esrgan_mixed_ref.check_convs): within 2^-8 |v| + (9 Cin + 2) 2^-24 S of the fp64 value, at
most 1e-2 of the elements off the once-rounded reference, each by one bf16 step."""
import numpy as np
import pytest
import torch

import dense_block_train_ref as R
from esrgan_mixed_ref import check_convs
from edsr_mixed_ref import rel_l2, t64, wgrad64
from sr355 import Context
from sr355 import _lib as L

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
NAN_BITS = 0x7FD5                       # a quiet NaN with a payload
FWD, BWD, PACK = "dense_block_fwd_lds<bf16,g8,nhwc>", "dense_block_bwd_lds<bf16,g8>", "dense_block_pack_dev<g8>"


def widest(h, fits):
    w = 1
    while fits(h, w + 1):
        w += 1
    assert fits(h, w) and not fits(h, w + 1)
    return w


# the forward kernel's own edge cases; W = None: the widest image at that height -- for the forward the edge of the LDS, read from sr_dense_block_lds_bytes, for the
# backward the narrower of that and the kernel's own pixel bound, both read from the library
CASES = R.CASES + [(2, 24, None, 0)]


def resolve(case, backward):
    B, H, W, cap = case
    if W is None:
        W = widest(H, Context.dense_block_train_fits if backward else (lambda h, w: Context.dense_block_lds_bytes(8, h, w) > 0))
    return B, H, W, cap


def case_id(c):
    return "x".join("widest" if v is None else str(v) for v in c)


@pytest.fixture()
def capped(ctx):
    yield ctx
    ctx.set_fused(ctx.FUSED_ALL, 0)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def dev_bf(ctx, a):
    return ctx.to_device(np.ascontiguousarray(a, np.float32), BF16)


def planted(ctx, shape):
    t = ctx.empty(shape, BF16)
    t.view(torch.int16).fill_(NAN_BITS)
    return t


def still_planted(t, lo, hi):
    return bool((t.view(torch.int16)[..., lo:hi] == NAN_BITS).all())


_PACKS = {}


def packed(ctx, seeds=(7, 8, 9)):
    """Three blocks packed by ONE launch: (weights per block, fwd, bias, bwd); block 0 is the tests' block (R.block_weights(7))."""
    if seeds not in _PACKS:
        wss = [R.block_weights(s) for s in seeds]
        dev = [([ctx.to_device(k) for k, _ in ws], [ctx.to_device(b) for _, b in ws]) for ws in wss]
        table = ctx.dense_block_pack_table(dev)
        fwd, bias, bwd = ctx.dense_block_pack_buffers(len(seeds))
        for t in (fwd, bwd):
            t.fill_(0xA5)                                      # stale memory: the packer writes every byte, padding included
        bias.fill_(float("nan"))
        ctx.dense_block_pack_dev(table, fwd, bias, bwd)
        _PACKS[seeds] = (wss, fwd, bias, bwd, dev, table)
    return _PACKS[seeds][:4]


# ------------------------------------------------------------------------------------------------ 1. the packer
def test_device_packer_is_the_numpy_restatement(ctx):
    wss, fwd, bias, bwd = packed(ctx)
    for i, ws in enumerate(wss):
        f_np, b_np = R.pack_forward_np(ws)
        assert np.array_equal(fwd[i].cpu().numpy().view(np.uint16).reshape(207, 64, 8), f_np), i
        assert np.array_equal(bias[i].cpu().numpy().view(np.uint32), b_np.view(np.uint32)), i
        assert np.array_equal(bwd[i].cpu().numpy().view(np.uint16).reshape(288, 64, 8), R.pack_backward_np(ws)), i


def test_forward_half_gives_the_bits_of_the_models_own_packing(capped):
    """sr_model_finalize packs the same weights on the host for the inference kernel; its packed image cannot be read back, so the two are compared through the
    kernel they feed: the same body on the same values gives the same bits, growth slices and block output."""
    ctx = capped
    from sr355 import Model
    from sr355.weights import bf16_rounded, init_weights
    m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=1, growth_channels=8, use_attention=False, ctx=ctx)
    w = bf16_rounded(init_weights(m.layer_shapes(), seed=5100))
    m.set_weights(w)
    x = np.random.default_rng(3).uniform(-1, 1, (3, 24, 24, 3)).astype(np.float32)
    name = "rrdb_0_dense1"
    names = ["initial_conv"] + [f"{name}_conv{k}" for k in range(1, 6)]
    ctx.set_fused(ctx.FUSED_ALL, 0)
    ctx.profile_begin()
    _, taps = m.forward_with_taps(ctx.to_device(x, BF16), names)
    assert "dense_block_lds<bf16,g8>" in {r["kernel"] for r in ctx.profile_end()}
    ws = [w[f"{name}_conv{k}"] for k in range(1, 6)]
    dev = [([ctx.to_device(k) for k, _ in ws], [ctx.to_device(b) for _, b in ws])]
    fwd, bias, bwd = ctx.dense_block_pack_buffers(1)
    ctx.dense_block_pack_dev(ctx.dense_block_pack_table(dev), fwd, bias, bwd)
    F = planted(ctx, (3, 24, 24, 96))
    F[..., :64] = taps["initial_conv"].to(BF16)
    out = ctx.empty((3, 24, 24, 64), BF16)
    ctx.dense_block_fwd_bf16(fwd[0], bias[0], F, out, alpha=0.2, beta1=1.0)
    for k in range(1, 5):
        assert np.array_equal(bits(F[..., 64 + 8 * (k - 1):64 + 8 * k]), bits(taps[f"{name}_conv{k}"].to(BF16))), k
    assert np.array_equal(bits(out), bits(taps[f"{name}_conv5"].to(BF16)))


# ------------------------------------------------------------------------------------------------ 2. forward
def run_forward(ctx, B, H, W, cap, a5, bx, with_rin):
    wss, fwd, bias, _ = packed(ctx)
    x, r_in, _ = R.case_inputs(B, H, W)
    F = planted(ctx, (B, H, W, 96))
    F[..., :64] = dev_bf(ctx, x)
    nxt = planted(ctx, (B, H, W, 96))                            # the next block's F: the kernel owns its channels [0, 64) only
    Rin = planted(ctx, (B, H, W, 96))
    Rin[..., :64] = dev_bf(ctx, r_in)
    ctx.set_fused(ctx.FUSED_ALL, cap)
    ctx.dense_block_fwd_bf16(fwd[0], bias[0], F, nxt, skip2=(Rin, 0) if with_rin else None, alpha=a5, beta1=bx, beta2=1.0 if with_rin else 0.0)
    return wss[0], x, r_in if with_rin else None, F, nxt


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("epilogue", [(0.2, 1.0, False), (0.04, 0.2, True)], ids=["x_skip", "rrdb_close"])
def test_forward_per_element(capped, case, epilogue):
    ctx = capped
    B, H, W, cap = case = resolve(case, False)
    a5, bx, with_rin = epilogue
    ws, x, r_in, F, nxt = run_forward(ctx, B, H, W, cap, a5, bx, with_rin)
    assert np.array_equal(bits(F[..., :64]), bits(dev_bf(ctx, x)))             # the input channels are read, never written
    assert still_planted(nxt, 64, 96)
    assert not torch.isnan(F.float()).any() and not torch.isnan(nxt[..., :64].float()).any()
    check_convs(R.forward_checks(ws, F.float(), nxt[..., :64].float(), a5, bx, r_in), what=f"{case_id(case)} a5={a5}")


# ------------------------------------------------------------------------------------------------ 3. backward
_FWD = {}


def stored_F(ctx, B, H, W):
    """The block's stored F of a case, from the forward kernel (shared by the backward tests; never modified)."""
    if (B, H, W) not in _FWD:
        _, _, _, F, _ = run_forward(ctx, B, H, W, 0, 0.2, 1.0, False)
        _FWD[(B, H, W)] = F
    return _FWD[(B, H, W)]


def run_backward(ctx, F, dY_np, cap, a5, bx, dump=True, block=0):
    _, _, _, bwd = packed(ctx)
    B, H, W, _ = F.shape
    dYb = planted(ctx, (B, H, W, 96))                            # dY as the first 64 channels of a wider buffer, as a drin / dX of another block may be
    dYb[..., :64] = dev_bf(ctx, dY_np)
    dz = planted(ctx, (B, H, W, 32))
    dXb = planted(ctx, (B, H, W, 96))
    stages = planted(ctx, (4, B, H, W, 96)) if dump else None
    ctx.set_fused(ctx.FUSED_ALL, cap)
    ctx.dense_block_bwd_bf16(bwd[block], dYb, F, a5, bx, dz, dXb, stages=stages)
    return dYb, dz, dXb, stages


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("epilogue", [(0.2, 1.0), (0.04, 0.2)], ids=["x_skip", "rrdb_close"])
def test_backward_teacher_forced(capped, case, epilogue):
    ctx = capped
    B, H, W, cap = case = resolve(case, True)
    a5, bx = epilogue
    ws = packed(ctx)[0][0]
    F = stored_F(ctx, B, H, W)
    Fb = bits(F).copy()
    _, _, dY = R.case_inputs(B, H, W)
    dYb, dz, dXb, stages = run_backward(ctx, F, dY, cap, a5, bx)
    assert np.array_equal(bits(F), Fb) and np.array_equal(bits(dYb[..., :64]), bits(dev_bf(ctx, dY)))      # inputs untouched
    assert still_planted(dXb, 64, 96) and still_planted(dYb, 64, 96)                                     # what the kernel does not own
    for name, t in (("dz", dz), ("dX", dXb[..., :64]), ("stages", stages)):
        assert not torch.isnan(t.float()).any(), name
    convs, exact = R.backward_checks(ws, F.float(), dY, stages.float(), dz.float(), dXb[..., :64].float(), a5, bx)
    for label, got, ref in exact:
        assert np.array_equal(bits(got.to(BF16)), bits(ref.to(BF16))), label                            # a select on bits, +0 where off
    check_convs(convs, what=f"{case_id(case)} a5={a5}")


def test_backward_exact_integers(capped):
    """Small-integer kernels, F signs and gradients: every sum is an integer below 2^8 in magnitude, so every stage and dX equal the fp64 integers exactly
    (a5 = bx = 1: no scale that is not a power of two)."""
    ctx = capped
    B, H, W = 3, 13, 21
    rng = np.random.default_rng(11)
    sparse = lambda shape, p: (rng.integers(-1, 2, shape) * (rng.random(shape) < p)).astype(np.float32)
    ws = [(sparse((3, 3, R.CIN[i], R.COUT[i]), 0.1 if i < 4 else 0.125), np.zeros(R.COUT[i], np.float32)) for i in range(5)]      # (the fp64 reference's largest |value| is 75)
    dev = [([ctx.to_device(k) for k, _ in ws], [ctx.to_device(b) for _, b in ws])]
    fwd, bias, bwd = ctx.dense_block_pack_buffers(1)
    ctx.dense_block_pack_dev(ctx.dense_block_pack_table(dev), fwd, bias, bwd)
    F = dev_bf(ctx, rng.integers(-1, 2, (B, H, W, 96)).astype(np.float32))
    dY = sparse((B, H, W, 64), 0.125)
    dYd, dz, dX = dev_bf(ctx, dY), planted(ctx, (B, H, W, 32)), planted(ctx, (B, H, W, 64))
    stages = planted(ctx, (4, B, H, W, 96))
    ctx.dense_block_bwd_bf16(bwd[0], dYd, F, 1.0, 1.0, dz, dX, stages=stages)
    st, dz64, dX64 = R.block_backward(ws, F.float(), dY, 1.0, 1.0)
    largest = max(float(s.abs().max()) for s in st.values())
    assert largest < 256 and float(dX64.abs().max()) < 256, largest                  # the reference itself never rounded
    assert torch.equal(t64(dX), dX64) and torch.equal(t64(dz), dz64)
    assert torch.equal(t64(stages[0]), st[5])
    for j, k in ((1, 4), (2, 3), (3, 2)):
        assert torch.equal(t64(stages[j])[..., :R.CIN[k - 1]], st[k][..., :R.CIN[k - 1]]), k
    assert float(dX64.abs().max()) > 8                                                # ... and the sums are not trivial


# ------------------------------------------------------------------------------------------------ 4. independence
def test_an_images_bits_do_not_depend_on_its_company(capped):
    ctx = capped
    B, H, W = 5, 24, 24
    F = stored_F(ctx, B, H, W)
    _, _, dY = R.case_inputs(B, H, W)
    _, dz0, dX0, _ = run_backward(ctx, F, dY, 0, 0.2, 1.0, dump=False)
    ref = (bits(dz0).copy(), bits(dX0[..., :64]).copy())

    def same(dz, dX, sel=slice(None), what=""):
        assert np.array_equal(bits(dz), ref[0][sel]) and np.array_equal(bits(dX[..., :64]), ref[1][sel]), what
    for cap in (1, 2, 3):                                                            # several images per workgroup
        _, dz, dX, _ = run_backward(ctx, F, dY, cap, 0.2, 1.0, dump=False)
        same(dz, dX, what=f"cap {cap}")
    _, dz, dX, _ = run_backward(ctx, F, dY, 2, 0.2, 1.0, dump=True)                  # the stage dump on
    same(dz, dX, what="dump")
    for i in (0, 4):                                                                 # alone in its batch
        _, dz, dX, _ = run_backward(ctx, F[i:i + 1].contiguous(), dY[i:i + 1], 0, 0.2, 1.0, dump=False)
        same(dz, dX, slice(i, i + 1), f"image {i} alone")
    # what the LDS held before: one workgroup runs an image of NaNs and Infs first, then image 2
    F2 = torch.cat([F[1:2], F[2:3]]).contiguous()
    dirty = np.concatenate([np.full_like(dY[:1], np.inf), dY[2:3]])
    dirty[0, ::2] = np.nan
    _, dz, dX, _ = run_backward(ctx, F2, dirty, 1, 0.2, 1.0, dump=False)
    same(dz[1:2], dX[1:2], slice(2, 3), "after a dirty image")


def test_forward_bits_do_not_depend_on_the_batch_or_the_cap(capped):
    ctx = capped
    _, _, _, F0, n0 = run_forward(ctx, 5, 24, 24, 0, 0.04, 0.2, True)
    for cap in (1, 2):
        _, _, _, F, n = run_forward(ctx, 5, 24, 24, cap, 0.04, 0.2, True)
        assert np.array_equal(bits(F), bits(F0)) and np.array_equal(bits(n[..., :64]), bits(n0[..., :64])), cap


# ------------------------------------------------------------------------------------------------ 5. weight gradients
def test_grouped_weight_gradients_at_the_blocks_widths(ctx):
    """One grouped call at (Cin, Cout) = (64, 8), (72, 8), (80, 8), (88, 8), (96, 64): against fp64 (rel-L2 <= 2e-6, 3.26's bar) and bit for bit the five
    single-job calls."""
    B, H, W = 2, 13, 21
    rng = np.random.default_rng(5)
    F = dev_bf(ctx, rng.normal(0, 1, (B, H, W, 96)))
    dz = dev_bf(ctx, rng.normal(0, 1, (B, H, W, 32)))
    dY = dev_bf(ctx, rng.normal(0, 1, (B, H, W, 64)))
    a5 = 0.2
    shapes = [(R.CIN[i], R.COUT[i]) for i in range(5)]

    def outs():
        return [(planted(ctx, (3, 3, ci, co)).float(), planted(ctx, (co,)).float()) for ci, co in shapes]

    def jobs(o):
        js = [(F, 0, R.CIN[k], dz, 8 * k, 8, 1.0) + o[k] for k in range(4)]
        return js + [(F, 0, 96, dY, 0, 64, a5) + o[4]]
    grouped = outs()
    ctx.conv2d_wgrad_group_bf16(jobs(grouped))
    single = outs()
    for j in jobs(single):
        ctx.conv2d_wgrad_group_bf16([j])
    for i, (ci, co) in enumerate(shapes):
        x64, dy64 = t64(F.float())[..., :ci], (t64(dz.float())[..., 8 * i:8 * i + 8] if i < 4 else t64(dY.float()))
        dw, db = wgrad64(x64, dy64, 1.0 if i < 4 else a5)
        ew, eb = rel_l2(grouped[i][0], dw), rel_l2(grouped[i][1], db)
        print(f"wgrad ({ci}, {co}): rel-L2 dw {ew:.3e} db {eb:.3e}")
        assert ew <= 2e-6 and eb <= 2e-6, (ci, co)
        for g, s in zip(grouped[i], single[i]):
            assert np.array_equal(g.cpu().numpy().view(np.uint32), s.cpu().numpy().view(np.uint32)), (ci, co)


# ------------------------------------------------------------------------------------------------ 6. the trainer end to end
NB, SCALE = 2, R.SCALE                   # x2, two RRDBs (six dense blocks), G = 8, attention, batch 2 of 12 x 12


def taped_pixel_pass(ctx, tr, lr, hr):
    """pixel_step's forward and backward by hand, with the trunk's tape and the activation masks collected -> (tape object, loss)."""
    from sr355 import gan_train as GT
    lr_t, hr_t = ctx.to_device(lr), ctx.to_device(hr)
    with tr._prepacked(False):
        tg = tr.generator_tape()
        assert tg.dense_block_impl == "lds" and tg.lds_packs is not None           # the trainer's pack of this step, not one of the tape's own
        tg.trunk_tape, tg.masks = [], {}
        y = GT.generator_forward(tg, GT.Var(lr_t, need=False), tr.scale, tr.nb, tr.att)
        loss = float(ctx.l1(hr_t, y.v).item())
        y.g = ctx.eltwise(L.ELT_SIGN_DIFF, y.v, hr_t, 1.0 / y.v.numel(), 0.0)
        tg.backward()
    assert tr.g_params.gather(tg.flat) is tg.flat.flat and tg.flat.flat.dtype == torch.float32
    return tg, loss


@pytest.fixture(scope="module")
def steps(ctx):
    """One device pass per weight set, run once and shared: (weights, lr, hr, tape as fp64, loss, masks, gradients {layer: (dw, db)} fp64, flat gradient)."""
    from esrgan_mixed_ref import batch
    from sr355 import gan_train as GT
    cache = {}

    def get(which):
        if which not in cache:
            w = R.weight_sets(NB)[which]
            lr, hr = batch()
            tr = GT.ESRGANTrainer(ctx, w, None, None, SCALE, NB, attention=True, train_dtype="bf16", dense_block_impl="lds")
            tg, loss = taped_pixel_pass(ctx, tr, lr, hr)
            assert all(v.dtype == (torch.float32 if n.endswith("_f32") else BF16) for n, v in tg.trunk_tape)
            tape = {n: t64(v) for n, v in tg.trunk_tape}
            assert len(tape) == len(tg.trunk_tape) and set(tg.grads) == set(w)
            flat = tg.flat.flat.cpu().numpy().copy()
            g = {n: (t64(a), t64(b)) for n, (a, b) in tr.g_params.split(flat).items()}
            cache[which] = (w, lr, hr, tape, loss, {n: m.cpu() for n, m in tg.masks.items()}, g, flat)
        return cache[which]
    return get


def tape_names(nb):
    """What trunk_lds stores: trunk_bf16's names without the G stages, which never leave the LDS."""
    names = {"x0_f32", "dout_f32", "out", f"dR_{nb - 1}"}
    for b, d, _, _, _ in R.blocks(nb):
        names |= {f"F_{b}_{d}", f"dz_{b}_{d}", f"dX_{b}_{d}"} | ({f"drin_{b}"} if d == 1 else set())
    return names


@pytest.mark.parametrize("which", ["he_normal", "relu_on"])
def test_trunk_weight_gradients_on_the_stored_operands(steps, which):
    """The trunk's weight and bias gradients rel-L2 <= 2e-6 against fp64 on the device's own stored F, dz and dY; the masks are read off the stored F slices; the
    entry roundings and the per-RRDB add are bitwise."""
    from edsr_mixed_ref import rb
    w, _, _, tape, _, masks, g, _ = steps(which)
    assert set(tape) == tape_names(NB)
    assert torch.equal(tape["F_0_1"][..., :64], rb(tape["x0_f32"])) and torch.equal(tape[f"dR_{NB - 1}"], rb(tape["dout_f32"]))
    dR = dY = tape[f"dR_{NB - 1}"]
    worst = 0.0
    for b, d, n, a5, bx in reversed(R.blocks(NB)):
        F, dz = tape[f"F_{b}_{d}"], tape[f"dz_{b}_{d}"]
        for k in range(1, 6):
            cin = R.CIN[k - 1]
            dw, db = wgrad64(F[..., :cin], dz[..., 8 * (k - 1):8 * k]) if k < 5 else wgrad64(F, dY, a5)
            ew, eb = rel_l2(g[f"{n}_conv{k}"][0], dw), rel_l2(g[f"{n}_conv{k}"][1], db)
            worst = max(worst, ew, eb)
            assert ew <= 2e-6 and eb <= 2e-6, (n, k, ew, eb)
            if k < 5:
                assert torch.equal(masks[f"{n}_conv{k}"], F[..., cin:cin + 8] > 0)
        dY = tape[f"dX_{b}_{d}"]
        if d == 1:
            assert torch.equal(tape[f"drin_{b}"], rb(dY + dR)), b
            dR = dY = tape[f"drin_{b}"]
    off = np.mean([float((~masks[n]).double().mean()) for n in R.trunk_names(NB) if not n.endswith("_conv5")])
    print(f"{which}: worst trunk gradient rel-L2 {worst:.3e}; {off:.3f} of the trunk's ReLUs are off")
    assert (off > 0.3) if which == "he_normal" else (off < 0.1)


@pytest.mark.parametrize("which", ["he_normal", "relu_on"])
def test_pixel_step_end_to_end_against_fp64_autograd(ctx, steps, which):
    """The device and the restated reference are two realisations of one contract: 1 - cos(device, fp64 autograd) <= 2 (1 - cos(restated, fp64 autograd)) over the
    flat generator gradient.  pixel_step itself applies that very gradient (same bits) through the flat bucket a data-parallel run reduces."""
    from esrgan_mixed_ref import flat as flat_of
    from edsr_mixed_ref import one_minus_cos
    from sr355 import gan_train as GT
    w, lr, hr, tape, loss, _, g, flat = steps(which)
    seen = []
    tr = GT.ESRGANTrainer(ctx, w, None, None, SCALE, NB, attention=True, train_dtype="bf16", dense_block_impl="lds", allreduce_flat=lambda t: (seen.append(t.clone()), t)[1])
    start = tr.g_params.flat.clone()
    assert tr.pixel_step(lr, hr) == loss
    assert len(seen) == 1 and np.array_equal(seen[0].cpu().numpy().view(np.int32), flat.view(np.int32))
    assert tr.g_params.flat.dtype == torch.float32 and not torch.equal(tr.g_params.flat, start)
    order = list(w)
    loss64, g64 = R.pixel_grads(w, lr, hr, NB, mode="plain")
    loss_ref, g_ref = R.pixel_grads(w, lr, hr, NB, mode="mixed")
    dev, ref = one_minus_cos(flat_of(g, order), flat_of(g64, order)), one_minus_cos(flat_of(g_ref, order), flat_of(g64, order))
    print(f"{which}: 1 - cos device {dev:.3e} restated {ref:.3e} (ratio {dev / ref:.2f}); pixel loss device {loss!r} restated {loss_ref!r} fp64 {loss64!r}")
    assert dev <= 2.0 * ref


# |bf16 lds - fp32| / fp32 of the first train_step's g_loss and d_loss, measured on an MI355X over the data seeds 11 .. 15, attention streamed / materialised
# (DESIGN.md 3.28); the assertions are three times the largest of each: the rule of tests/test_esrgan_mixed_gpu.py.
# g_loss is about 36 here (100 x pixel L1 leads it), d_loss 1.385.
G_LOSS_REL_DIFF = {"streamed": [1.616e-06, 2.754e-05, 6.236e-05, 8.965e-06, 2.045e-05], "materialised": [1.618e-06, 2.762e-05, 6.236e-05, 8.965e-06, 2.045e-05]}
D_LOSS_REL_DIFF = {"streamed": [2.582e-07, 2.150e-07, 1.291e-07, 8.608e-08, 8.603e-08], "materialised": [2.582e-07, 2.150e-07, 1.291e-07, 8.608e-08, 8.603e-08]}


@pytest.fixture(scope="module")
def gan_weights():
    from oracle import models as M
    from sr355.weights import init_weights
    dw = init_weights(M.discriminator_layers(), seed=5000)
    vw = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=6000)
    vw = {n: (k * 0.05 if n == "block1_conv1" else k, b) for n, (k, b) in vw.items()}          # inputs are +-128 after caffe preprocessing: keep the features O(1)
    return R.weight_sets(NB)["he_normal"], dw, vw


def first_losses(ctx, gan_weights, lds, attention_impl, seed, steps=1):
    from esrgan_mixed_ref import batch
    from sr355 import gan_train as GT
    gw, dw, vw = gan_weights
    lr, hr = batch(seed=seed)
    kw = {"train_dtype": "bf16", "dense_block_impl": "lds"} if lds else {}
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, SCALE, NB, attention=True, u_seed=3, discriminator="device", attention_impl=attention_impl, **kw)
    return tr, [tr.train_step(lr, hr) for _ in range(steps)]


@pytest.mark.parametrize("attention_impl", ["streamed", "materialised"])
def test_train_step_beside_the_fp32_trainer(ctx, gan_weights, attention_impl):
    """Two trainers from one start, device discriminator: the first step's g_loss and d_loss of the lds trainer beside the fp32 trainer's; three steps keep every
    loss finite; the trunk's layers have moved and their Adam moments are non-zero; the weights read back are fp32."""
    tr, out = first_losses(ctx, gan_weights, True, attention_impl, 11, steps=3)
    _, ref = first_losses(ctx, gan_weights, False, attention_impl, 11)
    rel = {k: abs(out[0][k] - ref[0][k]) / abs(ref[0][k]) for k in ("g_loss", "d_loss")}
    print(f"{attention_impl}: first step g_loss lds {out[0]['g_loss']!r} fp32 {ref[0]['g_loss']!r} ({rel['g_loss']:.3e}); "
          f"d_loss lds {out[0]['d_loss']!r} fp32 {ref[0]['d_loss']!r} ({rel['d_loss']:.3e})")
    assert all(np.isfinite(v) for o in out for v in o.values())
    assert rel["g_loss"] <= 3.0 * max(G_LOSS_REL_DIFF[attention_impl]) and rel["d_loss"] <= 3.0 * max(D_LOSS_REL_DIFF[attention_impl])
    gw = gan_weights[0]
    now, P = tr.gw, tr.g_params
    m = P.split(tr.g_opt.m)
    for n in R.trunk_names(NB):
        assert now[n][0].dtype == np.float32 and now[n][1].dtype == np.float32
        assert not np.array_equal(now[n][0], gw[n][0]) and not np.array_equal(now[n][1], gw[n][1]), n
        assert bool((m[n][0] != 0).any()) and bool((m[n][1] != 0).any()), n
    assert set(tr.last_grads["g"]) == set(gw)


def test_host_discriminator_and_masks_compose(ctx, gan_weights):
    """discriminator_update="host" and collect_masks run through the same step: the trunk's masks are those of the stored F slices (all 24 growth convs)."""
    from esrgan_mixed_ref import batch
    from sr355 import gan_train as GT
    gw, dw, vw = gan_weights
    lr, hr = batch(seed=12)
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, SCALE, NB, attention=True, u_seed=3, discriminator="host", train_dtype="bf16", dense_block_impl="lds")
    tr.collect_masks = True
    out = tr.train_step(lr, hr)
    assert all(np.isfinite(v) for v in out.values())
    trunk = [n for n in R.trunk_names(NB) if not n.endswith("_conv5")]
    assert all(tuple(tr.last_masks["g"][n].shape) == (2, 12, 12, 8) and tr.last_masks["g"][n].dtype == torch.bool for n in trunk)


# ------------------------------------------------------------------------------------------------ 7. the interface
def profiled(ctx, fn):
    ctx.profile_begin()
    out = fn()
    return out, {r["kernel"]: r["launches"] for r in ctx.profile_end()}


def test_notebook_configuration_through_the_wrapper(ctx, gan_weights):
    """ESRGAN(train_dtype="bf16", train_dense_block="lds") at the notebook's configuration -- x2, 4 RRDBs, G 8, LR patches of 24 x 24: _train_step runs the new
    kernels (one pack, 12 forward and 12 backward launches) and no row-sliding conv, the trunk's only other bf16 conv kernel; a 48 x 48 batch is refused and leaves
    the parameters, Adam's moments and the step counts alone."""
    from oracle import models as M
    from sr355.synth import make_pairs
    from sr355.weights import init_weights
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    _, dw, vw = gan_weights
    gw = R.weight_sets(4, seed=4200)["he_normal"]
    m = ESRGAN(train_dtype="bf16", train_dense_block="lds", discriminator_update="device", train_attention="streamed")
    m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=4)
    m.set_weights(gw)
    m.set_loss_network_weights(discriminator=dw, vgg19=vw)
    tr = m._ensure_trainer()
    assert tr.dense_block_impl == "lds" and tr.generator_tape(wgrad=False).dense_block_impl == "layers"
    lr, hr = make_pairs(2, 24, 24, 2, 21)
    lr, hr = (lr * 2.0 - 1.0).astype(np.float32), (hr * 2.0 - 1.0).astype(np.float32)
    out, ran = profiled(ctx, lambda: m._train_step(lr, hr))
    assert all(np.isfinite(v) for v in out.values())
    assert ran.get(PACK) == 1 and ran.get(FWD) == 12 and ran.get(BWD) == 12, ran
    assert not any(k.startswith("conv_rows") for k in ran), sorted(ran)
    m._sync_from_trainer()
    assert all(k.dtype == np.float32 and b.dtype == np.float32 for k, b in m.weights.values())
    assert all(not np.array_equal(m.weights[n][0], gw[n][0]) for n in R.trunk_names(4))
    # a patch that does not fit: refused by the step, nothing touched
    before = (tr.g_params.flat.clone(), tr.g_opt.m.clone(), tr.g_opt.v.clone(), tr.g_opt.t, tr.step, tr.d_opt.t)
    d_before = tr.d_params.flat.clone()
    lr2, hr2 = make_pairs(2, 48, 48, 2, 22)
    with pytest.raises(ValueError, match=r"H = 48, W = 48 .* <= 676"):
        m._train_step(lr2.astype(np.float32), hr2.astype(np.float32))
    with pytest.raises(ValueError, match=r"H = 48, W = 48"):
        tr.pixel_step(lr2.astype(np.float32), hr2.astype(np.float32))
    assert torch.equal(tr.g_params.flat, before[0]) and torch.equal(tr.g_opt.m, before[1]) and torch.equal(tr.g_opt.v, before[2])
    assert (tr.g_opt.t, tr.step, tr.d_opt.t) == before[3:] and torch.equal(tr.d_params.flat, d_before)


def test_growth_other_than_8_is_refused_before_anything_runs(ctx):
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    m = ESRGAN(train_dtype="bf16", train_dense_block="lds")
    m.setup_model(scale_factor=2, growth_channels=32, num_rrdb_blocks=1)
    ctx.conv_routes(True)
    with pytest.raises(ValueError, match=r"rrdb_0_dense1_conv1 has 32 growth channels"):
        m._ensure_trainer()
    assert ctx.conv_routes(False) == [] and m._trainer is None


def test_default_is_unchanged(ctx):
    """dense_block_impl="layers" is the argument omitted: one pixel_step gives the same bits, at G = 8 in fp32 and at G = 32 in bf16, and none of the new kernels runs."""
    from esrgan_mixed_ref import batch, weight_sets
    from sr355 import gan_train as GT
    lr, hr = batch()
    for w, kw0 in ((R.weight_sets(NB)["he_normal"], {}), (weight_sets()["he_normal"], {"train_dtype": "bf16"})):
        runs = []
        for kw in ({}, {"dense_block_impl": "layers"}):
            tr = GT.ESRGANTrainer(ctx, w, None, None, SCALE, NB, attention=True, **kw0, **kw)
            loss, ran = profiled(ctx, lambda: tr.pixel_step(lr, hr))
            assert not ({FWD, BWD, PACK} & set(ran)), sorted(ran)
            runs.append((loss, tr.g_params.flat.cpu().numpy().view(np.int32)))
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
