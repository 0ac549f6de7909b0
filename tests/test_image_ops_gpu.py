"""The image ops of csrc/imgops.hip -- sr_bicubic, sr_resize, sr_psnr, sr_ssim, sr_mse, sr_extract_patches, sr_overlap_add -- per
element at the edges of their host-side kernel choices.

The cases and the route each one takes are in tests/image_ops_cases.py (tests/test_image_ops_cases_cpu.py proves the tables reach
both sides of every predicate term).  Contracts are the ones of test_kernels_gpu.py: fp32 resizes within 2e-6 of the oracle on
U[0,1) data, uint8 resizes bit for bit, PSNR within 2e-4 dB, MSE 1e-5 relative, the SSIM mean within 5e-5, overlap-add within 1e-6.
Added here: every resize writes into the middle of a poisoned buffer whose guard bytes must come back untouched; sequences on one
context without a synchronisation in between (tap table, reduction scratch) must equal the same calls made alone, bit for bit; the
SSIM is held at window level by a perturbation confined to one 6 x 6 block; the patch plumbing runs in the types of the bf16
generator path, once on exact k/64 data where a wrong index is a bit mismatch.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import image_ops_cases as T
from oracle import ops as O
from sr355 import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096                      # bytes of poison on either side of an output
F32_NAN_BITS = 0x7FC0DEAD
U8_POISON = 0xA5
BF16_NAN_BITS = 0x7FDE
_TD = {"f32": torch.float32, "u8": torch.uint8, "bf16": torch.bfloat16}
_LD = {"f32": L.DTYPE_F32, "u8": L.DTYPE_U8, "bf16": L.DTYPE_BF16}


class Guarded:
    """n elements of `dtype` in the middle of a buffer with GUARD poisoned bytes on each side."""

    def __init__(self, ctx, n, dtype):
        td = _TD[dtype]
        self.esz = torch.empty((), dtype=td).element_size()
        self.g = GUARD // self.esz
        self.n = n
        self.itd, self.bits = {"f32": (torch.int32, F32_NAN_BITS), "u8": (torch.uint8, U8_POISON), "bf16": (torch.int16, BF16_NAN_BITS)}[dtype]
        self.buf = torch.empty(n + 2 * self.g, dtype=td, device=ctx.torch_device)
        self.buf.view(self.itd).fill_(self.bits)
        self.y = self.buf[self.g:self.g + n]

    def untouched(self):
        torch.cuda.synchronize()
        guard = torch.cat([self.buf[:self.g], self.buf[self.g + self.n:]]).view(self.itd)
        return bool((guard == self.bits).all().item())

    def written(self):
        """every element of the output was stored (uint8: unless the result happens to be the poison byte, which proves nothing)"""
        if self.itd == torch.uint8:
            return True
        return not bool((self.y.view(self.itd) == self.bits).any().item())


def raw_resize(ctx, x, out, interp=None):
    """sr_bicubic (interp None) or sr_resize into a Guarded buffer -> (result as NumPy, guards untouched, all written)."""
    dtype = "u8" if x.dtype == np.uint8 else "f32"
    B, H, W, Cx = x.shape
    xd = ctx.to_device(x, _TD[dtype])
    gb = Guarded(ctx, B * out[0] * out[1] * Cx, dtype)
    if interp is None:
        rc = ctx.lib.sr_bicubic(ctx.h, xd.data_ptr(), _LD[dtype], B, H, W, Cx, out[0], out[1], gb.y.data_ptr(), ctx.stream())
    else:
        rc = ctx.lib.sr_resize(ctx.h, xd.data_ptr(), _LD[dtype], B, H, W, Cx, out[0], out[1], int(interp), gb.y.data_ptr(), ctx.stream())
    ctx.check(rc)
    ok = gb.untouched()
    return gb.y.cpu().numpy().reshape(B, out[0], out[1], Cx), ok, gb.written()


def u8_reference(x, out, interp):
    return np.stack([O.bicubic_resize_u8(im, out[0], out[1]) if interp in (None, T.CUBIC) else O.cv_resize_u8(im, out[0], out[1], interp) for im in x])


# ------------------------------------------------------------------------------------------------ bicubic
@pytest.mark.parametrize("case", T.BICUBIC_CASES, ids=[c[0] for c in T.BICUBIC_CASES])
def test_bicubic_per_element(ctx, case):
    """Every row of BICUBIC_CASES through sr_bicubic: the tile kernel at C = 1..4, ragged and batched, at win_rows == BT_ROWS, one
    window column inside BT_WIN and above 64 KB of LDS; the per-pixel kernel for each reason that selects it; the uint8 kernel."""
    cid, dtype, shape, out = case
    x = T.case_input(cid, dtype, shape)
    got, untouched, written = raw_resize(ctx, x, out)
    assert untouched, "stores outside the output"
    assert written, "output elements never stored"
    if dtype == "f32":
        ref = O.bicubic_resize(x, out[0], out[1], dtype=np.float64)
        err = float(np.max(np.abs(got - ref)))
        print(f"{cid}: {T.bicubic_route(dtype, shape, out).kernel}, max |got - fp64| = {err:.3e}")
        assert err <= 2e-6, err
    else:
        ref = u8_reference(x, out, None)
        for b in range(shape[0]):
            assert np.array_equal(got[b], ref[b]), (cid, b, int(np.abs(got[b].astype(int) - ref[b].astype(int)).max()))


def test_bicubic_wrapper_equals_raw_call(ctx):
    """Context.bicubic on the largest-LDS tile case: the wrapper path raises nothing and returns the raw call's bits."""
    cid, dtype, shape, out = next(c for c in T.BICUBIC_CASES if c[0] == "tile_c4_lds_above_64k")
    x = T.case_input(cid, dtype, shape)
    got, _, _ = raw_resize(ctx, x, out)
    assert np.array_equal(ctx.bicubic(ctx.to_device(x), out[0], out[1]).cpu().numpy(), got)
    assert np.array_equal(ctx.resize(ctx.to_device(x), out[0], out[1], "INTER_CUBIC").cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------ the resize family
_SERVED = [c for c in T.RESIZE_CASES if T.resize_route(c[1], c[2], c[3], c[4]).kernel != "refused"]
_REFUSED = [c for c in T.RESIZE_CASES if T.resize_route(c[1], c[2], c[3], c[4]).kernel == "refused"]


@pytest.mark.parametrize("case", _SERVED, ids=[c[0] for c in _SERVED])
def test_resize_per_element(ctx, case):
    cid, dtype, shape, out, interp = case
    x = T.case_input(cid, dtype, shape)
    got, untouched, written = raw_resize(ctx, x, out, interp)
    assert untouched, "stores outside the output"
    assert written, "output elements never stored"
    if dtype == "f32":
        ref = O.bicubic_resize(x, out[0], out[1], dtype=np.float64) if interp == T.CUBIC else O.cv_resize(x, out[0], out[1], interp)
        err = float(np.max(np.abs(got - ref)))
        print(f"{cid}: {T.resize_route(dtype, shape, out, interp).kernel}, max |got - ref| = {err:.3e}")
        assert err <= 2e-6, err
    else:
        ref = u8_reference(x, out, interp)
        for b in range(shape[0]):
            assert np.array_equal(got[b], ref[b]), (cid, b, int(np.abs(got[b].astype(int) - ref[b].astype(int)).max()))


@pytest.mark.parametrize("interp,out", T.SATURATION_RUNS)
def test_resize_u8_saturates_at_both_ends(ctx, interp, out):
    """0 / 255 steps and a one-pixel checkerboard: the fixed-point sums leave [0, 255] on both sides (asserted on the reference in
    test_image_ops_cases_cpu.py); bit for bit, for the image alone and as the middle one of a batch."""
    img = T.saturation_image()
    ref = u8_reference(img[None], out, interp)[0]
    assert (ref == 0).any() and (ref == 255).any()
    rng = np.random.default_rng(out[0])
    batch = np.stack([rng.integers(0, 256, img.shape, dtype=np.uint8), img, img[::-1, ::-1].copy()])
    got, untouched, _ = raw_resize(ctx, batch, out, interp)
    assert untouched
    assert np.array_equal(got[1], ref)
    assert np.array_equal(got, u8_reference(batch, out, interp))
    if interp == T.CUBIC:
        got2, untouched2, _ = raw_resize(ctx, batch, out)
        assert untouched2 and np.array_equal(got2, got)


def test_resize_tap_table_sequence_without_sync(ctx):
    """The per-context tap table: a small LANCZOS4 resize, an INTER_AREA shrink whose table is far larger than any other in the suite
    (the table is freed and regrown behind a device synchronisation), then the small one again -- nothing synchronises in between on
    the caller's side.  Each result equals the same call made alone."""
    rng = np.random.default_rng(77)
    small = rng.uniform(0, 1, (1, 9, 11, 3)).astype(np.float32)
    big = rng.uniform(0, 1, (1, 6000, 6, 1)).astype(np.float32)            # -> 2999 x 5: 5 taps x 2999 rows
    ds, db = ctx.to_device(small), ctx.to_device(big)
    assert T.resize_route("f32", big.shape, (2999, 5), T.AREA).kernel == "float_taps"
    torch.cuda.synchronize()
    s1 = ctx.resize(ds, 20, 25, "INTER_LANCZOS4")
    b1 = ctx.resize(db, 2999, 5, "INTER_AREA")
    s2 = ctx.resize(ds, 20, 25, "INTER_LANCZOS4")
    b2 = ctx.resize(db, 2999, 5, "INTER_AREA")                             # table reused this time
    torch.cuda.synchronize()
    alone = []
    for t, o, ip in ((ds, (20, 25), "INTER_LANCZOS4"), (db, (2999, 5), "INTER_AREA")):
        alone.append(ctx.resize(t, o[0], o[1], ip))
        torch.cuda.synchronize()
    assert torch.equal(s1, alone[0]) and torch.equal(s2, alone[0])
    assert torch.equal(b1, alone[1]) and torch.equal(b2, alone[1])
    assert np.max(np.abs(alone[0].cpu().numpy() - O.cv_resize(small, 20, 25, T.LANCZOS4))) <= 2e-6
    assert np.max(np.abs(alone[1].cpu().numpy() - O.cv_resize(big, 2999, 5, T.AREA))) <= 2e-6


@pytest.mark.parametrize("case", _REFUSED, ids=[c[0] for c in _REFUSED])
def test_resize_refusal_leaves_the_context_usable(ctx, case):
    cid, dtype, shape, out, interp = case
    x = T.case_input(cid, dtype, shape)
    xd = ctx.to_device(x, _TD[dtype])
    with pytest.raises(ValueError) as e:
        ctx.resize(xd, out[0], out[1], interp)
    assert str(e.value) == T.REFUSAL_MESSAGE
    # the factor-14 neighbour on the same context, right after the refusal
    ncid, ndtype, nshape, nout, ninterp = next(c for c in T.RESIZE_CASES if c[1] == dtype and c[0].endswith("factor_14"))
    nx = T.case_input(ncid, ndtype, nshape)
    got = ctx.resize(ctx.to_device(nx, _TD[dtype]), nout[0], nout[1], ninterp).cpu().numpy()
    if dtype == "f32":
        assert np.max(np.abs(got - O.cv_resize(nx, nout[0], nout[1], ninterp))) <= 2e-6
    else:
        assert np.array_equal(got, u8_reference(nx, nout, ninterp))


# ------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("shape,sds", T.REDUCE_CASES, ids=["x".join(map(str, s)) for s, _ in T.REDUCE_CASES])
def test_psnr_mse_sizes(ctx, shape, sds):
    """270 000 elements per image (the grid is capped at 1024 x 256 threads per image: the grid-stride loop runs, with blockIdx.y > 0),
    1, 255 and 257 elements; the images of a batch differ by orders of magnitude in error, so a wrong image offset cannot hide."""
    a, b = T.reduce_pair(shape, sds)
    da, db = ctx.to_device(a), ctx.to_device(b)
    p = ctx.psnr(da, db).cpu().numpy().astype(np.float64)
    ref = O.psnr(a, b, dtype=np.float64)
    print(f"psnr {shape}: got {p}, fp64 {ref}")
    assert np.all(np.abs(p - ref) <= 2e-4), (p, ref)
    m = float(ctx.mse(da, db).cpu().numpy()[0])
    mref = float(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))
    assert abs(m - mref) <= 1e-5 * mref, (m, mref)
    assert torch.isinf(ctx.psnr(da, da)).all() and (ctx.psnr(da, da) > 0).all()
    assert float(ctx.mse(db, db).cpu().numpy()[0]) == 0.0


def test_metrics_share_scratch_without_sync(ctx):
    """psnr (B = 1, small), ssim (B = 4), mse (large), psnr (B = 3, large) back to back: all four use the context's reduction scratch
    on one stream.  The reductions are fixed-order, so each value must equal, bit for bit, the one from the same call made alone."""
    (big_shape, big_sds) = T.REDUCE_CASES[0]
    a3, b3 = T.reduce_pair(big_shape, big_sds)
    a1, b1 = T.reduce_pair((1, 5, 7, 3), (0.05,))
    a4, b4 = T.ssim_pair((4, 43, 50, 3))
    d = {k: ctx.to_device(v) for k, v in dict(a3=a3, b3=b3, a1=a1, b1=b1, a4=a4, b4=b4).items()}
    calls = [lambda: ctx.psnr(d["a1"], d["b1"]), lambda: ctx.ssim(d["a4"], d["b4"]), lambda: ctx.mse(d["a3"], d["b3"]),
             lambda: ctx.psnr(d["a3"], d["b3"])]
    torch.cuda.synchronize()
    together = [f() for f in calls]
    torch.cuda.synchronize()
    for f, t in zip(calls, together):
        alone = f()
        torch.cuda.synchronize()
        assert torch.equal(alone, t), (alone, t)
    assert np.all(np.abs(together[3].cpu().numpy() - O.psnr(a3, b3, dtype=np.float64)) <= 2e-4)
    assert np.allclose(together[1].cpu().numpy(), O.ssim(a4, b4, dtype=np.float64), atol=5e-5, rtol=0)


# ------------------------------------------------------------------------------------------------ SSIM
@pytest.mark.parametrize("shape", T.SSIM_MEAN_SHAPES, ids=["x".join(map(str, s)) for s in T.SSIM_MEAN_SHAPES])
def test_ssim_mean_shapes(ctx, shape):
    """One window (11 x 11), one row / column of windows, exactly one full 32 x 32 tile of windows (42 x 42), one extra tile row and
    column holding a single window each (43 x 43); C = 1..4."""
    a, b = T.ssim_pair(shape)
    s = ctx.ssim(ctx.to_device(a), ctx.to_device(b)).cpu().numpy().astype(np.float64)
    ref = O.ssim(a, b, dtype=np.float64)
    print(f"ssim {shape}: max |got - fp64| = {np.max(np.abs(s - ref)):.3e}")
    assert np.all(np.abs(s - ref) <= 5e-5), (s, ref)


def test_ssim_max_val_255(ctx):
    a, b = T.ssim_255_pair()
    bound, gap = T.ssim_255_bound(a, b)
    s = ctx.ssim(ctx.to_device(a), ctx.to_device(b), max_val=255.0).cpu().numpy().astype(np.float64)
    ref = O.ssim(a, b, max_val=255.0, dtype=np.float64)
    print(f"ssim max_val=255: fp32-vs-fp64 oracle gap {gap:.3e}, bound {bound:.3e}, max |got - fp64| = {np.max(np.abs(s - ref)):.3e}")
    assert np.all(np.abs(s - ref) <= bound), (s, ref, bound)
    # scored with the constants of max_val = 1 the same images are 0.09 away (test_image_ops_cases_cpu.py): max_val reached the kernel


@pytest.mark.parametrize("name", sorted(T.SSIM_LOCAL_BLOCKS))
def test_ssim_localised_block(ctx, name):
    """b equals a outside one 6 x 6 block, so every window away from it contributes exactly 1.0 in the kernel and the summed deficit
    D = (1 - ssim) * oH * oW * C is the affected windows' alone.  Every affected window loses at least 0.02 in the fp64 reference
    (asserted), so |D_dev - D_ref| below half the smallest loss admits no window dropped, doubled or read one tap off -- at a tile
    seam, in the one-window last tile row / column, or at the corner.
    First run on an MI355X: |D_dev - D_ref| between 1.2e-4 and 4.1e-4 over the ten blocks (D is 100 .. 736, the bounds 0.036 .. 0.043)."""
    a, b = T.ssim_local_pair(name)
    d = T.ssim_window_deficits(a, b, name)
    assert d.min() >= T.SSIM_MIN_DEFICIT
    bound = 0.5 * float(d.min())
    D_ref = T.ssim_deficit_sum(a, b, O.ssim(a, b, dtype=np.float64)[0])
    da, db = ctx.to_device(a), ctx.to_device(b)
    D_dev = T.ssim_deficit_sum(a, b, ctx.ssim(da, db).cpu().numpy().astype(np.float64)[0])
    print(f"ssim block {name}: D_ref {D_ref:.6f}, D_dev {D_dev:.6f}, |diff| {abs(D_dev - D_ref):.3e}, bound {bound:.3e}")
    assert abs(D_dev - D_ref) <= bound, (D_dev, D_ref, bound)
    same = float(ctx.ssim(da, da).cpu().numpy()[0])
    print(f"ssim block {name}: ssim(a, a) = {same!r}")
    assert abs(same - 1.0) <= 1e-6


# ------------------------------------------------------------------------------------------------ patches
def _raw_extract(ctx, img, patch, stride, mul, add, out_dtype):
    H, W, Cx = img.shape
    n = ctx.num_patches(H, W, Cx, patch, stride)
    gb = Guarded(ctx, n * patch * patch * Cx, out_dtype)
    cnt = C.c_int()
    d = ctx.to_device(img)
    ctx.check(ctx.lib.sr_extract_patches(ctx.h, d.data_ptr(), H, W, Cx, patch, stride, float(mul), float(add), _LD[out_dtype], gb.y.data_ptr(),
                                         gb.n, C.byref(cnt), ctx.stream()))
    ok = gb.untouched()
    assert cnt.value == n
    return gb.y.float().cpu().numpy().reshape(n, patch, patch, Cx), ok, gb.written()


def _raw_overlap_add(ctx, patches, in_dtype, hw, patch, stride, scale, mul, add):
    Cx = patches.shape[-1]
    d = ctx.to_device(patches, _TD[in_dtype])
    gb = Guarded(ctx, hw[0] * scale * hw[1] * scale * Cx, "f32")
    ctx.check(ctx.lib.sr_overlap_add(ctx.h, d.data_ptr(), _LD[in_dtype], hw[0], hw[1], Cx, patch, stride, scale, float(mul), float(add),
                                     gb.y.data_ptr(), ctx.stream()))
    ok = gb.untouched()
    return gb.y.cpu().numpy().reshape(hw[0] * scale, hw[1] * scale, Cx), ok, gb.written()


@pytest.mark.parametrize("hw,p,s", T.PATCH_CASES)
def test_extract_patches_bf16_out(ctx, hw, p, s):
    """The bf16 generator path's extraction: img * 2 - 1 in fp32, stored as bf16, gathered at the reference's positions (reflect
    padding bottom / right); bit for bit."""
    rng = np.random.default_rng(hw[0] * 100 + hw[1])
    img = rng.uniform(0, 1, (*hw, 3)).astype(np.float32)
    got, untouched, written = _raw_extract(ctx, img, p, s, 2.0, -1.0, "bf16")
    assert untouched and written
    val = O.round_bf16(img * np.float32(2.0) + np.float32(-1.0))
    ref, pos = O.extract_patches(O.add_padding(val, p, s), p, s)
    assert got.shape == ref.shape and len(pos) == got.shape[0]
    assert np.array_equal(got, ref)
    wrapped = ctx.extract_patches(ctx.to_device(img), p, s, mul=2.0, add=-1.0, out_dtype=torch.bfloat16)
    assert wrapped.dtype == torch.bfloat16 and np.array_equal(wrapped.float().cpu().numpy(), ref)
    got32, untouched32, written32 = _raw_extract(ctx, img, p, s, 2.0, -1.0, "f32")
    assert untouched32 and written32
    assert np.array_equal(got32, O.extract_patches(O.add_padding(img * np.float32(2.0) + np.float32(-1.0), p, s), p, s)[0])


def test_extract_patches_pad_limit_raises(ctx):
    hw, p, s = T.PATCH_REFUSED
    with pytest.raises(ValueError, match="pad < image size"):
        ctx.extract_patches(ctx.to_device(np.zeros((*hw, 3), np.float32)), p, s, out_dtype=torch.bfloat16)


@pytest.mark.parametrize("scale", T.OVERLAP_SCALES)
@pytest.mark.parametrize("hw,p,s", T.PATCH_CASES)
def test_overlap_add_from_bf16(ctx, hw, p, s, scale):
    """bf16 patches in [-1.4, 1.4] with mul = add = 0.5 (the generator's tanh range back to [0, 1], values beyond the clip on both
    sides present); the fp64 reference is applied to the bf16-rounded patches."""
    n = ctx.num_patches(hw[0], hw[1], 3, p, s)
    rng = np.random.default_rng(hw[0] + 7 * scale)
    patches = O.round_bf16(rng.uniform(-1.4, 1.4, (n, p * scale, p * scale, 3)).astype(np.float32))
    vals = patches.astype(np.float64) * 0.5 + 0.5
    assert (vals < 0).any() and (vals > 1).any()
    padded = (hw[0] + O.pad_amount(hw[0], p, s), hw[1] + O.pad_amount(hw[1], p, s))
    pos = O.patch_positions(padded[0], padded[1], p, s)
    assert len(pos) == n
    ref = O.overlap_add(vals, pos, padded, hw, p, scale, dtype=np.float64)
    assert (ref == 0).any() and (ref == 1).any()
    got, untouched, written = _raw_overlap_add(ctx, patches, "bf16", hw, p, s, scale, 0.5, 0.5)
    assert untouched and written
    err = float(np.max(np.abs(got - ref)))
    assert err <= 1e-6, err
    wrapped = ctx.overlap_add(ctx.to_device(patches, torch.bfloat16), hw[0], hw[1], p, s, scale, mul=0.5, add=0.5).cpu().numpy()
    assert np.array_equal(wrapped, got)


@pytest.mark.parametrize("in_dtype", ["bf16", "f32"])
@pytest.mark.parametrize("scale", T.OVERLAP_SCALES)
@pytest.mark.parametrize("hw,p,s", T.PATCH_CASES)
def test_overlap_add_exact_integers(ctx, hw, p, s, scale, in_dtype):
    """Patches hold k/64 with |k| <= 96 (exact in bf16), mul = add = 0.5: sums of up to four such values and their quotients by 1, 2
    or 4 are exact in fp32, so the result equals the reference bit for bit and a patch read at a wrong index is a mismatch."""
    n = ctx.num_patches(hw[0], hw[1], 3, p, s)
    rng = np.random.default_rng(hw[1] + 11 * scale)
    patches = (rng.integers(-96, 97, (n, p * scale, p * scale, 3)) / 64.0).astype(np.float32)
    assert np.array_equal(O.round_bf16(patches), patches)
    padded = (hw[0] + O.pad_amount(hw[0], p, s), hw[1] + O.pad_amount(hw[1], p, s))
    pos = O.patch_positions(padded[0], padded[1], p, s)
    ref64 = O.overlap_add(patches.astype(np.float64) * 0.5 + 0.5, pos, padded, hw, p, scale, dtype=np.float64)
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64)             # exact: nothing was rounded on the way
    got, untouched, written = _raw_overlap_add(ctx, patches, in_dtype, hw, p, s, scale, 0.5, 0.5)
    assert untouched and written
    assert np.array_equal(got, ref), int((got != ref).sum())
