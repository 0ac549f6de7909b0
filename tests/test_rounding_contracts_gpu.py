"""The kernels whose contract names two roundings -- a product rounded, then the sum that takes it -- held to the bits on inputs where one
fused multiply-add gives other bits.  Every comparison is exact, covers every element and is against the UNFUSED reference (oracle.ops,
classic_ref, patch_dataset_ref); tests/rounding_ref.py's fused variants only count, per case, the elements a contracted kernel would get
wrong (printed), and tests/test_rounding_contracts_cpu.py asserts that count is large enough for the case to mean something.

Not exact, and why: nothing here.  Two comparisons elsewhere stay toleranced for a reason other than contraction: sr_nl_means' denoised image
(1e-5: exp() and a different summation order than skimage's integral images) and Context.non_local_means' up-scale against the fp64
classic_ref.resize_f64 (2e-5: the device resizes the fp32 image in fp32); the same up-scale is exact here against the fp32 oracle."""
import numpy as np
import pytest
import torch

import classic_ref as CR
import patch_dataset_ref as PR
import rounding_ref as R
from oracle import ops as O
from test_image_ops_gpu import raw_resize

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def assert_bits(got, ref, fused, what):
    """got == ref in every bit; prints how many elements the fused evaluation gets wrong, and how many of those the device got wrong."""
    got, ref, fused = np.asarray(got), np.asarray(ref), np.asarray(fused)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = bits(got) != bits(ref)
    disc = bits(fused) != bits(ref)
    print(f"{what}: {int(disc.sum())} of {ref.size} elements discriminate; device differs from the unfused reference in {int(bad.sum())}, "
          f"equals the fused one in {int((bad & (bits(got) == bits(fused))).sum())} of them")
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def dev_u8(ctx, *arrs):
    return ctx.to_device(np.stack(arrs), torch.uint8)


# ---------------------------------------------------------------------------------------------------- sr_resize, float taps
@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("case", R.RESIZE_F32_CASES, ids=[c[0] for c in R.RESIZE_F32_CASES])
def test_resize_f32_is_the_oracle_bit_for_bit(ctx, case, C):
    cid, shape, out, interp, data = case
    x = R.resize_input(cid, shape, C, data)
    got, untouched, written = raw_resize(ctx, x, out, interp)
    assert untouched and written
    assert_bits(got, O.cv_resize(x, *out, interp), R.cv_resize(x, *out, interp, fused=True), f"sr_resize {cid} C={C}")


@pytest.mark.parametrize("kind", ["ramp", "random"])
@pytest.mark.parametrize("pair", R.COORD_PAIRS, ids=[f"{a}to{b}_interp{i}" for a, b, i in R.COORD_PAIRS])
def test_resize_coordinates_an_fma_would_move(ctx, pair, kind):
    """resize_taps_kernel's (d + 0.5) * scale - 0.5: unfused it is exactly 0 at one d of these size pairs, fused 1e-17, and the second tap
    then has a weight where it should have none."""
    n_src, n_dst, interp = pair
    x = R.coord_case_input(n_src, n_dst, interp, kind)
    got, untouched, written = raw_resize(ctx, x, (n_dst, n_dst), interp)
    assert untouched and written
    assert_bits(got, O.cv_resize(x, n_dst, n_dst, interp), R.cv_resize(x, n_dst, n_dst, interp, fused_coords=True), f"sr_resize {pair} {kind}")


@pytest.mark.parametrize("cid", list(R.AREA_U8_CASES))
def test_resize_area_u8_on_the_planted_image(ctx, cid):
    """resize_apply_area_u8_kernel, a fractional INTER_AREA shrink of uint8: the float taps, then rint.  The image holds searched pixels under
    fifteen outputs whose fused sum rounds to the other integer (none can exist at the first size: rounding_ref.AREA_U8_CASES)."""
    shape, out = R.AREA_U8_CASES[cid]
    img, planted = R.area_u8_case(cid)
    got, untouched, _ = raw_resize(ctx, img[None], out, O.INTER_AREA)
    assert untouched
    ref = O.cv_resize_area_shrink_u8(img, *out)
    assert_bits(got[0], ref, R.cv_resize_area_shrink_u8(img, *out, fused=True), f"sr_resize uint8 INTER_AREA {shape} -> {out} ({len(planted)} planted)")


# ---------------------------------------------------------------------------------------------------- the classical up-scalers
@pytest.mark.parametrize("iterations", R.IBP_ITERATIONS)
@pytest.mark.parametrize("shape", R.IBP_SHAPES)
def test_back_projection_bit_for_bit(ctx, shape, iterations):
    hr, lr = R.ibp_inputs(*shape)
    y, est = ctx.back_projection(ctx.to_device(hr), ctx.to_device(lr), iterations, raw=True)
    ref = [CR.back_projection(hr[b], lr[b], iterations) for b in range(R.IBP_BATCH)]
    fus = [R.back_projection(hr[b], lr[b], iterations, fused=True) for b in range(R.IBP_BATCH)]
    assert_bits(est.cpu().numpy(), np.stack([r[1] for r in ref]), np.stack([f[1] for f in fus]), f"sr_back_projection {shape} x{iterations} y_f32")
    assert np.array_equal(y.cpu().numpy(), np.stack([r[0] for r in ref]))


@pytest.mark.parametrize("shape", R.EGI_SHAPES)
def test_edge_guided_bit_for_bit(ctx, shape):
    H, W, h, w = shape
    x = R.egi_input(*shape)
    for wt, _ in [(0.3, 0)] + R.egi_weights(*shape):
        y, up_e = ctx.edge_guided(dev_u8(ctx, x), H, W, weight=wt, raw=True)
        ref_y, ref_up_e = CR.edge_guided(x, H, W, wt)
        fus_y, fus_up_e = R.edge_guided(x, H, W, wt, fused=True)
        assert_bits(up_e[0].cpu().numpy(), ref_up_e, fus_up_e, f"sr_edge_guided {shape} weight {wt!r} up_e_f32")
        assert_bits(y[0].cpu().numpy(), ref_y, fus_y, f"sr_edge_guided {shape} weight {wt!r} y_u8")


@pytest.mark.parametrize("shape", R.SIGMA_SHAPES)
def test_noise_sigma_bit_for_bit(ctx, shape):
    x = R.sigma_input(shape)
    got = ctx.noise_sigma(dev_u8(ctx, x, x[::-1, ::-1].copy())).cpu().numpy()
    ref = np.array([CR.noise_sigma(x), CR.noise_sigma(x[::-1, ::-1])])
    fus = np.array([R.noise_sigma(x, fused=True), R.noise_sigma(x[::-1, ::-1], fused=True)])
    print(f"db2 dd band {shape}: {R.differing(R.db2_hh(x), R.db2_hh(x, fused=True))} of {R.db2_hh(x).size} coefficients discriminate")
    assert_bits(got, ref, fus, f"sr_noise_sigma {shape}")


def test_nl_means_upscale_is_the_fp32_oracle(ctx):
    """Context.non_local_means' INTER_LANCZOS4 step is sr_resize on the fp32 denoised image: exact against the fp32 oracle on the device's own
    denoised image (against classic_ref.resize_f64 it can only be close: that one accumulates in fp64)."""
    H, W, h, w = R.EGI_SHAPES[0]
    x = R.egi_input(H, W, h, w)
    up, den, _ = ctx.non_local_means(dev_u8(ctx, x), H, W, raw=True)
    den = den.cpu().numpy()[:, :, :, None]
    assert_bits(up.cpu().numpy()[:, :, :, None], O.cv_resize(den, H, W, O.INTER_LANCZOS4), R.cv_resize(den, H, W, O.INTER_LANCZOS4, fused=True),
                "non_local_means Lanczos up-scale")


# ---------------------------------------------------------------------------------------------------- v * mul + add
def _patches_ref(img, p, s, mul, add, fused):
    return O.extract_patches(O.add_padding(R.scale(img, mul, add, fused), p, s), p, s)[0]


@pytest.mark.parametrize("op", ["gather_patch_pairs_u8", "gather_patch_pairs_f32", "extract_patches", "extract_patches_batch_u8_quad",
                                "extract_patches_batch_f32_quad", "extract_patches_batch_u8_scalar", "extract_patches_batch_f32_scalar"])
def test_scaling_rounds_product_and_sum_separately(ctx, op):
    """gather_pixel (patch_dataset.hip), extract_patches_kernel (imgops.hip) and affine (study.hip, both of its kernels): NumPy's v * mul + add."""
    if op.startswith("gather_patch_pairs"):
        stack = R.scale_stack(op[-3:].lstrip("_"))
        mul, add = R.SCALE_UNIT
        table = np.array([(0, 0, 0), (1, 24, 24), (0, 11, 5), (1, 24, 0)], np.int32)
        rows = [2, 0, 3, 1]
        X, _ = ctx.gather_patch_pairs(dict(stack=ctx.to_device(stack), pad=(0, 0), mul=mul, add=add), None, ctx.to_device(table),
                                      ctx.to_device(np.array(rows, np.int32)), 0, 4, 24)
        ref = PR.gather_side(stack, table, rows, (0, 0), 24, 1, False, mul, add)
        fus = R.scale(PR.gather_side(stack, table, rows, (0, 0), 24, 1), mul, add, fused=True)
        assert_bits(X.cpu().numpy(), ref, fus, f"sr_gather_patch_pairs {stack.dtype}")
    elif op == "extract_patches":
        img = R.scale_stack("f32")[0]
        mul, add = R.SCALE_UNIT
        for p, s in ((24, 12), (11, 5)):
            got = ctx.extract_patches(ctx.to_device(img), p, s, mul=mul, add=add).cpu().numpy()
            assert_bits(got, _patches_ref(img, p, s, mul, add, False), _patches_ref(img, p, s, mul, add, True), f"sr_extract_patches patch {p}")
    else:
        _, _, _, dtype, route = op.split("_")
        frames = R.scale_stack(dtype)
        mul, add = R.SCALE_RAW_U8 if dtype == "u8" else R.SCALE_UNIT
        p, s = (24, 12) if route == "quad" else (11, 5)              # patch * C a multiple of 4, or not: extract_batch_quad / _scalar
        got = ctx.extract_patches_batch(ctx.to_device(frames), p, s, mul=mul, add=add).cpu().numpy()
        ref, fus = (np.concatenate([_patches_ref(f.astype(F32), p, s, mul, add, fz) for f in frames]) for fz in (False, True))
        assert_bits(got, ref, fus, f"sr_extract_patches_batch {dtype} {route}")
