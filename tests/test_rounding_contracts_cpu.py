"""tests/rounding_ref.py against the project's own references and the source: the unfused restatements ARE oracle.ops / classic_ref /
sr355.train bit for bit; every kernel of csrc/ that uses a rounding intrinsic or an fp_sep.h helper is in one table with the GPU test that
holds it or the reason no contraction can change its bits; and every case of tests/test_rounding_contracts_gpu.py discriminates -- the
fused reference differs from the unfused one there (the negative controls).  No GPU.

The conditions, from the formats and not from any device result: a float output needs 5 % of its elements and 32 elements to differ; a
uint8 output one position per case and eight in all.  Two cases the issue names cannot meet them, for reasons of arithmetic that the tests
below assert instead: back-projection at an exact 2x (every product that feeds a sum has a power-of-two-times-three weight on a value of
few bits and is exact) and the uint8 INTER_AREA 150 x 151 -> 100 x 99 (no sum can lie near a half-integer).  Both stay device cases.
"""
import os
import shutil
from fractions import Fraction

import numpy as np
import pytest

import classic_ref as CR
import patch_dataset_ref as PR
import rounding_ref as R
from oracle import ops as O

F32 = np.float32
MIN_SHARE, MIN_COUNT = 0.05, 32


def assert_discriminates(unfused, fused, what):
    n, total = R.differing(unfused, fused), np.asarray(unfused).size
    print(f"{what}: {n} of {total} elements differ under contraction ({100.0 * n / total:.1f} %)")
    assert n >= MIN_COUNT and n >= MIN_SHARE * total, (what, n, total)


# ---------------------------------------------------------------------------------------------------- the emulations
def test_fma32_is_one_rounding():
    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(4000).astype(F32) for _ in range(3))
    got = R.fma32(a, b, c)
    exact = np.array([float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.mean(got == exact.astype(F32)) >= 0.999               # double rounding through fp64 shows about once in 2^29
    assert R.differing(got, (a * b + c).astype(F32)) > 400          # and it is not the two-rounding result


def test_fma64_is_one_rounding():
    rng = np.random.default_rng(1)
    a, b, c = (rng.standard_normal(3000) for _ in range(3))
    got = R.fma64(a, b, c)
    exact = np.array([R.fma64_exact(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.mean(got == exact) >= 0.999
    assert R.differing(exact, a * b + c) > 300


# ---------------------------------------------------------------------------------------------------- the inventory
def test_every_kernel_with_a_rounding_intrinsic_is_in_one_table():
    found = set(R.rounding_sites())
    held, cannot = set(R.HELD_BY), set(R.CANNOT_CHANGE)
    assert not (held & cannot), held & cannot
    assert found - held - cannot == set(), f"rounding intrinsics in kernels that no table lists: {sorted(found - held - cannot)}"
    assert (held | cannot) - found == set(), f"listed but not in the source: {sorted((held | cannot) - found)}"
    assert all(len(r.split()) >= 8 for r in R.CANNOT_CHANGE.values())
    assert len(found) >= 30
    for six in (("classic.hip", "ibp_lr_kernel"), ("classic.hip", "ibp_hr_kernel"), ("classic.hip", "egi_hr_kernel"), ("classic.hip", "db2_hh_abs_kernel"),
                ("imgops.hip", "resize_apply_f32_kernel"), ("imgops.hip", "resize_apply_area_u8_kernel")):
        assert six in held


def test_the_tests_named_in_the_table_exist():
    for site, test in R.HELD_BY.items():
        module, name = test.split("::")
        src = open(os.path.join(R.ROOT, "tests", module)).read()
        assert f"def {name}(" in src and "pytest.mark.gpu" in src, (site, test)


def test_no_kernel_pairs_an_intrinsic_product_with_an_intrinsic_sum():
    """The spelling that does not hold -- a sum intrinsic whose operand is a product intrinsic -- is gone from csrc/; fp_sep.h's helpers
    replace it."""
    import re
    for f in sorted(os.listdir(R.CSRC)):
        if f.endswith((".hip", ".h")):
            text = R._strip_comments(open(os.path.join(R.CSRC, f)).read())
            assert not re.search(r"__[fd](?:add|sub)_rn\s*\([^;]*__[fd]mul_rn", text), f


def test_design_md_has_a_row_for_every_kernel():
    text = open(os.path.join(R.ROOT, "DESIGN.md")).read()
    section = text[text.index("**Two roundings where the contract says two.**"):text.index("**Synthetic weights: attention logits conditioned.**")]
    missing = [s for s in sorted(R.rounding_sites()) if f"| `{s[0]}` `{s[1]}` |" not in section]
    assert not missing, missing


def test_a_new_kernel_with_a_rounding_intrinsic_is_found(tmp_path):
    scratch = tmp_path / "csrc"
    shutil.copytree(R.CSRC, scratch)
    p = scratch / "study.hip"
    p.write_text(p.read_text() + "\n// __fmul_rn(a, b) in a comment is not a use\n"
                 "__global__ void __launch_bounds__(256) extra_kernel(const float* a, float* y) { y[0] = __fadd_rn(__fmul_rn(a[0], a[1]), y[0]); }\n"
                 "__device__ __forceinline__ double extra_fn(double a, double b) { return add_sep(mul_sep(a, b), b); }\n")
    new = set(R.rounding_sites(str(scratch))) - set(R.rounding_sites())
    assert new == {("study.hip", "extra_kernel"), ("study.hip", "extra_fn")}
    assert R.rounding_sites(str(scratch))[("study.hip", "extra_kernel")] == 2


# ---------------------------------------------------------------------------------------------------- sr_resize
@pytest.mark.parametrize("C", R.CHANNELS)
@pytest.mark.parametrize("case", R.RESIZE_F32_CASES, ids=[c[0] for c in R.RESIZE_F32_CASES])
def test_resize_f32_cases_discriminate(case, C):
    cid, shape, out, interp, data = case
    x = R.resize_input(cid, shape, C, data)
    unfused = R.cv_resize(x, *out, interp)
    assert np.array_equal(unfused.view(np.uint32), O.cv_resize(x, *out, interp).view(np.uint32))
    assert_discriminates(unfused, R.cv_resize(x, *out, interp, fused=True), f"{cid} C={C}")


def test_axis_taps_unfused_is_the_oracle_and_the_stored_pairs_are_the_search():
    for n_src, n_dst, interp in [(23, 46, O.INTER_LINEAR), (50, 17, O.INTER_AREA), (9, 37, O.INTER_AREA), (31, 62, O.INTER_LANCZOS4)]:
        a, b = R.axis_taps(n_src, n_dst, interp, interp == O.INTER_AREA and n_dst > n_src), O.resize_axis_taps(n_src, n_dst, interp, interp == O.INTER_AREA and n_dst > n_src)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # a benign pair: the fused coordinates give the same taps
        c = R.axis_taps(n_src, n_dst, interp, interp == O.INTER_AREA and n_dst > n_src, fused_coords=True)
        assert np.array_equal(a[0], c[0]) and np.array_equal(a[1].view(np.uint32), c[1].view(np.uint32))
    assert R.search_coord_pairs() == R.COORD_PAIRS and 1 <= len(R.COORD_PAIRS) <= 12
    assert all(n_dst <= 700 and n_src <= 700 for n_src, n_dst, _ in R.COORD_PAIRS)


@pytest.mark.parametrize("pair", R.COORD_PAIRS, ids=[f"{a}to{b}_interp{i}" for a, b, i in R.COORD_PAIRS])
def test_coordinate_pairs_are_not_benign(pair):
    """One element is enough here: what contraction changes is a single coordinate (an exact 0 becomes 1e-17), and with it the taps of one
    output column and row."""
    n_src, n_dst, interp = pair
    assert R.coord_pair_differs(n_src, n_dst, interp) >= 1
    for kind in ("ramp", "random"):
        x = R.coord_case_input(n_src, n_dst, interp, kind)
        unfused = R.cv_resize(x, n_dst, n_dst, interp)
        assert np.array_equal(unfused.view(np.uint32), O.cv_resize(x, n_dst, n_dst, interp).view(np.uint32))
        n = R.differing(unfused, R.cv_resize(x, n_dst, n_dst, interp, fused_coords=True))
        print(f"{pair} {kind}: {n} of {unfused.size} elements differ with fused coordinates")
        assert n >= 1


def test_area_u8_planted_image_discriminates():
    total = 0
    for cid, (shape, out) in R.AREA_U8_CASES.items():
        img, planted = R.area_u8_case(cid)
        assert img.shape == shape + (1,) and np.array_equal(R.area_u8_case(cid)[0], img)
        unfused = R.cv_resize_area_shrink_u8(img, *out)
        assert np.array_equal(unfused, O.cv_resize_area_shrink_u8(img, *out))
        diff = np.argwhere(unfused != R.cv_resize_area_shrink_u8(img, *out, fused=True))
        print(f"{cid}: planted {len(planted)} positions, {len(diff)} outputs differ under contraction")
        assert {tuple(p[:2]) for p in diff} >= set(planted)
        if cid == "issue_100x99":
            assert len(planted) == 0
        else:
            assert len(planted) >= 1
        total += len(diff)
    assert total >= 8


def test_the_issues_area_u8_size_cannot_discriminate():
    """150 x 151 -> 100 x 99: every weight is a multiple of 1/3 (rows) or 1/151 (columns) up to its fp32 rounding, so a sum of integer pixels
    is m / 453 and at least 1 / 906 from any half-integer; fused and unfused fp32 sums differ by a few 2^-17."""
    (H, W), (oh, ow) = R.AREA_U8_CASES["issue_100x99"]
    _, wx = O.resize_axis_taps(W, ow, O.INTER_AREA)
    _, wy = O.resize_axis_taps(H, oh, O.INTER_AREA)
    assert np.max(np.abs(wx * 151 - np.rint(wx * 151))) < 1e-4 and np.max(np.abs(wy * 3 - np.rint(wy * 3))) < 1e-5
    assert 453 % 2 == 1
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    v = O.cv_resize(img.astype(F32), oh, ow, O.INTER_AREA)
    assert np.min(np.abs(v - np.floor(v) - 0.5)) > 1.0 / 906 - 1e-3


# ---------------------------------------------------------------------------------------------------- the classical up-scalers
@pytest.mark.parametrize("shape", R.IBP_SHAPES)
def test_back_projection_cases_discriminate(shape):
    H, W, h, w = shape
    hr, lr = R.ibp_inputs(*shape)
    for it in R.IBP_ITERATIONS:
        unf = [R.back_projection(hr[b], lr[b], it) for b in range(R.IBP_BATCH)]
        fus = [R.back_projection(hr[b], lr[b], it, fused=True) for b in range(R.IBP_BATCH)]
        for b in range(R.IBP_BATCH):
            ref = CR.back_projection(hr[b], lr[b], it)
            assert np.array_equal(unf[b][1].view(np.uint32), ref[1].view(np.uint32)) and np.array_equal(unf[b][0], ref[0])
        est_u, est_f = np.stack([u[1] for u in unf]), np.stack([f[1] for f in fus])
        if H == 2 * h and W == 2 * w:
            # the exact 2x: the LR pass is the 2 x 2 mean (weights 0.5, exact products); the HR pass has weights 0.25 and 0.75 on differences
            # that are multiples of the estimate's ulp and small, so 3 d has 24 bits or fewer and the product is exact too
            assert R.differing(est_u, est_f) == 0
            print(f"{shape} x{it}: exact products, contraction changes nothing (the case holds the 2x rule, not the roundings)")
        else:
            assert_discriminates(est_u, est_f, f"back_projection {shape} x{it}")


@pytest.mark.parametrize("shape", R.EGI_SHAPES)
def test_edge_guided_cases_discriminate(shape):
    H, W, h, w = shape
    x = R.egi_input(*shape)
    weights = R.egi_weights(*shape)
    assert len(weights) == 4 and all(n >= 1 for _, n in weights) and all(0.3 <= wt < 0.31 for wt, _ in weights)
    total = 0
    for wt, n in weights:
        y, up_e = R.edge_guided(x, H, W, wt)
        ry, rup = CR.edge_guided(x, H, W, wt)
        assert np.array_equal(y, ry) and np.array_equal(up_e.view(np.uint32), rup.view(np.uint32))
        yf, up_ef = R.edge_guided(x, H, W, wt, fused=True)
        assert R.differing(y, yf) == n
        total += n
        print(f"edge_guided {shape} weight {wt!r}: {n} uint8 outputs differ under contraction; up_e: {R.differing(up_e, up_ef)} of {up_e.size}")
    assert total >= 4                                               # two shapes: eight positions in all


@pytest.mark.parametrize("shape", R.SIGMA_SHAPES)
def test_noise_sigma_cases_discriminate(shape):
    x = R.sigma_input(shape)
    d = R.db2_hh(x)
    assert np.array_equal(d.view(np.uint64), CR.db2_hh(x).view(np.uint64))
    nz = int(np.count_nonzero(d))
    assert nz % 2 == {(13, 19): 0, (16, 16): 1}[shape], nz        # the even count takes the mean of the middle two
    assert_discriminates(d, R.db2_hh(x, fused=True), f"db2 dd band {shape} ({nz} non-zero coefficients)")
    assert R.noise_sigma(x) == CR.noise_sigma(x) and R.noise_sigma(x, fused=True) != R.noise_sigma(x)


def test_nl_means_upscale_discriminates():
    """sr_nl_means' Lanczos up-scale is sr_resize on the fp32 denoised image (Context.non_local_means): resize_apply_f32_kernel again."""
    H, W, h, w = R.EGI_SHAPES[0]
    x = R.egi_input(H, W, h, w)
    den = CR.nl_means(x, 1.15 * CR.noise_sigma(x)).astype(F32)[None, :, :, None]
    assert_discriminates(O.cv_resize(den, H, W, O.INTER_LANCZOS4), R.cv_resize(den, H, W, O.INTER_LANCZOS4, fused=True), "nl_means Lanczos up-scale")


# ---------------------------------------------------------------------------------------------------- v * mul + add
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_scaling_cases_discriminate(dtype):
    stack = R.scale_stack(dtype)
    unit = PR.unit(stack)
    mul, add = R.SCALE_UNIT
    assert np.array_equal(R.scale(unit, mul, add).view(np.uint32), (unit * F32(mul) + F32(add)).view(np.uint32))
    assert_discriminates(R.scale(unit, mul, add), R.scale(unit, mul, add, fused=True), f"{dtype} stack in [0, 1], v * {mul} + {add}")
    assert R.differing(R.scale(unit, 2.0, -1.0), R.scale(unit, 2.0, -1.0, fused=True)) == 0     # the existing tests' x * 2 - 1 cannot
    if dtype == "u8":
        raw = stack.astype(F32)
        mul, add = R.SCALE_RAW_U8
        assert_discriminates(R.scale(raw, mul, add), R.scale(raw, mul, add, fused=True), f"float(u8), v * {mul} + {add}")


# ---------------------------------------------------------------------------------------------------- Adam, clip-by-norm
def test_the_existing_adam_tests_inputs_discriminate():
    """test_train_gpu.py::test_device_adam_is_the_host_adam_bit_for_bit's three steps, restated: the unfused step is sr355.train.Adam bit for
    bit, and the fused one differs in the moments it leaves, which that test compares as well."""
    from sr355 import train as T
    rng = np.random.default_rng(12)
    w0 = {"a": (rng.standard_normal((3, 3, 8, 16)).astype(F32), rng.standard_normal(16).astype(F32))}
    host = T.Adam(w0, 1e-4, epsilon=1e-7)
    flat = lambda d: np.concatenate([d["a"][0].ravel(), d["a"][1].ravel()])
    wh = w0
    state = {f: (flat(w0), np.zeros(flat(w0).size, F32), np.zeros(flat(w0).size, F32)) for f in (False, True)}
    for step in range(3):
        g = {"a": ((rng.standard_normal((3, 3, 8, 16)) * 10.0 ** rng.integers(-6, 2)).astype(F32), rng.standard_normal(16).astype(F32))}
        scale = 1.0 if step < 2 else 0.5
        wh = host.apply(wh, {"a": (g["a"][0] * F32(scale), g["a"][1] * F32(scale))})
        lr_t = F32(1e-4 * np.sqrt(1.0 - 0.999 ** (step + 1)) / (1.0 - 0.9 ** (step + 1)))
        for f in (False, True):
            state[f] = R.adam_step(*state[f][:1], flat(g), *state[f][1:], lr_t, gscale=scale, fused=f)
        assert np.array_equal(state[False][0].view(np.uint32), flat(wh).view(np.uint32)), step
        print(f"Adam weights after step {step + 1}: {R.differing(state[False][0], state[True][0])} of {state[False][0].size} differ under contraction")
    # a step of 1e-4 moves a weight of order 1 by a few ulp, so the weights hide the moments' last bit; the existing test compares m and v too
    assert_discriminates(state[False][1], state[True][1], "Adam first moment after three steps")
    assert_discriminates(state[False][2], state[True][2], "Adam second moment after three steps")


def test_the_clip_kernels_square_is_exact():
    """clip_by_norm_kernel's s += x * x: x an fp32 value widened to fp64, so the square has 48 bits and a fused sum is the separate one."""
    rng = np.random.default_rng(11)
    g = (rng.standard_normal(4097) * 10.0 ** rng.integers(-6, 3, 4097)).astype(F32)
    x = g.astype(np.float64)
    p, e = R.two_prod(x, x)
    assert np.all(e == 0)
    assert R.sum_squares_f64(g[:600], fused=True) == R.sum_squares_f64(g[:600], fused=False)
