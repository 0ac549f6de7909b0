"""The classical kernels with their arguments moved off the notebook's defaults (csrc/classic.hip, csrc/metrics.hip), per element against the
fp64 restatements of tests/classic_ref.py and tests/metrics_ref.py.  The tables and images are in tests/classic_cases.py;
tests/test_classic_args_cpu.py proves what they claim.

1. sr_nl_means through the C ABI with a sigma tensor the test fills: every accepted (patch, distance) at the default h_scale, where no
   weight is cut, and at selective ones, where 5 % to 95 % are; tile remainders, images smaller than the halo, axes of length 1; the cutoff
   dist == 5.0 itself; refusals; a poisoned output buffer; a non-finite sigma for one image of a batch.  One fp32 step of tolerance.
2. Context.classic_scores' hf_radius_frac at seven values with seven masks.
3. The four up-scalers with an axis, or both, at scale 1."""
import math

import numpy as np
import pytest
import torch

import classic_cases as K
import classic_ref as CR
import metrics_ref as MR
from sr355 import _lib as L

pytestmark = pytest.mark.gpu

GUARD = 4096                      # bytes of poison on either side of an output
F32_NAN_BITS = 0x7FC0DEAD


def dev(ctx, a):
    """uint8 NumPy -> device tensor, through a copy: the case images are shared between tests and read-only."""
    assert a.dtype == np.uint8
    return ctx.to_device(np.array(a))


class GuardedF32:
    """n float32 in the middle of a buffer of one NaN bit pattern, GUARD bytes of it on either side."""

    def __init__(self, ctx, n):
        self.g, self.n = GUARD // 4, n
        self.buf = torch.empty(n + 2 * self.g, dtype=torch.float32, device=ctx.torch_device)
        self.buf.view(torch.int32).fill_(F32_NAN_BITS)
        self.y = self.buf[self.g:self.g + n]

    def guards_untouched(self):
        torch.cuda.synchronize()
        guard = torch.cat([self.buf[:self.g], self.buf[self.g + self.n:]]).view(torch.int32)
        return bool((guard == F32_NAN_BITS).all().item())

    def poison_left(self):
        """how many elements of the output still hold the poison pattern"""
        torch.cuda.synchronize()
        return int((self.y.view(torch.int32) == F32_NAN_BITS).sum().item())


def nl_means_raw(ctx, x, sigmas, patch, distance, h_scale, B=None, with_sigma=True):
    """sr_nl_means on x [B, h, w] uint8 with the given per-image sigmas, into a guarded buffer -> (return code, the buffer)."""
    n, h, w = x.shape
    xd = dev(ctx, x)
    sd = torch.tensor([float(s) for s in sigmas], dtype=torch.float64, device=ctx.torch_device)
    assert sd.numel() == n
    out = GuardedF32(ctx, n * h * w)
    rc = ctx.lib.sr_nl_means(ctx.h, xd.data_ptr(), n if B is None else B, h, w, int(patch), int(distance), sd.data_ptr() if with_sigma else None,
                             float(h_scale), out.y.data_ptr(), ctx.stream())
    torch.cuda.synchronize()
    return rc, out


def nl_means_checked(ctx, x, sigmas, patch, distance, h_scale):
    """-> float32 [B, h, w] as NumPy, after asserting that the guards are intact and every output element was stored."""
    rc, out = nl_means_raw(ctx, x, sigmas, patch, distance, h_scale)
    ctx.check(rc)
    assert out.guards_untouched(), "sr_nl_means wrote outside its output"
    assert out.poison_left() == 0, "sr_nl_means left output elements unwritten"
    return out.y.cpu().numpy().reshape(x.shape)


def report(name, got, ref, cuts):
    st = K.steps(got, ref)
    exact = float(np.mean(got == ref.astype(np.float32)))
    print(f"nl_means {name}: cut share {'/'.join(f'{c:.3f}' for c in cuts)}  worst |got - ref| {st.max():.3f} fp32 steps  equal to float32(ref): {exact:.4f}")
    return st


# ------------------------------------------------------------------------------------------------ 1. sr_nl_means
@pytest.mark.parametrize("case", K.NLM_CASES, ids=[K.nlm_id(c) for c in K.NLM_CASES])
def test_nl_means_per_element(ctx, case):
    """Tolerance: dist is an exact int32 SSD divided twice in fp64 in NumPy's order and h2s2 the same product chain, so the device's cutoff
    decisions are the restatement's; the sums run in the same shift order in fp64.  Only exp and a possible fma in swp += wt * v differ:
    <= 625 terms x a few 2^-53, ~1e-13 relative, before the one rounding to float32 (half a step).  One step is asserted."""
    h, w, p, d, hs = case
    x = K.nlm_images(h, w)
    ref, cuts = K.nlm_reference(case)
    got = nl_means_checked(ctx, x, K.SIGMAS, p, d, hs)
    st = report(K.nlm_id(case), got, ref, cuts)
    assert st.max() <= 1.0, (np.unravel_index(np.argmax(st), st.shape), st.max())
    if d == 0:                                                     # one shift of weight 1: x / 255 rounded to float32, exactly
        assert np.array_equal(got, (x / 255.0).astype(np.float32))


def test_nl_means_keeps_the_weight_at_the_cutoff(ctx):
    """Image 0: every pair of a 0 and a 255 pixel has dist == 5.0 exactly (48 % of the pairs), which `<=` keeps; dropping them would move every
    output by thousands of steps.  Images 1 and 2: sigma a relative 1e-12 below and above, where the same pairs are just cut and just kept."""
    x = np.stack([K.cutoff_image()] * 3)
    got = nl_means_checked(ctx, x, K.CUTOFF_SIGMAS, K.CUTOFF_PATCH, K.CUTOFF_DISTANCE, K.CUTOFF_H_SCALE)
    for b, sigma in enumerate(K.CUTOFF_SIGMAS):
        dist, vals = CR.nl_means_dist(x[b], K.CUTOFF_H_SCALE * sigma, K.CUTOFF_PATCH, K.CUTOFF_DISTANCE)
        ref = CR.nl_means_of_dist(dist, vals, dist <= 5.0)
        st = report(f"cutoff sigma {sigma.hex()} (dist == 5.0 for {np.mean(dist == 5.0):.3f} of the pairs)", got[b], ref, (float(np.mean(dist > 5.0)),))
        assert st.max() <= 1.0, (b, st.max())
        if b == 0:                                                 # and nowhere near what `<` would give
            assert K.steps(got[0], CR.nl_means_of_dist(dist, vals, dist < 5.0)).min() > 100
    assert K.steps(got[1], got[0].astype(np.float64)).min() > 100  # just past the boundary the same pairs are gone ...
    assert K.steps(got[2], got[0].astype(np.float64)).max() <= 1.0  # ... and just inside it they weigh what they weigh on it


@pytest.mark.parametrize("row", K.NLM_REFUSALS, ids=[r[0] for r in K.NLM_REFUSALS])
def test_nl_means_refusals_launch_nothing(ctx, row):
    _, patch, distance, B, with_sigma = row
    x = K.nlm_images(32, 32)
    rc, out = nl_means_raw(ctx, x, K.SIGMAS, patch, distance, 0.02, B=B, with_sigma=with_sigma)
    assert rc == L.SR_ERR_INVALID
    assert out.guards_untouched() and out.poison_left() == out.n
    with pytest.raises(ValueError):
        ctx.check(rc)


@pytest.mark.parametrize("bad", [0.0, float("nan")])
def test_nl_means_non_finite_sigma_stays_in_its_image(ctx, bad):
    x = K.nlm_images(33, 65)
    good = K.SIGMAS[1]
    for slot in (0, 1):
        sig = [good, good]
        sig[slot] = bad
        got = nl_means_checked(ctx, x, sig, 5, 6, 0.02)
        alone = nl_means_checked(ctx, x[1 - slot:2 - slot], [good], 5, 6, 0.02)
        assert not np.isfinite(got[slot]).any()
        assert got[1 - slot].tobytes() == alone[0].tobytes()
        assert np.isfinite(alone).all()


def test_non_local_means_wrapper_off_the_defaults(ctx):
    """Context.non_local_means with patch_size, patch_distance and h_scale all moved: the device's own sigma (held to the restatement's), the
    denoised image within one step of nl_means at that sigma, the Lanczos up-size at the existing 2e-5."""
    H, W = 70, 80
    lr = K.nlm_images(33, 65)
    up, den, sigma = ctx.non_local_means(dev(ctx, lr), H, W, patch_size=7, patch_distance=2, h_scale=0.02, raw=True)
    sigma = sigma.cpu().numpy()
    for b in range(2):
        ref_sigma = CR.noise_sigma(lr[b])
        assert abs(sigma[b] - ref_sigma) <= 1e-12 * ref_sigma
        dist, vals = CR.nl_means_dist(lr[b], 0.02 * float(sigma[b]), 7, 2)
        cut = float(np.mean(dist > 5.0))
        assert 0.05 <= cut <= 0.95
        ref = CR.nl_means_of_dist(dist, vals, dist <= 5.0)
        st = report(f"wrapper image {b} p7 d2 h0.02 sigma {sigma[b]:.4f}", den[b].cpu().numpy(), ref, (cut,))
        assert st.max() <= 1.0
        ref_up = CR.resize_f64(ref, H, W, CR.O.INTER_LANCZOS4)
        assert np.max(np.abs(up[b].cpu().numpy() - ref_up)) <= 2e-5
    with pytest.raises(ValueError):
        ctx.non_local_means(dev(ctx, lr), H, W, patch_distance=13)


# ------------------------------------------------------------------------------------------------ 2. hf_radius_frac
HF = MR.NAMES.index("hf_ratio")


def assert_scores(got, ref):
    """test_classic_metrics_gpu.py's per-column tolerances for uint8 pairs."""
    for k, name in enumerate(MR.NAMES):
        g, r = float(got[k]), float(ref[k])
        if math.isnan(r) or math.isinf(r):
            assert (math.isnan(g) and math.isnan(r)) or g == r, (name, g, r)
        elif name == "ssim":
            assert abs(g - r) <= 1e-9, (name, g, r)
        else:
            rel = {"grad_mse": 1e-5, "epi": 1e-5, "hf_ratio": 1e-9}.get(name, 1e-12)
            assert abs(g - r) <= rel * abs(r), (name, g, r, abs(g - r) / abs(r))


@pytest.mark.parametrize("C", [1, 3], ids=["gray", "rgb"])
@pytest.mark.parametrize("H,W", K.HF_SHAPES)
def test_hf_radius_frac(ctx, H, W, C):
    hr, sr = K.hf_pair(H, W, C)
    hd, sd = dev(ctx, hr[None]), dev(ctx, sr[None])
    rows = {}
    for f in K.HF_FRACS:
        rows[f] = ctx.classic_scores(hd, sd, hf_radius_frac=f).cpu().numpy()[0]
        ref = MR.scores(hr, sr, radius_frac=f)
        print(f"hf_ratio {H}x{W}x{C} frac {f}: device {rows[f][HF]!r} restatement {ref[HF]!r}")
        assert_scores(rows[f], ref)
        if f >= 1.0:
            assert rows[f][HF] == 1.0                              # the empty mask
    others = [k for k in range(len(MR.NAMES)) if k != HF]
    for f in K.HF_FRACS:                                           # the other eight columns do not see the argument
        assert rows[f][others].tobytes() == rows[0.6][others].tobytes(), f
    assert rows[0.6].tobytes() == ctx.classic_scores(hd, sd).cpu().numpy()[0].tobytes()      # 0.6 is the default
    assert len({float(rows[f][HF]) for f in K.HF_FRACS}) == 6


@pytest.mark.parametrize("f", [float("nan"), float("inf"), float("-inf")])
def test_hf_radius_frac_not_finite_is_refused(ctx, f):
    hr, sr = K.hf_pair(20, 23, 1)
    hd, sd = dev(ctx, hr[None]), dev(ctx, sr[None])
    dr = torch.full((1,), 255.0, dtype=torch.float64, device=ctx.torch_device)
    out = torch.full((1, len(MR.NAMES)), -7.0, dtype=torch.float64, device=ctx.torch_device)
    rc = ctx.lib.sr_classic_scores(ctx.h, hd.data_ptr(), L.DTYPE_U8, sd.data_ptr(), L.DTYPE_U8, 1, 20, 23, 1, dr.data_ptr(), f, out.data_ptr(),
                                   None, None, None, None, ctx.stream())
    torch.cuda.synchronize()
    assert rc == L.SR_ERR_INVALID and bool((out == -7.0).all().item())
    with pytest.raises(ValueError):
        ctx.classic_scores(hd, sd, hf_radius_frac=f)


# ------------------------------------------------------------------------------------------------ 3. the up-scalers at scale 1
def same_bits(got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    return got.dtype == ref.dtype and got.shape == ref.shape and got.tobytes() == ref.tobytes()


@pytest.mark.parametrize("H,W,h,w", K.UNIT_SCALE_SHAPES)
def test_upscalers_at_scale_one(ctx, H, W, h, w):
    hr, lr = K.unit_scale_pair(H, W, h, w)
    hd, ld = dev(ctx, hr[None]), dev(ctx, lr[None])

    y, est = ctx.back_projection(hd, ld, 3, raw=True)
    ref_y, ref_est = CR.back_projection(hr, lr, 3)
    assert same_bits(est[0].cpu().numpy(), ref_est) and same_bits(y[0].cpu().numpy(), ref_y)

    y, up_e = ctx.edge_guided(ld, H, W, raw=True)
    ref_y, ref_up_e = CR.edge_guided(lr, H, W)
    assert same_bits(up_e[0].cpu().numpy(), ref_up_e) and same_bits(y[0].cpu().numpy(), ref_y)

    f = ctx.freq_extrapolate(ld, H, W)[0].cpu().numpy()
    ref_f = CR.freq_extrapolate(lr, H, W)
    assert f.dtype == np.float64 and np.max(np.abs(f - ref_f)) <= 1e-12 * np.max(ref_f)

    up, den, sigma, flag = ctx.non_local_means(ld, H, W, raw=True, check=False)
    ref_sigma = CR.noise_sigma(lr)
    assert same_bits(sigma.cpu().numpy(), np.array([ref_sigma]))
    if math.isnan(ref_sigma):                                      # the 1 x 1 image: no detail coefficient at all
        assert bool(flag[0]) and not np.isfinite(den.cpu().numpy()).any() and not np.isfinite(up.cpu().numpy()).any()
        with pytest.raises(ValueError):
            ctx.non_local_means(ld, H, W)
    else:
        ref_den = CR.nl_means(lr, 1.15 * ref_sigma)
        st = report(f"scale one {(H, W, h, w)}", den[0].cpu().numpy(), ref_den, (0.0,))
        assert not bool(flag[0]) and st.max() <= 1.0
        assert np.max(np.abs(up[0].cpu().numpy() - CR.resize_f64(ref_den, H, W, CR.O.INTER_LANCZOS4))) <= 2e-5

    if (H, W) == (h, w):
        # both resizes are the identity: one iteration gives hr + (lr - hr), the observation, whatever the starting estimate; a starting
        # estimate that already is the observation comes back as passed
        assert np.array_equal(ctx.back_projection(hd, ld, 3)[0].cpu().numpy(), lr)
        assert np.array_equal(ctx.back_projection(hd, hd, 3)[0].cpu().numpy(), hr)
        assert np.array_equal(ctx.back_projection(ld, ld, 1)[0].cpu().numpy(), lr)
        assert np.max(np.abs(f - lr)) <= 1e-12 * np.max(ref_f)      # the spectrum is not padded: the input values
        assert same_bits(up[0].cpu().numpy(), den[0].cpu().numpy())                 # Lanczos at scale 1: one tap of weight 1
