"""The case tables of tests/classic_cases.py do what they claim, on the fp64 restatements alone (no GPU needed): which NL-means cases cut
weights and how many, that the cutoff case sits on dist == 5.0 exactly and that `<` for `<=` would show, that the seven hf_radius_frac values
give seven masks, that the refusal table is complete, and that the scale-1 shapes have the fixed points the device test expects.  The
extension of classic_ref (nl_means_dist / nl_means_of_dist) is held to nl_means bit for bit, and nl_means to skimage's loop structure."""
import numpy as np
import pytest

import classic_cases as K
import classic_ref as CR
import metrics_ref as MR

IDS = [K.nlm_id(c) for c in K.NLM_CASES]


def test_table_covers_the_arguments_and_geometry_it_names():
    assert len(set(K.NLM_CASES)) == len(K.NLM_CASES)
    at_main = {(p, d) for (h, w, p, d, hs) in K.NLM_CASES if (h, w) == (33, 65)}
    assert at_main == set(K.PATCH_DISTANCE) == {(5, 6), (1, 0), (1, 12), (9, 12), (9, 0), (3, 1), (7, 2)}
    for p, d in K.PATCH_DISTANCE:                                  # the default regime and two others for every argument pair
        hs = [c[4] for c in K.NLM_CASES if c[:4] == (33, 65, p, d)]
        assert hs[0] == K.H_DEFAULT and len(set(hs)) == 3, (p, d, hs)
        assert p % 2 == 1 and 1 <= p <= 9 and 0 <= d <= 12         # what sr_nl_means accepts
    assert K.H_SCALES == (1.15, 0.02, 0.008)
    shapes = {c[:2] for c in K.NLM_CASES}
    assert shapes == set(K.GEOMETRY) == {(32, 32), (33, 65), (5, 7), (1, 9), (40, 1), (40, 3)}
    T = K.NLM_TILE
    assert 32 % T == 0 and 33 % T and 65 % T and 33 > T and 65 > 2 * T and 40 > T
    # 5 x 7 at distance 12: numpy's reflect period is 2 (n - 1); the halo s + d is at least a whole period on both axes (a second bounce
    # starts n - 1 pixels out), and with patch 9 more than one
    for p in (1, 9):
        assert (5, 7, p, 12, K.H_DEFAULT) in K.NLM_CASES and p // 2 + 12 >= 2 * (7 - 1) > 2 * (5 - 1)
    assert 9 // 2 + 12 > 2 * (7 - 1)
    for hw in ((1, 9), (40, 1), (40, 3), (5, 7)):                  # every small shape runs a large halo, the default and a selective regime
        assert {c[2:4] for c in K.NLM_CASES if c[:2] == hw} >= {(9, 12), (5, 6)}
        assert len({c[4] for c in K.NLM_CASES if c[:2] == hw}) == 2
    assert len(K.SIGMAS) == 2 and K.SIGMAS[0] != K.SIGMAS[1]
    for hw in shapes:                                              # the two images of a batch differ, and both levels are in each
        x = K.nlm_images(*hw)
        assert x.dtype == np.uint8 and x.shape == (2,) + hw and not np.array_equal(x[0], x[1])
        assert all(im.min() < 100 and im.max() > 160 for im in x)


@pytest.mark.parametrize("case", K.NLM_CASES, ids=IDS)
def test_cut_share_of_each_case(case):
    """The default regime cuts nothing and weighs everything ~1 (all the device tests had before); a selective case cuts between 5 % and 95 % of
    the (pixel, shift) pairs of each image; distance 0 has one shift, never cut, and returns x / 255."""
    h, w, p, d, hs = case
    ref, cuts = K.nlm_reference(case)
    assert ref.shape == (2, h, w) and np.isfinite(ref).all()
    if K.nlm_selective(case):
        assert all(0.05 <= c <= 0.95 for c in cuts), cuts
    else:
        assert cuts == (0.0, 0.0)
    if hs == K.H_DEFAULT:
        for img, sigma in zip(K.nlm_images(h, w), K.SIGMAS):
            assert CR.nl_means_dist(img, hs * sigma, p, d)[0].max() <= 0.05       # D / 65025 <= patch^2, so dist <= 1 / h^2 <= 1 / 4.6^2: every weight above 0.95
    if d == 0:
        assert np.array_equal(ref, K.nlm_images(h, w) / 255.0)


def test_default_regime_of_the_existing_device_tests_cuts_nothing():
    """The finding: on a noisy natural-looking image with its own sigma estimate, h = 1.15 sigma never reaches the cutoff."""
    from sr355.synth import hr_tile
    rng = np.random.default_rng(7)
    x = np.clip(hr_tile(rng, 33, 24)[:, :, 0].astype(np.float64) * 255.0 + rng.normal(0, 6.0, (33, 24)), 0, 255).astype(np.uint8)
    dist = CR.nl_means_dist(x, 1.15 * CR.noise_sigma(x))[0]
    assert dist.max() <= 0.02
    assert 0.05 <= np.mean(CR.nl_means_dist(x, 0.02 * CR.noise_sigma(x))[0] > 5.0) <= 0.95


def test_wrapper_case_is_selective_at_the_images_own_sigma():
    """Context.non_local_means(patch_size=7, patch_distance=2, h_scale=0.02) on the 33 x 65 images, with sigma estimated, not supplied."""
    for img in K.nlm_images(33, 65):
        sigma = CR.noise_sigma(img)
        assert np.isfinite(sigma) and sigma > 0
        assert 0.05 <= np.mean(CR.nl_means_dist(img, 0.02 * sigma, 7, 2)[0] > 5.0) <= 0.95


def test_dist_extension_is_nl_means_bit_for_bit():
    for case in K.NLM_CASES:
        h, w, p, d, hs = case
        if (h, w) == (33, 65) and d == 12:
            continue                                               # 625 shifts at the largest shape twice over: the 5 x 7 cases run d = 12
        for img, sigma, ref in zip(K.nlm_images(h, w), K.SIGMAS, K.nlm_reference(case)[0]):
            assert np.array_equal(ref, CR.nl_means(img, hs * sigma, p, d)), case


def test_gather_matches_the_pair_loop_at_every_new_argument():
    """classic_ref.nl_means against skimage's loop structure at every (patch, distance, h) of the table, on one small image."""
    x = K.structured_small(12, 15, seed=3)
    seen = set()
    for (_, _, p, d, hs) in K.NLM_CASES:
        for sigma in K.SIGMAS:
            key = (p, d, hs * sigma)
            if key in seen:
                continue
            seen.add(key)
            a = CR.nl_means(x, hs * sigma, p, d)
            b = CR.nl_means_pairloop(x, hs * sigma, p, d)
            assert np.max(np.abs(a - b)) <= 1e-12, key
    assert len(seen) >= 2 * 3 * len(K.PATCH_DISTANCE)
    # and at the cutoff case's arguments, off the boundary itself (the pair loop squares x / 255 in floating point)
    c = K.cutoff_image()[:12, :15]
    for sigma in K.CUTOFF_SIGMAS[1:]:
        a = CR.nl_means(c, K.CUTOFF_H_SCALE * sigma, K.CUTOFF_PATCH, K.CUTOFF_DISTANCE)
        b = CR.nl_means_pairloop(c, K.CUTOFF_H_SCALE * sigma, K.CUTOFF_PATCH, K.CUTOFF_DISTANCE)
        assert np.max(np.abs(a - b)) <= 1e-12


def test_cutoff_case_sits_on_the_boundary():
    s0, s_lo, s_hi = K.CUTOFF_SIGMAS
    assert 65025 / 65025.0 / (s0 * s0 * K.CUTOFF_PATCH * K.CUTOFF_PATCH) == 5.0 and abs(s0 * s0 - 0.2) < 1e-16
    x = K.cutoff_image()
    assert set(np.unique(x)) == {0, 255}
    args = (K.CUTOFF_PATCH, K.CUTOFF_DISTANCE)
    dist, vals = CR.nl_means_dist(x, K.CUTOFF_H_SCALE * s0, *args)
    assert np.mean(dist == 5.0) >= 0.1 and not np.any(dist > 5.0)
    kept = CR.nl_means_of_dist(dist, vals, dist <= 5.0)
    dropped = CR.nl_means_of_dist(dist, vals, dist < 5.0)
    assert np.array_equal(kept, CR.nl_means(x, K.CUTOFF_H_SCALE * s0, *args))
    assert K.steps(dropped, kept).min() > 100                     # `<` for `<=` moves EVERY pixel by more than 100 times the tolerance
    # the neighbouring sigmas: the same pairs just past the boundary (cut), and just inside it (kept); nothing on it
    d_lo = CR.nl_means_dist(x, K.CUTOFF_H_SCALE * s_lo, *args)[0]
    d_hi = CR.nl_means_dist(x, K.CUTOFF_H_SCALE * s_hi, *args)[0]
    assert np.array_equal(d_lo > 5.0, dist == 5.0) and not np.any(d_lo == 5.0)
    assert not np.any(d_hi >= 5.0) and np.array_equal((d_hi > 4.99), dist == 5.0)


def test_refusal_table_is_complete():
    rows = {name: (p, d, B, sig) for name, p, d, B, sig in K.NLM_REFUSALS}
    assert len(rows) == len(K.NLM_REFUSALS)
    valid = lambda p, d, B, sig: p % 2 == 1 and 1 <= p <= 9 and 0 <= d <= 12 and B >= 1 and sig
    assert not any(valid(*r) for r in rows.values())
    assert {r[0] for r in rows.values() if valid(5, *r[1:])} == {0, 4, 11, -1}          # wrong in the patch alone
    assert {r[1] for r in rows.values() if valid(r[0], 6, *r[2:])} == {-1, 13}          # in the distance alone
    assert [r for r in rows.values() if valid(r[0], r[1], 2, r[3])] == [(5, 6, 0, True)]
    assert [r for r in rows.values() if valid(r[0], r[1], r[2], True)] == [(5, 6, 2, False)]


def test_hf_masks_and_scores_tell_the_fractions_apart():
    assert K.HF_FRACS == (-0.5, 0.0, 0.25, 0.6, 0.999, 1.0, 1.5)
    sizes = tuple(int(MR.hf_mask(20, 23, f).sum()) for f in K.HF_FRACS)
    assert sizes == K.HF_MASK_SIZES_20x23 == (460, 459, 415, 219, 2, 0, 0)
    assert len(set(sizes[:-1])) == 6
    k = MR.NAMES.index("hf_ratio")
    for H, W in K.HF_SHAPES:
        for C in (1, 3):
            hr, sr = K.hf_pair(H, W, C)
            assert hr.dtype == sr.dtype == np.uint8 and hr.shape == ((H, W) if C == 1 else (H, W, 3))
            s = {f: MR.scores(hr, sr, radius_frac=f) for f in (0.25, 0.6, 1.0, 1.5)}
            assert abs(s[0.25][k] - s[0.6][k]) > 1e-3              # a device that ignored the argument cannot pass
            assert s[1.0][k] == 1.0 and s[1.5][k] == 1.0            # the empty mask: (0 + 1e-9) / (0 + 1e-9)
            others = [i for i in range(len(MR.NAMES)) if i != k]
            assert s[0.25][others].tobytes() == s[0.6][others].tobytes() == s[1.5][others].tobytes()


def test_unit_scale_shapes_and_their_fixed_points():
    assert K.UNIT_SCALE_SHAPES == ((24, 30, 24, 15), (24, 30, 12, 30), (24, 30, 24, 30), (9, 7, 8, 7), (2, 2, 1, 1))
    for H, W, h, w in K.UNIT_SCALE_SHAPES:
        assert H >= h and W >= w and (H == h or W == w or (h, w) == (1, 1))
        hr, lr = K.unit_scale_pair(H, W, h, w)
        assert hr.shape == (H, W) and lr.shape == (h, w)
        for interp in (CR.O.INTER_LINEAR, CR.O.INTER_LANCZOS4):    # an axis of scale 1 is the identity of that axis: one tap of weight 1
            for n, N in ((h, H), (w, W)):
                idx, wgt = CR.O.resize_axis_taps(n, N, interp)
                if n == N:
                    assert np.array_equal((wgt * (idx == np.arange(n)[:, None])).sum(1), np.ones(n)) and np.count_nonzero(wgt) == n
    hr, lr = K.unit_scale_pair(24, 30, 24, 30)
    assert not np.array_equal(hr, lr)
    # equal sizes: both resizes are the identity, so one iteration gives hr + (lr - hr): the observation, whatever the starting estimate ...
    y, est = CR.back_projection(hr, lr, 3)
    assert np.array_equal(y, lr) and np.array_equal(est, lr.astype(np.float32))
    # ... and a starting estimate that already is the observation comes back as passed
    assert np.array_equal(CR.back_projection(hr, hr, 3)[0], hr)
    f = CR.freq_extrapolate(lr, 24, 30)
    assert np.max(np.abs(f - lr)) <= 1e-12 * np.max(f)
    assert np.isnan(CR.noise_sigma(K.unit_scale_pair(2, 2, 1, 1)[1]))
    assert all(np.isfinite(CR.noise_sigma(K.unit_scale_pair(*s)[1])) for s in K.UNIT_SCALE_SHAPES[:4])
