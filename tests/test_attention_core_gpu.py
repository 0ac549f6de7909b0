"""The SelfAttention core (csrc/attention.hip) alone, per element, on every key-loop path.

sr_self_attention is run with 0/1 selector weights (attention_ref.run_core), which makes both of its convs exact copies: what
comes back is bit for bit what the core stored.  It is compared with the fp64 softmax of the values the core received
(attention_ref.core_fp64) under the derived per-element bound (attention_ref.bound): every element, no norm.  The gather
cases are compared bit for bit.  tests/test_attention_core_cpu.py shows on the same inputs which path every wave and key
group takes (first / unguarded / guarded_pass / redo@0..3 / tail_ragged / tail_whole_tiles, both special threshold
branches) and that this comparison rejects seven injected faults.

Worst err / bound observed on an MI355X, per family (bf16 | f32):
    gauss1 0.39 | 0.011    gauss15 0.72 | 0.035    zero_queries 0.61 | 0.003    minus400 0.15 | 0.022    norm_table 0.34 | 0.026
    gather: bit-exact in both dtypes.  The module takes 2.6 s (72 tests).
gauss15 bf16 is above 0.5 because its rows are nearly one-hot: the store's half spacing alone is a third of the bound and
rounding attains it, and where the kernel takes probabilities against a stale maximum the leading one is no longer exactly 1,
so it draws a 2^-8 rounding of its own (the emulation with the true maximum reads 0.57, with a stale one 0.7).  zero_queries
bf16 is the wave of zero queries, whose bound is little more than the store's half spacing.  The f32 bound charges every
accumulation step a whole ulp in the same direction, hence the small ratios.
"""
import numpy as np
import pytest

import attention_ref as R

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f32"]
BY_FAMILY = {}
for _name, _c in R.cases("bf16").items():
    BY_FAMILY.setdefault(_c["family"], []).append(_name)


def _run_and_check(ctx, name, dtype):
    c = R.cases(dtype)[name]
    got = R.run_core(ctx, c["k"], c["q"], c["v"], dtype)
    ref, bnd = R.reference(name, dtype)
    ratio = R.worst_ratio(got, ref, bnd)
    print(f"{name} {dtype}: worst err/bound = {ratio:.3f}")
    assert got.shape == ref.shape
    assert ratio <= 1.0, (name, dtype, ratio, np.argwhere(~(np.abs(got - ref) <= bnd))[:8].tolist())
    return c, got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", BY_FAMILY["gather"])
def test_exact_gather(ctx, name, dtype):
    """Ternary keys, queries 32 x the target's code: the target leads every other key by 46 bits (32 nats), the leak is far
    below half an ulp, and the core must return the target's value row bit for bit -- through group 0, unguarded groups,
    passing guarded groups, a redo at tile 0..3 of the last full group, the ragged tail, and a near-permutation whose maxima grow in
    almost every group; the two images of a case take different paths."""
    c = R.cases(dtype)[name]
    got = R.run_core(ctx, c["k"], c["q"], c["v"], dtype)
    want = np.stack([c["v"][b][c["pi"][b]] for b in range(c["v"].shape[0])])
    bad = np.argwhere(got != want)
    assert bad.size == 0, (name, dtype, len(bad), bad[:8].tolist())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", BY_FAMILY["gauss1"] + BY_FAMILY["gauss15"])
def test_gaussian_families(ctx, name, dtype):
    """Score sd ~ 1 (everything unguarded: a stale maximum is the norm) and ~ 15 (the maximum grows in varying lanes, often in
    only one of a wave's two query blocks: the lane + 16 denominator rescale), at every N where the key loop or the staging changes."""
    _run_and_check(ctx, name, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_queries_give_the_mean_of_v(ctx, dtype):
    """One whole wave of image 1 has all-zero queries (threshold +inf, every group unguarded): every probability is exactly 1, so
    the bound there carries no probability-rounding term -- accumulation and the store only -- around the plain mean of V."""
    c, got = _run_and_check(ctx, "zero_queries", dtype)
    b, q0, q1 = c["zero"]
    ref, _ = R.reference("zero_queries", dtype)
    assert np.abs(ref[b, q0:q1] - c["v"][b].mean(axis=0)).max() <= 1e-14
    assert (got[b, q0:q1] == got[b, q0]).all()                    # identical queries, identical rows


@pytest.mark.parametrize("dtype", DTYPES)
def test_scores_near_minus_400(ctx, dtype):
    """Every score about -400 plus noise: the running maxima sit far below -GROW_OK, the threshold is -1 and the bound unreachable,
    so every full group runs guarded and passes."""
    _run_and_check(ctx, "minus400", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_per_image_key_norm_table(ctx, dtype):
    """One group of 64x larger keys, group 2 in image 0 and group 3 in image 1: only the image's own row of the key-norm table sends
    that group through the guard and the redo; with the other image's row it would run unguarded up to 2^240 above the running
    maximum and overflow."""
    _, got = _run_and_check(ctx, "norm_table", dtype)
    assert np.isfinite(got).all()
