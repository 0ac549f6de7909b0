"""The fused dense-block kernels (csrc/dense_fused.hip: dense_pair_fused<bf16>, dense_tail_fused<bf16,conv4+conv5>, plain and SEAM) give
the same BITS as before their compute waves carried operand reads across granule barriers: every accumulator still receives the same MFMAs
in the same order, so equality is the criterion and there is no tolerance.

Shapes: the ones of test_dense_fused_elementwise_gpu.py that cut the row stream everywhere it can be cut, plus the bench shape and one
two-up (SEAM) case.  Random seeded weights, two RRDBs (a launch with the second skip is included), taps on conv1, conv2, conv3 and conv5 of
every dense block.  Each forward runs twice and must return identical bytes; a SHA-256 per tap is compared with the value recorded on the
GPU from the commit before the change (tests/golden/dense_prefetch_bits.json, written by tests/golden/make_dense_prefetch_bits.py)."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import dense_ref as D
from sr355 import Context, Model

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_prefetch_bits.json")
PAIR, TAIL = "dense_pair_fused<bf16>", "dense_tail_fused<bf16,conv4+conv5>"
MASKS = {
    "mid": (Context.FUSED_DENSE_MID, {PAIR}),
    "tail": (Context.FUSED_DENSE_TAIL, {TAIL}),
    "three": (Context.FUSED_TWO_UP, {PAIR, TAIL}),      # 48-pixel rows: every fused dense kernel, no seam
    "all": (Context.FUSED_ALL, {PAIR, TAIL}),           # 24-pixel rows: two-up, the SEAM instances
}
# (B, H, W, grid cap)
CASES_48 = [(5, 9, 48, 2), (2, 17, 48, 0), (9, 8, 48, 4), (3, 48, 48, 0)]
CASE_24 = (7, 24, 24, 2)
PARAMS = [(c, mk) for c in CASES_48 for mk in ("mid", "tail", "three")] + [(CASE_24, "all")]
SEED, NUM_BLOCKS = 4000, 2

_MODEL = []


def key_of(case, mask_name):
    return "x".join(map(str, case)) + "|" + mask_name


def tap_hashes(ctx, case, mask_name):
    """-> {tap name: sha256 hex of the fp32 NHWC tap}; the forward runs twice and both runs must agree byte for byte."""
    B, H, W, cap = case
    mask, fused = MASKS[mask_name]
    if not _MODEL:
        m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=NUM_BLOCKS, growth_channels=32, use_attention=False, ctx=ctx)
        m.set_weights(D.random_weights(m.layer_shapes(), SEED))
        _MODEL.append(m)
    m = _MODEL[0]
    x = D.rbf(np.random.default_rng(B * 1000 + H * 10 + W).uniform(-1, 1, (B, H, W, 3)))
    xd = ctx.to_device(x.astype(np.float32), torch.bfloat16)
    blocks = [f"rrdb_{b}_dense{d}" for b in range(NUM_BLOCKS) for d in (1, 2, 3)]
    names = [f"{n}_conv{k}" for n in blocks for k in (1, 2, 3, 5)]
    ctx.set_fused(mask, cap)
    try:
        runs = []
        for _ in range(2):
            ctx.profile_begin()
            _, taps = m.forward_with_taps(xd, names)
            ran = {r["kernel"] for r in ctx.profile_end()}
            assert fused <= ran, (mask_name, ran)
            runs.append({n: np.ascontiguousarray(taps[n].float().cpu().numpy()).tobytes() for n in names})
    finally:
        ctx.set_fused(ctx.FUSED_ALL, 0)
    for n in names:
        assert runs[0][n] == runs[1][n], f"{key_of(case, mask_name)} {n}: two runs of the same forward differ"
    return {n: hashlib.sha256(runs[0][n]).hexdigest() for n in names}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case,mask_name", PARAMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_taps_are_bit_identical_to_the_recorded_ones(ctx, golden, case, mask_name):
    want = golden["sha256"][key_of(case, mask_name)]
    got = tap_hashes(ctx, case, mask_name)
    assert sorted(got) == sorted(want)
    bad = [n for n in sorted(got) if got[n] != want[n]]
    assert not bad, f"{key_of(case, mask_name)}: taps differ from the recorded bits: {bad}"
