"""attn_bf16_kernel (csrc/attention.hip) stores the same BITS as before its unguarded groups got a loop of their own and its key fetch
lost the per-tile address arithmetic: the loads read the same bytes and every MFMA, exp and convert runs in the same order on the same
values, so equality is the criterion and there is no tolerance.

The cases (tests/attention_fastpath_cases.py) walk every shape of the key-group loop and leave and re-enter the loop of unguarded groups;
tests/test_attention_fastpath_cpu.py shows without a device which path every wave and group takes, and each test here asserts it again
before it looks at the output.  The recorded bits (tests/golden/attention_fastpath_bits.json, written on the GPU by
tests/golden/make_attention_fastpath_bits.py on the commit before the change) are a SHA-256 of the stored bf16 output per case and the
raw bits where N <= 256.  One case is also held to the fp64 softmax under attention_ref.bound, so the fixture is not the only judge."""
import base64
import json
import os

import numpy as np
import pytest

import attention_fastpath_cases as F
import attention_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_fastpath_bits.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", F.names_smallest_first())
def test_output_bits_are_the_recorded_ones(ctx, golden, name):
    c = F.cases()[name]
    hit = F.labels_hit(name)
    assert "ambiguous" not in hit and c["want"] <= hit, (name, sorted(hit))
    if c["runs"]:
        assert F.has_runs_around_a_slow_group(name), name
    got = R.run_core(ctx, c["k"], c["q"], c["v"], "bf16")
    assert got.shape == (c["k"].shape[0], c["n"], 32)
    bits = F.stored_bits(got)
    if name in golden["bits"]:
        want = np.frombuffer(base64.b64decode(golden["bits"][name]), "<i2").reshape(bits.shape)
        bad = np.argwhere(bits != want)
        assert bad.size == 0, (name, len(bad), bad[:8].tolist())
    assert F.sha256_of(bits) == golden["sha256"][name], name


def test_n640_is_within_the_fp64_bound(ctx):
    c = F.cases()[F.BOUND_CASE]
    k, q, v, base = R.core_inputs(c["k"], c["q"], c["v"], "bf16")
    ref, A = R.core_fp64(k, q, v, base)
    bnd = R.bound(ref, A, "bf16", R.score_scale(k, q), c["n"])
    got = R.run_core(ctx, c["k"], c["q"], c["v"], "bf16")
    ratio = R.worst_ratio(got, ref, bnd)
    print(f"{F.BOUND_CASE}: worst err/bound = {ratio:.3f}")
    assert ratio <= 1.0, (ratio, np.argwhere(~(np.abs(got - ref) <= bnd))[:8].tolist())
