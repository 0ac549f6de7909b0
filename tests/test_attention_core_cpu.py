"""Proof, on the CPU, that tests/test_attention_core_gpu.py can fail: on the very inputs of that module (imported from
attention_ref.cases, not regenerated) the path model reaches every key-loop path, the bound admits the bf16 emulation on
every case, and the comparison rejects each of seven injected kernel faults."""
import numpy as np
import pytest

import attention_ref as R

BF = R.cases("bf16")


def _core(name):
    c = BF[name]
    return R.core_inputs(c["k"], c["q"], c["v"], "bf16")[:3]


@pytest.fixture(scope="module")
def paths():
    return {name: R.bf16_paths(*_core(name)[:2], c["n"]) for name, c in BF.items() if c["steered"]}


# ------------------------------------------------------------------------------------------------ path coverage
def test_steered_cases_cover_every_path(paths):
    seen = {lab for recs in paths.values() for r in recs for lab in r["labels"]}
    assert seen == set(R.LABELS), sorted(set(R.LABELS) ^ seen)          # every label, and no "ambiguous" group


@pytest.mark.parametrize("name,b,want", [
    ("gather_g0_sub0", 0, ["first"] + ["unguarded"] * 4 + ["tail_ragged"]),
    ("gather_g0_sub0", 1, ["first"] + ["guarded_pass"] * 3 + ["redo@0", "tail_ragged"]),
    ("gather_sub1_sub2", 0, ["first"] + ["guarded_pass"] * 3 + ["redo@1", "tail_ragged"]),
    ("gather_sub1_sub2", 1, ["first"] + ["guarded_pass"] * 3 + ["redo@2", "tail_ragged"]),
    ("gather_sub3_tail", 0, ["first"] + ["guarded_pass"] * 3 + ["redo@3", "tail_ragged"]),
    ("gather_sub3_tail", 1, ["first"] + ["guarded_pass"] * 4 + ["tail_ragged"]),
    ("gather_perm_g0", 1, ["first"] + ["unguarded"] * 4 + ["tail_ragged"]),
    ("gather_n160", 0, ["first", "tail_whole_tiles"]),
    ("minus400", 0, ["first"] + ["guarded_pass"] * 4 + ["tail_ragged"]),
    ("norm_table", 0, ["first", "unguarded", "redo@0", "unguarded", "unguarded", "tail_ragged"]),
    ("norm_table", 1, ["first", "unguarded", "unguarded", "redo@0", "unguarded", "tail_ragged"]),
])
def test_steering_gives_the_intended_path_in_every_wave(paths, name, b, want):
    recs = [r for r in paths[name] if r["b"] == b]
    assert len(recs) == (4 if BF[name]["n"] == 160 else 12)             # N = 650: three workgroups of four waves; 160: one
    for r in recs:
        assert r["labels"] == want, (r["wave"], r["labels"])


def test_random_permutation_grows_the_maximum_in_almost_every_group(paths):
    recs = [r for r in paths["gather_perm_g0"] if r["b"] == 0]
    redo = sum(lab.startswith("redo@") for r in recs for lab in r["labels"])
    assert redo >= 40, redo                                             # of 48 full groups after the first (12 waves x 4)


def test_both_special_threshold_branches_are_taken(paths):
    z = BF["zero_queries"]["zero"]
    for r in paths["zero_queries"]:
        zero_wave = r["b"] == z[0] and r["wave"] == z[1] // R.WAVE_Q
        assert (set(r["thresh"]) == {"inf"}) == zero_wave, r
        if zero_wave:
            assert r["labels"][1:-1] == ["unguarded"] * 4
    kp, q, _ = _core("minus400")
    assert (np.matmul(q, kp.transpose(0, 2, 1))[:, :, :R.KT].max(-1) < -R.GROW_OK).all()      # running maxima below -40
    assert all(set(r["thresh"]) == {"neg"} for r in paths["minus400"])


def test_gaussian_families_reach_the_fast_paths_too():
    seen = set()
    for name, c in BF.items():
        if not c["steered"]:
            seen |= {lab for r in R.bf16_paths(*_core(name)[:2], c["n"]) for lab in r["labels"]}
    assert {"first", "unguarded", "guarded_pass", "tail_ragged", "tail_whole_tiles"} <= seen


def test_path_model_clamps_queries_and_counts_waves():
    c = BF["gauss1_n257"]
    recs = R.bf16_paths(*_core("gauss1_n257")[:2], 257)
    assert len(recs) == 2 * 8                                           # two workgroups of four waves per image
    last = [r for r in recs if r["b"] == 0 and r["wave"] >= 5]          # waves wholly made of the clamped query 256
    assert len(last) == 3 and all(r["labels"] == last[0]["labels"] and r["thresh"] == last[0]["thresh"] for r in last)
    assert c["n"] == 257


# ------------------------------------------------------------------------------------------------ the bound admits the emulation
@pytest.mark.parametrize("name", sorted(BF))
def test_bound_admits_the_emulation(name):
    ref, bnd = R.reference(name, "bf16")
    em = R.emulate_bf16(*_core(name))
    ratio = R.worst_ratio(em, ref, bnd)
    print(f"{name}: emulation worst err/bound = {ratio:.3f}")
    assert ratio <= 1.0, ratio
    c = BF[name]
    if c["family"] == "gather":
        want = np.stack([c["v"][b][c["pi"][b]] for b in range(c["v"].shape[0])])
        assert np.array_equal(em, want)


def test_gather_codes_are_as_the_cases_assume():
    C = R.codes()
    assert C.shape == (1120, 8)
    g = C @ C.T
    assert (g[~np.eye(1120, dtype=bool)] <= 3).all() and (np.diag(g) == 4).all()
    assert np.array_equal(R.rbf(R.LOG2E_BF16 * C), R.LOG2E_BF16 * C)     # the codes survive the log2(e) pre-scale exactly
    for dtype in ("bf16", "f32"):
        for name, c in R.cases(dtype).items():
            for a in (c["k"], c["q"], c["v"]):                           # every input is exact in the dtype it is uploaded in
                assert np.array_equal(a, R.rbf(a) if dtype == "bf16" else a.astype(np.float32).astype(np.float64)), name
            assert not np.array_equal(c["k"][0], c["k"][1])              # the two images differ


# ------------------------------------------------------------------------------------------------ negative controls
def _argmax_key(name, b, lo, hi):
    """(query, key): the key in [lo, hi) that carries the largest probability of any query of image b, ties to the lowest query."""
    kp, q, _ = _core(name)
    s = q[b] @ kp[b].T
    s = s - s.max(axis=1, keepdims=True)
    qi, ki = np.unravel_index(np.argmax(s[:, lo:hi]), s[:, lo:hi].shape)
    return int(qi), int(ki) + lo


def _faulted(fault):
    """(case name, output of the emulation with the fault injected)."""
    if fault == "last_key_dropped":                                      # off-by-one in the ragged mask, one-key tail
        name = "gauss1_n33"
        return name, R.emulate_bf16(*_core(name), drop_key=(0, 32))
    if fault == "interior_key_dropped":                                  # a key of a fast group
        name = "gauss15_n650"
        _, key = _argmax_key(name, 1, 2 * R.KT, 3 * R.KT)
        return name, R.emulate_bf16(*_core(name), drop_key=(1, key))
    if fault == "v_rows_swapped":                                        # two adjacent V rows inside one 32-key tile
        name = "gauss15_n650"
        kp, q, v = _core(name)
        _, key = _argmax_key(name, 0, 3 * R.KT, 4 * R.KT)
        a = key if key % R.TILE < R.TILE - 1 else key - 1
        v = v.copy()
        v[0, [a, a + 1]] = v[0, [a + 1, a]]
        return name, R.emulate_bf16(kp, q, v)
    if fault == "tile_double_weighted":                                  # a skipped rescale: one tile counts twice for one 32-query block
        name = "gauss15_n650"
        return name, R.emulate_bf16(*_core(name), tile_weight=(1, 320, 2 * R.KT + 64, 2.0))
    if fault == "denominator_16_31":                                     # the lane + 16 rescale: second 16 denominators of one block
        name = "gauss15_n650"
        return name, R.emulate_bf16(*_core(name), den_scale=(0, 96 + 16, 1.0 + 2.0 ** -6))
    if fault == "neighbours_output":
        name = "gauss1_n257"
        em = R.emulate_bf16(*_core(name))
        em[1, 200] = em[1, 201]
        return name, em
    if fault == "other_images_key_norms":                                # an unguarded group > 2^40 above the running max, no rescale
        name = "norm_table"
        kp, q, v = _core(name)
        return name, R.emulate_bf16(kp, q, v, m=R.stale_max(kp, q, BF[name]["n"]))
    raise KeyError(fault)


FAULTS = ["last_key_dropped", "interior_key_dropped", "v_rows_swapped", "tile_double_weighted", "denominator_16_31",
          "neighbours_output", "other_images_key_norms"]


@pytest.mark.parametrize("fault", FAULTS)
def test_comparison_rejects_fault(fault):
    name, bad = _faulted(fault)
    ref, bnd = R.reference(name, "bf16")
    clean = R.emulate_bf16(*_core(name))
    assert R.accepts(clean, ref, bnd)
    ratio = R.worst_ratio(bad, ref, bnd)
    print(f"{fault} on {name}: worst err/bound = {ratio:.2f}")
    assert not R.accepts(bad, ref, bnd), ratio
    assert ratio > 1.5, ratio                                            # rejected with room, not by a rounding draw


def test_stale_maximum_within_grow_ok_is_harmless():
    """The counterpart of the last control: probabilities taken against a maximum that is stale by less than 2^GROW_OK -- what the
    fast tiles do by design -- stay inside the bound."""
    name = "gauss15_n650"
    kp, q, v = _core(name)
    s = np.matmul(q, kp.transpose(0, 2, 1))
    m = np.maximum(R.stale_max(kp, q, 650), s.max(-1, keepdims=True) - R.GROW_OK)
    ref, bnd = R.reference(name, "bf16")
    assert R.accepts(R.emulate_bf16(kp, q, v, m=m), ref, bnd)
