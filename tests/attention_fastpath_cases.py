"""Cases shared by tests/test_attention_fastpath_{cpu,gpu}.py and tests/golden/make_attention_fastpath_bits.py: inputs of the bf16
SelfAttention core (csrc/attention.hip, attn_bf16_kernel) that walk every shape its key-group loop can take, and that leave and re-enter
the loop of unguarded groups.  A case is dict(k, q, v [B,N,*] exactly representable in bf16, want = labels attention_ref.bf16_paths must
report for it, runs = whether an unguarded run of >= 2 groups must stand on both sides of a slow group).

Loop shapes (Gaussian inputs, score sd ~ 1, B = 2 images from one stream, so they differ):
    N = 1, 31, 33, 96   a single ragged group
    N = 128, 256        whole groups only: the loop of unguarded groups exits straight into the epilogue
    N = 160, 385        a tail (whole tiles / ragged) behind full groups
    N = 640             first group plus four unguarded groups
    N = 2304            the 48 x 48 layer
Leaving and re-entering (N = 1056: group 0, three unguarded groups, the planted group 4, three unguarded groups, a 32-key tail):
    planted_pass        one key 64 e_7 in group 4 and every query's component 7 zero: the group bound fails (|k| = 92 against a threshold
                        near 14) while the key scores exactly 0 for every query -- every wave runs the group guarded and it passes
    planted_redo        B = 3, the same key in tile 0, 2, 3 of group 4 and every query's component 7 equal to 1: the key scores 92.5, more
                        than 2^40 above the running maxima, and the guarded group redoes from that tile; the new maxima lift the threshold
                        far above the ordinary keys, so the groups behind run unguarded again
    zero_queries        N = 640, image 1 all-zero queries: threshold +inf
"""
import functools
import hashlib

import numpy as np
import torch

import attention_ref as R

GAUSS_N = (1, 31, 33, 96, 128, 160, 256, 385, 640, 2304)
N_PLANT = 1056
PLANT_GROUP = 4
RAW_BITS_MAX_N = 256
BOUND_CASE = "gauss_n640"


def _gauss(seed, N, B):
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(1.0 / np.sqrt(8.0))
    return dict(k=R.rbf(sigma * rng.standard_normal((B, N, 8))), q=R.rbf(sigma * rng.standard_normal((B, N, 8))),
                v=R.rbf(rng.standard_normal((B, N, 32))))


def _want_gauss(n):
    want = {"first"}
    if n >= 2 * R.KT:
        want.add("unguarded")
    if n > R.KT and n % R.KT:
        want.add("tail_ragged" if n % R.TILE else "tail_whole_tiles")
    return want


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in GAUSS_N:
        out["gauss_n%d" % n] = dict(_gauss(5000 + n, n, 2), want=_want_gauss(n), runs=False)
    c = _gauss(6001, N_PLANT, 2)
    c["q"][..., 7] = 0.0
    for b, sub in enumerate((1, 3)):
        c["k"][b, PLANT_GROUP * R.KT + sub * R.TILE + 5 + b] = 64.0 * np.eye(8)[7]
    out["planted_pass"] = dict(c, want={"first", "unguarded", "guarded_pass", "tail_whole_tiles"}, runs=True)
    c = _gauss(6002, N_PLANT, 3)
    c["q"][..., 7] = 1.0
    for b, sub in enumerate((0, 2, 3)):
        c["k"][b, PLANT_GROUP * R.KT + sub * R.TILE + 9 + b] = 64.0 * np.eye(8)[7]
    out["planted_redo"] = dict(c, want={"first", "unguarded", "redo@0", "redo@2", "redo@3", "tail_whole_tiles"}, runs=True)
    c = _gauss(6003, 640, 2)
    c["q"][1] = 0.0
    out["zero_queries"] = dict(c, want={"first", "unguarded"}, runs=False, zero_image=1)
    for c in out.values():
        c["n"] = c["k"].shape[1]
        for a in ("k", "q", "v"):
            c[a].setflags(write=False)
    return out


def names_smallest_first():
    cs = cases()
    return sorted(cs, key=lambda name: (cs[name]["n"], name))


@functools.lru_cache(maxsize=None)
def paths(name):
    """attention_ref.bf16_paths of a case, on the values the core receives."""
    c = cases()[name]
    kp, q, _, _ = R.core_inputs(c["k"], c["q"], c["v"], "bf16")
    return R.bf16_paths(kp, q, c["n"])


def labels_hit(name):
    return {lab for rec in paths(name) for lab in rec["labels"]}


def has_runs_around_a_slow_group(name):
    """Some wave runs >= 2 unguarded groups, then a guarded group, then >= 2 unguarded groups again."""
    for rec in paths(name):
        lab = ["u" if x == "unguarded" else ("s" if x == "guarded_pass" or x.startswith("redo@") else "-") for x in rec["labels"]]
        if "uusuu" in "".join(lab):
            return True
    return False


def stored_bits(out):
    """run_core's fp64 copy of the stored bf16 output -> the stored 16-bit patterns [B,N,32] (little-endian int16)."""
    t = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float64)).to(torch.bfloat16)
    assert (t.to(torch.float64).numpy() == out).all() or not np.isfinite(out).all()
    return np.ascontiguousarray(t.view(torch.int16).numpy()).astype("<i2")


def sha256_of(bits):
    return hashlib.sha256(bits.tobytes()).hexdigest()
