"""Test-side references for the SelfAttention core (csrc/attention.hip), driven alone through sr_self_attention.

Driving the core alone
----------------------
sr_self_attention computes f | g | h with one 1x1 conv 64 -> 48, runs the core on (k = f, q = g, v = h) and applies a
1x1 conv 32 -> 64 plus x.  With 0/1 selector weights and zero biases both convs are exact copies, so with

    x[..., 0:8] = keys    x[..., 8:16] = queries    x[..., 16:48] = values    x[..., 48:64] = 0

and wv routing 16 of the core's 32 output channels to output channels 48..63, y[..., 48:64] is bit for bit what the
core stored (product with 1.0, skip connection 0, exact store).  Two runs give all 32 channels (run_core).  On the
bf16 path the key projection is packed as bf16(log2(e) * wf) = 1.4453125, so the core receives
k' = round_bf16(1.4453125 * k) and works in the exp2 domain (core_inputs).  Every reference here takes the values the
core receives (k' or k, q, v), never x and the weights.

The per-element bound (bound())
-------------------------------
ref = sum_k p_k v_k / sum_k p_k with p_k = base^(s_k - max s), s_k = k_k . q, computed in fp64 (core_fp64), and
A = sum_k p_k |v_k| / sum_k p_k, the scale of what was summed (|ref| <= A; ref may be a cancelled sum).  If every
probability carries a relative error |e_k| <= eps, the quotient moves by sum_k p_k e_k (v_k - ref) / sum_k p_k, which is
at most eps * (A + |ref|): numerator and denominator together.  Every term below has that form; u = 2^-23 is one fp32
ulp, charged per operation so that the bound does not depend on how the matrix core rounds internally.

bf16 kernel, rounding points in the order the kernel documents them:
  1. score MFMA  k'.q - m1 - m2 - m3  (the running max rides in K-slots 8..10 as three bf16 pieces that carry all 24
     bits): 16 fp32 accumulation steps on partial sums no larger than T + |m|, T = max_k sum_i |k'_i q_i|.  Each update
     m_run += delta of the running max rounds to fp32 as well and shifts every later score against the accumulators
     that were rescaled by exp2(-delta): at most one such update per 32-key tile, ceil(N / 32) in all.  The caller
     passes smax >= T + |m| per query (score_scale(): T + max_k |s_k|).  Absolute score error (16 + ceil(N/32)) u smax,
     relative probability error ln 2 times that.
  2. the shifted score itself, s - delta or the MFMA result, rounded to fp32: u * |s - m|.  Only probabilities above
     2^-D of the largest matter, and a fast tile runs up to 2^GROW_OK = 2^40 above a stale maximum: D = 40, relative
     ln 2 * u * D.  (Keys further down carry weight < 2^-40 each; N of them stay below the fp64 reference's own
     resolution relative to the terms carried here and are not carried.)
  3. v_exp_f32: one ulp, u.
     Together eps_s = u * (1 + ln 2 * ((16 + ceil(N/32)) * smax + 40)).
  4. each probability rounded to bf16 before it enters BOTH sums (the row sums ride on the matrix core over the same
     fragment): relative 2^-8 at the bottom of a binade.  eps_p = 2^-8, i.e. 2^-8 (A + |ref|) <= 2^-7 A.  Where all
     probabilities are exactly representable (all-zero queries: every p = 1) this term is absent (p_exact=True).
  5. fp32 accumulation of N products in the numerator and N probabilities in the denominator, the per-tile rescale
     multiplies of both (alpha = exp2(-delta): one ulp of v_exp plus the multiply, per tile), the reciprocal and the final
     multiply: eps_acc = u * (N + N / 8 + 4).
  6. the output store, round-to-nearest bf16: half the bf16 spacing at the stored value, between 2^-9 |o| (top of a
     binade) and 2^-8 |o| (bottom); taken exactly, at |ref| + the sum of the terms above.
  bound = E + half_spacing_bf16(|ref| + E),  E = (eps_p + eps_s + eps_acc) (A + |ref|).

f32 kernel (exact fp32 MFMA, natural exp, per-tile rescale, no path split):
  1. the 8-term fp32 dot product: 8 u T <= 8 u smax absolute, the same relative on p (d e^x = e^x dx).
  2. the __expf argument: s - m rounded, then multiplied by a rounded log2(e): 2 u |s - m| in all, with |s - m| <= D = 32
     nats for every key that matters (e^-32 per key below that).
  3. v_exp_f32: u.   eps_s = u * (1 + 8 smax + 2 * 32).
  4. fp32 accumulation over N keys, rescales, reciprocal: eps_acc as above.
  5. the final multiply oacc * inv: half an ulp of the result, 2^-24 |ref|; the f32 store is exact.
  bound = (eps_s + eps_acc) (A + |ref|) + 2^-24 |ref|.

Nothing in the bound was fitted to kernel output.  Its yardstick is emulate_bf16(): a NumPy restatement of the bf16
kernel's rounding points (probabilities rounded to bf16 before both sums, output rounded to bf16) on fp64 arithmetic.
Worst err / bound of the emulation against core_fp64, per case family (tests/test_attention_core_cpu.py asserts <= 1
on every case):
    gauss1 0.39    gauss15 0.57    gather 0 (exact)    zero_queries 0.61    minus400 0.12    norm_table 0.34
(gauss15: near one-hot rows, where the store's half spacing is a third of the bound and rounding attains it; zero_queries:
the wave of zero queries, whose bound is little more than that half spacing.)

The path model (bf16_paths())
-----------------------------
A CPU model of the bf16 key loop's control flow written from the kernel's comments and constants: 256 queries per
workgroup, waves of 2 x 32 queries, out-of-range queries clamped to N - 1, 128-key groups of four 32-key tiles,
GROW_OK = 40, the 2^-10 margins on |q|max and on the threshold, group 0 and a partial last group always on the full
logic, the threshold refreshed only after a group that ran the full logic (so the running maxima it sees are stale
through unguarded and passing groups).
"""
import functools
import itertools

import numpy as np
import torch

LOG2E_BF16 = 1.4453125          # bf16(log2 e): what the bf16 key projection is multiplied with
GROW_OK = 40.0
KT = 128                        # keys per group
TILE = 32
WAVE_Q = 64                     # queries per wave (2 blocks of 32)
LABELS = ("first", "unguarded", "guarded_pass", "redo@0", "redo@1", "redo@2", "redo@3", "tail_ragged", "tail_whole_tiles")
U32 = 2.0 ** -23


def rbf(x):
    """Round to the nearest bf16 (ties to even), returned as fp64."""
    a = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return a.to(torch.bfloat16).to(torch.float32).numpy().astype(np.float64)


def core_inputs(k, q, v, dtype):
    """The values the core receives and the base of its exponential: bf16 -> (round_bf16(1.4453125 k), q, v, 2), f32 -> (k, q, v, e)."""
    k, q, v = (np.asarray(a, np.float64) for a in (k, q, v))
    if dtype == "bf16":
        return rbf(LOG2E_BF16 * k), q, v, 2.0
    return k, q, v, np.e


def core_fp64(k, q, v, base):
    """Materialised softmax in fp64.  k, q [B,N,8], v [B,N,32] -> (ref, A) [B,N,32]."""
    s = np.matmul(q, k.transpose(0, 2, 1))
    s -= s.max(axis=-1, keepdims=True)
    p = np.exp2(s) if base == 2.0 else np.exp(s)
    den = p.sum(axis=-1, keepdims=True)
    return np.matmul(p, v) / den, np.matmul(p, np.abs(v)) / den


def score_scale(k, q):
    """smax [B,N,1]: T + max_k |s_k| per query, T = max_k sum_i |k_i q_i| (see the module docstring)."""
    t = np.matmul(np.abs(q), np.abs(k).transpose(0, 2, 1)).max(axis=-1, keepdims=True)
    s = np.abs(np.matmul(q, k.transpose(0, 2, 1))).max(axis=-1, keepdims=True)
    return t + s


def half_spacing_bf16(x):
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-300))) - 8), 0.0)


def bound(ref, A, dtype, smax, n, p_exact=False):
    """Per-element error bound of the core against core_fp64; derivation in the module docstring."""
    scale = A + np.abs(ref)
    eps_acc = U32 * (n + n / 8.0 + 4)
    if dtype == "bf16":
        ntiles = -(-n // TILE)
        eps_s = U32 * (1 + np.log(2.0) * ((16 + ntiles) * smax + 40))
        e = ((0.0 if p_exact else 2.0 ** -8) + eps_s + eps_acc) * scale
        return e + half_spacing_bf16(np.abs(ref) + e)
    eps_s = U32 * (1 + 8 * smax + 2 * 32)
    return (eps_s + eps_acc) * scale + 2.0 ** -24 * np.abs(ref)


def worst_ratio(got, ref, bnd):
    """max err / bound over every element; inf where got is not finite or the bound is zero and missed."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bnd)
    r = np.where(np.isfinite(r), r, np.inf)
    return float(r.max())


def accepts(got, ref, bnd):
    """The comparison of the GPU test: every element within its bound (no norm, no element left out)."""
    return worst_ratio(got, ref, bnd) <= 1.0


def emulate_bf16(kp, q, v, m=None, drop_key=None, tile_weight=None, den_scale=None):
    """The bf16 kernel's rounding points on fp64 arithmetic: p = round_bf16(2^(s - m)) enters both sums, the quotient is
    rounded to bf16.  m [B,N,1] is the maximum the probabilities are taken against (default: the true row maximum; a stale
    one models a fast tile).  The remaining arguments inject the faults of the negative controls:
    drop_key (b, key): that key is masked;  tile_weight (b, q0, k0, w): probabilities of keys k0..k0+31 times w for
    queries q0..q0+31;  den_scale (b, q0, f): denominators of queries q0..q0+15 times f."""
    s = np.matmul(q, kp.transpose(0, 2, 1))
    if drop_key is not None:
        s[drop_key[0], :, drop_key[1]] = -np.inf
    if m is None:
        m = s.max(axis=-1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        p = rbf(np.exp2(s - m))
        if tile_weight is not None:
            b, q0, k0, w = tile_weight
            p[b, q0:q0 + 32, k0:k0 + 32] *= w
        den = p.sum(axis=-1, keepdims=True)
        if den_scale is not None:
            b, q0, f = den_scale
            den[b, q0:q0 + 16] *= f
        return rbf(np.matmul(p, v) / den)


# ------------------------------------------------------------------------------------------------ path model
def _thresh(m_min, qmaxv):
    lim = np.float32(GROW_OK) + np.float32(m_min)
    if not lim >= 0:
        return -1.0, "neg"
    if not qmaxv > 0:
        return np.inf, "inf"
    return float(lim) / qmaxv * 0.9990234375, "ordinary"


def _near(a, b):
    return abs(a - b) <= 0.05 * abs(b)


def bf16_paths(kp, q, N):
    """Control flow of the bf16 key loop.  kp, q [B,N,8] as the core receives them.  Returns a list of records
    dict(b, wave, labels=[one per key group], thresh=[kind of every threshold refresh, in order])."""
    B = kp.shape[0]
    ngroups = -(-N // KT)
    nwaves = -(-N // (4 * WAVE_Q)) * 4
    out = []
    for b in range(B):
        knorm = [float(np.sqrt((kp[b, g * KT:(g + 1) * KT] ** 2).sum(-1).max())) for g in range(ngroups)]
        for w in range(nwaves):
            idx = np.minimum(w * WAVE_Q + np.arange(WAVE_Q), N - 1)       # clamped, also for a wave wholly out of range
            qw = q[b, idx]
            s = qw @ kp[b].T                                               # [64, N]
            qmaxv = float(np.sqrt((qw ** 2).sum(-1).max())) * 1.0009765625
            labels, kinds = ["first"], []
            m = s[:, :min(KT, N)].max(axis=1)
            th, kind = _thresh(m.min(), qmaxv)
            kinds.append(kind)
            for g in range(1, ngroups):
                k0 = g * KT
                if k0 + KT > N:
                    labels.append("tail_ragged" if N % TILE else "tail_whole_tiles")
                    m = np.maximum(m, s[:, k0:].max(axis=1))
                    th, kind = _thresh(m.min(), qmaxv)
                    kinds.append(kind)
                    continue
                amb = kind == "ordinary" and _near(knorm[g], th)
                if knorm[g] <= th:
                    labels.append("ambiguous" if amb else "unguarded")
                    continue
                label = "guarded_pass"
                for sub in range(KT // TILE):
                    ex = float((s[:, k0 + sub * TILE:k0 + (sub + 1) * TILE] - m[:, None]).max())
                    amb = amb or _near(ex, GROW_OK)
                    if ex > GROW_OK:
                        label = "redo@%d" % sub
                        m = np.maximum(m, s[:, k0 + sub * TILE:k0 + KT].max(axis=1))
                        th, kind = _thresh(m.min(), qmaxv)
                        kinds.append(kind)
                        break
                labels.append("ambiguous" if amb else label)
            out.append(dict(b=b, wave=w, labels=labels, thresh=kinds))
    return out


def stale_max(kp, q, N):
    """[B,N,1] group 0's row maxima: what every later probability is taken against when all full groups after group 0 run unguarded
    without a rescale -- what the kernel does if its group bound wrongly holds (an image reading another image's key norms)."""
    s = np.matmul(q, kp.transpose(0, 2, 1))
    return s[:, :, :min(KT, N)].max(axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ selector construction
def grid_of(n):
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def selector_inputs(k, q, v, half):
    """x [B,H,W,64] fp32 and the eight weight / bias arrays that turn sr_self_attention into the bare core; `half` picks which 16
    of the core's 32 output channels reach y[..., 48:64]."""
    B, N = k.shape[:2]
    H, W = grid_of(N)
    x = np.zeros((B, N, 64), np.float32)
    x[..., 0:8], x[..., 8:16], x[..., 16:48] = k, q, v
    wf, wg, wh, wv = (np.zeros(s, np.float32) for s in ((1, 1, 64, 8), (1, 1, 64, 8), (1, 1, 64, 32), (1, 1, 32, 64)))
    for c in range(8):
        wf[0, 0, c, c] = 1.0
        wg[0, 0, 8 + c, c] = 1.0
    for c in range(32):
        wh[0, 0, 16 + c, c] = 1.0
    for c in range(16):
        wv[0, 0, 16 * half + c, 48 + c] = 1.0
    z = lambda n: np.zeros(n, np.float32)
    return x.reshape(B, H, W, 64), [wf, z(8), wg, z(8), wh, z(32), wv, z(64)]


def run_core(ctx, k, q, v, dtype):
    """The core's stored output [B,N,32] (fp64 copy) for inputs k, q, v (before the bf16 path's key pre-scale)."""
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    B, N = k.shape[:2]
    halves = []
    for half in (0, 1):
        x, ws = selector_inputs(k, q, v, half)
        y = ctx.self_attention(ctx.to_device(x, td), *ws).float().cpu().numpy()
        halves.append(y.reshape(B, N, 64)[..., 48:64])
    return np.concatenate(halves, axis=-1).astype(np.float64)


# ------------------------------------------------------------------------------------------------ the cases
GAUSS_N = (1, 31, 32, 33, 127, 128, 129, 160, 255, 256, 257, 384, 385, 650)
N_STEER = 650
GATHER_PAIRS = (("g0", "sub0"), ("sub1", "sub2"), ("sub3", "tail"), ("perm", "g0"))


@functools.lru_cache(maxsize=None)
def codes():
    """The 1120 ternary codes in {-1, 0, +1}^8 with exactly four non-zeros."""
    out = []
    for pos in itertools.combinations(range(8), 4):
        for sg in itertools.product((-1.0, 1.0), repeat=4):
            c = np.zeros(8)
            c[list(pos)] = sg
            out.append(c)
    return np.array(out)


def _gather_image(rng, choice, N):
    """keys [N,8] (distinct codes) and pi [N] for one image."""
    C = codes()
    last = (N // KT - 1) * KT if N >= 2 * KT else 0          # first key of the last full group
    if choice.startswith("sub") or choice == "tail":
        sub = KT // TILE if choice == "tail" else int(choice[3:])      # "tail": the targets sit in the ragged tile after the last full group
        # 16 targets: the codes on support {0,1,2,3}.  Every key before the target tile comes from the codes whose dot product with
        # each target is <= 2, so that no non-target score outgrows group 0's maximum (a dot-2 key) and the group passes its guard.
        tgt = np.flatnonzero((np.abs(C[:, :4]).sum(1) == 4))
        dots = C @ C[tgt].T
        avail = np.flatnonzero(dots.max(1) <= 2)
        rest = np.setdiff1d(np.arange(len(C)), np.concatenate([tgt, avail]))
        t0 = last + sub * TILE
        before = rng.permutation(avail)
        width = min(TILE, N - t0)
        slots = np.sort(rng.choice(width, min(16, width), replace=False))
        tile_ids = before[t0:t0 + width].copy()
        tile_ids[slots] = rng.permutation(tgt)[:len(slots)]
        after = rng.permutation(np.concatenate([before[t0 + width:], rest]))[:N - t0 - width]
        ids = np.concatenate([before[:t0], tile_ids, after])
        pi = t0 + slots[rng.integers(0, len(slots), N)]
        assert (C[ids[:KT]] @ C[tgt].T).max(0).min() == 2
    elif choice == "perm":
        # A random permutation, except that the first query of every wave and the last query (all that a wholly clamped wave holds)
        # target an anchor: the last key, in the ragged tile, with no dot-3 neighbour among the keys.  Its queries keep a running
        # maximum of at most a dot-2 score through every full group, which holds the wave's threshold well below the key norm
        # (guarded, no decision near its threshold) while the other queries' maxima grow tile after tile.
        a = rng.integers(len(C))
        pool = np.flatnonzero(C @ C[a] <= 2)
        ids = np.concatenate([rng.permutation(pool)[:N - 1], [a]])
        pi = rng.permutation(N)
        pi[::WAVE_Q] = N - 1
        pi[N - 1] = N - 1
    else:
        ids = rng.permutation(len(C))[:N]
        pi = rng.integers(0, min(KT, N), N)
    assert len(set(ids.tolist())) == N
    return C[ids], pi


def _gather_case(seed, choices, N):
    rng = np.random.default_rng(seed)
    ks, qs, vs, pis = [], [], [], []
    for ch in choices:
        k, pi = _gather_image(rng, ch, N)
        ks.append(k)
        qs.append(32.0 * k[pi])
        vs.append(rng.choice((-1.0, 1.0), (N, 32)) * (1.0 + rng.integers(0, 128, (N, 32)) / 128.0))    # bf16-exact, |v| in [1, 2)
        pis.append(pi)
    return dict(k=np.array(ks), q=np.array(qs), v=np.array(vs), pi=np.array(pis), choices=choices, family="gather")


def _gauss(seed, N, sd, dtype, B=2):
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(sd / np.sqrt(8.0))
    k, q, v = sigma * rng.standard_normal((B, N, 8)), sigma * rng.standard_normal((B, N, 8)), rng.standard_normal((B, N, 32))
    cast = rbf if dtype == "bf16" else (lambda a: a.astype(np.float32).astype(np.float64))
    return dict(k=cast(k), q=cast(q), v=cast(v))


@functools.lru_cache(maxsize=None)
def cases(dtype):
    """name -> dict(k, q, v [B,N,*] exactly representable in dtype, family, steered, ...).  Built once per dtype and shared,
    unchanged, by the CPU and the GPU module."""
    out = {}
    for i, ch in enumerate(GATHER_PAIRS):
        out["gather_%s_%s" % ch] = dict(_gather_case(100 + i, ch, N_STEER), steered=True)
    out["gather_n160"] = dict(_gather_case(110, ("g0", "perm"), 160), steered=True)
    for sd in (1, 15):
        for n in GAUSS_N:
            out["gauss%d_n%d" % (sd, n)] = dict(_gauss(1000 * sd + n, n, sd, dtype), family="gauss%d" % sd, steered=False)
    c = _gauss(7, N_STEER, 1, dtype)
    c["q"][1, 3 * WAVE_Q:4 * WAVE_Q] = 0.0                 # one whole wave of image 1
    out["zero_queries"] = dict(c, family="zero_queries", steered=True, zero=(1, 3 * WAVE_Q, 4 * WAVE_Q))
    c = _gauss(8, N_STEER, 1, dtype)
    c["k"][..., 0], c["q"][..., 0] = 20.0, -20.0           # every score about -400 (-577 in the exp2 domain) plus noise
    out["minus400"] = dict(c, family="minus400", steered=True)
    c = _gauss(9, N_STEER, 1, dtype)                       # one group of huge keys per image, a different group in each: the
    c["k"][0, 2 * KT:3 * KT] *= 64.0                       # per-image key-norm table decides which group must run guarded
    c["k"][1, 3 * KT:4 * KT] *= 64.0
    out["norm_table"] = dict(c, family="norm_table", steered=True)
    for c in out.values():
        c["n"] = c["k"].shape[1]
    return out


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(ref, bound) of a case: computed once, shared, never modified."""
    c = cases(dtype)[name]
    k, q, v, base = core_inputs(c["k"], c["q"], c["v"], dtype)
    ref, A = core_fp64(k, q, v, base)
    bnd = bound(ref, A, dtype, score_scale(k, q), c["n"])
    if "zero" in c:
        b, q0, q1 = c["zero"]
        bnd[b, q0:q1] = bound(ref, A, dtype, score_scale(k, q), c["n"], p_exact=True)[b, q0:q1]
    ref.setflags(write=False)
    bnd.setflags(write=False)
    return ref, bnd
