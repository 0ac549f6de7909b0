"""Test-side references for the fused dense-block kernels (csrc/dense_fused.hip), one kernel launch at a time.

Isolation
---------
A forward with taps on initial_conv and on conv1, conv2, conv3 and conv5 of every dense block returns the bf16 tensors every
fused kernel read and wrote (never conv4: a tap there makes the tail pair run layer by layer, api.hip chain_fits).  Each launch
is restated here in fp64 from the DEVICE's inputs, so no error compounds through the network:

    dense_conv1_stream   c1 = relu(conv(x))
    dense_pair_fused     c2 = relu(conv([x, c1])),  c3 = relu(conv([x, c1, c2_device]))
    dense_tail_fused     c4 = relu(conv([x, c1, c2, c3])),  out = alpha * conv([x, c1, c2, c3, c4]) + beta_x * x + beta_o * so

conv3 may take the stored c2: the pair kernel's layer-0 epilogue rounds relu(acc) to bf16 ONCE (`const bf16x4 o = {...}`) and
writes that same value into the LDS ring row and, through ob[n], to memory -- what conv3 reads on chip is what the tap returns.
x is the block's input (initial_conv or the previous block's conv5 tap); so, for dense3 only, the RRDB's input.  dense1/2:
alpha = 0.2, beta_x = 1; dense3: alpha = 0.04, beta_x = 0.2, beta_o = 1 (rrdb_in + 0.2 * (x + 0.2 * conv5)).

conv4 lives only in the tail kernel's LDS ring and the tail's skip can mask its conv, so two designed weight sets make the tail
checkable per element (probe_conv5_weights, probe_conv4_weights); with all-random weights the tail stays with the aggregate tests.

Contract (check / assert_bf16_close)
------------------------------------
The project's bf16 per-element contract (tests/test_kernels_gpu.py): every element within
    2^-7 |round_bf16(ref)| + 3e-5 scale  [+ extra]
of round_bf16(ref), and rel_l2 <= 1e-3.  scale is 1 for unit-scale tensors and the tensor's own rms where the designed sets scale
the weights up by a power of two (the absolute term stands for fp32 accumulation of cancelled sums, which scales with the data).
`extra` is the one derived allowance of the probe-conv4 set (see probe_conv4_reference).  A failure reports the count and the first
(image, row, column, channel) indices, each with its stream row, workgroup and ring row (stream_position).
"""
import hashlib

import numpy as np

from oracle import ops as O

G = 32                      # growth channels of the fused configuration
STEP, WINR = 8, 10          # rows per step and ring rows of the chain kernels (dense_fused.hip)
TAIL_ALPHA = {1: (0.2, 1.0, 0.0), 2: (0.2, 1.0, 0.0), 3: (0.04, 0.2, 1.0)}      # dense index -> alpha, beta_x, beta_o


def rbf(x):
    """Round to the nearest bf16, as fp64."""
    return O.round_bf16(np.asarray(x, np.float64))


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def spacing_bf16(x):
    """Distance from |x| (a bf16 value) to the next bf16 value above it: 2^(floor(log2 |x|) - 7); 0 at 0."""
    x = np.abs(np.asarray(x, np.float64))
    return np.where(x > 0, 2.0 ** (np.floor(np.log2(np.maximum(x, 1e-300))) - 7), 0.0)


def rms(x):
    return float(np.sqrt(np.mean(np.square(np.asarray(x, np.float64)))))


# ------------------------------------------------------------------------------------------------ where an element sits in the row stream
def stream_position(img, y, B, H, cap, ncu, packed=False, min_rows=24):
    """(stream row, workgroup, local row, step, ring row) of row y of image img, as chain_launch / conv1_stream_launch cut the
    stream: T = B (H + 1) rows (a separator after each image; packed: image pairs), ceil(T / min(ncu, ceil(T / min_rows))) rows
    per workgroup, the local stream starting one row before the range; layer 0 (conv2 / conv4) computes local row l in step
    l // 8 into ring row l % 10.  min_rows: 24 for the chain kernels, 16 for the streaming conv1."""
    if packed:
        img, B = img // 2, (B + 1) // 2
    T = B * (H + 1)
    n = ncu if not (0 < cap < ncu) else cap
    nwg = max(1, min(n, (T + min_rows - 1) // min_rows))
    rows = (T + nwg - 1) // nwg
    g = img * (H + 1) + y
    wg = g // rows
    l = g - (wg * rows - 1)
    return g, wg, l, l // STEP, l % WINR


# ------------------------------------------------------------------------------------------------ the contract
def check(got, ref, scale=1.0, extra=0.0, rel=1e-3):
    """-> dict(count, worst = max err / bound, first = up to 8 failing (image, row, column, channel), rel_l2, ok)."""
    refq = rbf(ref)
    got = np.asarray(got, np.float64)
    d = np.abs(got - refq)
    bound = 2.0 ** -7 * np.abs(refq) + 3e-5 * scale + extra
    bad = ~(d <= bound)                                             # a NaN fails
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(d == 0, 0.0, d / bound)
    ratio = np.where(np.isfinite(ratio), ratio, np.inf)
    r = rel_l2(got, refq) if np.isfinite(got).all() else float("inf")
    return dict(count=int(bad.sum()), worst=float(ratio.max()), first=[tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:8]],
                rel_l2=r, ok=not bad.any() and r <= rel)


def assert_bf16_close(got, ref, scale=1.0, extra=0.0, rel=1e-3, what="", locate=None):
    """got: the device's bf16 tensor; ref: the fp64 restatement BEFORE the storage rounding.  Returns the worst err / bound.
    locate(image, row) -> text, for the failure message (stream_position)."""
    r = check(got, ref, scale, extra, rel)
    if r["count"]:
        where = [(ix, locate(ix[0], ix[1])) if locate else ix for ix in r["first"]]
        raise AssertionError(f"{what}: {r['count']} elements outside the bf16 contract, worst err/bound {r['worst']:.3g}; first (image, row, column, channel): {where}")
    assert r["rel_l2"] <= rel, (what, r["rel_l2"])
    return r["worst"]


# ------------------------------------------------------------------------------------------------ the restatement, one launch each
def conv(x, kb, act=None):
    return O.conv2d(np.asarray(x, np.float64), kb[0], kb[1], act=act, dtype=np.float64)


def cat(*a):
    return np.concatenate([np.asarray(t, np.float64) for t in a], axis=-1)


def growth_ref(feats, w, name, k):
    """conv<k> (k = 1..4) of block `name` from the tensors it reads: relu(conv([x, c1, ..]))."""
    assert len(feats) == k
    return conv(cat(*feats), w[f"{name}_conv{k}"], act="relu")


def tail_ref(x, c1, c2, c3, c4, w, name, so=None):
    """The block's stored output from the tensors the tail reads (c4 as the ring holds it: bf16).  Without `so` the expression is
    oracle.models._dense_block's own, x + 0.2 * conv5; with it, the RRDB's so + 0.2 * (x + 0.2 * conv5)."""
    x = np.asarray(x, np.float64)
    out = x + conv(cat(x, c1, c2, c3, c4), w[f"{name}_conv5"]) * np.float64(0.2)
    return out if so is None else np.asarray(so, np.float64) + out * np.float64(0.2)


def tail_terms(x, c1, c2, c3, c4, w, name, so=None):
    """(|alpha * conv5 term|, |skips|) of tail_ref, for the median-dominance conditions of the designed sets."""
    alpha, bx, _ = TAIL_ALPHA[3 if so is not None else 1]
    cterm = alpha * conv(cat(x, c1, c2, c3, c4), w[f"{name}_conv5"])
    skip = bx * np.asarray(x, np.float64) + (0.0 if so is None else np.asarray(so, np.float64))
    return np.abs(cterm), np.abs(skip)


def dense_block_chain(x, w, name, q=rbf):
    """The launches chained over one block with storage rounding q after each growth conv: oracle.models._dense_block restated
    (tests/test_dense_ref_cpu.py asserts equality).  -> (unrounded block output, [x, c1, c2, c3, c4])."""
    feats = [np.asarray(x, np.float64)]
    for k in range(1, 5):
        feats.append(q(growth_ref(feats, w, name, k)))
    return tail_ref(*feats, w, name), feats


def probe_conv4_reference(x, c1, c2, c3, w, name, so=None):
    """probe-conv4 set: (ref, extra).  conv5 only copies alpha 2^k c4[y + dy, x + dx, j] (zero padded) onto the skips, so
    ref = tail_ref with c4 = round_bf16(c4_ref).  The device's c4 is the bf16 rounding of an fp32 sum instead of the fp64 one:
    round_bf16(c4_ref) or one of its two bf16 neighbours, at most spacing_bf16(round_bf16(c4_ref)) away (the larger of the two
    distances), which the same one-hot conv5 carries to the output: extra = alpha * conv(spacing, |w5|) -- derived, not measured."""
    c4 = rbf(growth_ref([x, c1, c2, c3], w, name, 4))
    ref = tail_ref(x, c1, c2, c3, c4, w, name, so)
    alpha = TAIL_ALPHA[3 if so is not None else 1][0]
    k5 = np.abs(np.asarray(w[f"{name}_conv5"][0], np.float64))[:, :, 64 + 3 * G:, :]
    extra = alpha * O.conv2d(spacing_bf16(c4), k5, None, dtype=np.float64)
    return ref, extra, c4


def tail_reference(weight_set, x, c1, c2, c3, w, name, so=None):
    """What the tail's stored output is checked against under a designed weight set, from the device's x, c1, c2, c3 (and so):
    dict(ref, extra, scale, c4, conv_median, skip_median).  scale = max(1, rms(ref)): the designed sets scale the weights up."""
    if weight_set == "probe_conv5":
        c4 = growth_ref([x, c1, c2, c3], w, name, 4)
        assert np.array_equal(c4, rbf(c4)), "one-hot conv4: c4 is exact in bf16"
        ref, extra = tail_ref(x, c1, c2, c3, c4, w, name, so), 0.0
    elif weight_set == "probe_conv4":
        ref, extra, c4 = probe_conv4_reference(x, c1, c2, c3, w, name, so)
    else:
        raise ValueError(weight_set)
    ct, sk = tail_terms(x, c1, c2, c3, c4, w, name, so)
    return dict(ref=ref, extra=extra, scale=max(1.0, rms(ref)), c4=c4, conv_median=float(np.median(ct)), skip_median=float(np.median(sk)))


# ------------------------------------------------------------------------------------------------ memo of references by their inputs' bits
_MEMO = {}


def memo(key, fn, *arrays):
    """fn(*arrays), computed once per (key, bit pattern of the arrays): fusion masks whose tapped inputs are bit-equal share it."""
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    k = (key, h.hexdigest())
    if k not in _MEMO:
        _MEMO[k] = fn(*arrays)
    return _MEMO[k]


# ------------------------------------------------------------------------------------------------ weight sets
def dense_names(layer_shapes):
    return sorted({n.rsplit("_conv", 1)[0] for n, _ in layer_shapes if "_dense" in n})


def dense_block_shapes(name):
    """[(layer, kernel shape)] of one dense block at G = 32 (what Model.layer_shapes() lists for it)."""
    return [(f"{name}_conv{k}", (3, 3, 64 + G * (k - 1), G)) for k in range(1, 5)] + [(f"{name}_conv5", (3, 3, 64 + 4 * G, 64))]


def random_weights(layer_shapes, seed):
    from sr355.weights import bf16_rounded, init_weights
    return bf16_rounded(init_weights(layer_shapes, seed=seed))


# powers of two of the designed sets, per dense index (dense3's alpha is 0.04 and it carries a second skip).  Chosen on the CPU reference so
# that the conv term exceeds the skips in the median (tests assert it; the ratios are in tests/test_dense_ref_cpu.py)
K5_PROBE_CONV5 = {1: 5, 2: 5, 3: 6}
K5_PROBE_CONV4 = {1: 4, 2: 4, 3: 6}
# probe-conv4: added to conv4's random bias.  About one standard deviation of conv4's pre-activation, which grows from block to block with the
# scaled-up block outputs (0.19, 1.0, 5.1 at 48 x 48): 80-90 % of c4 is then above the ReLU's zero and the median of the conv term means something
C4_BIAS_SHIFT = {1: 0.25, 2: 1.0, 3: 4.0}


def _dense_index(name):
    return int(name[-1])


def probe_conv5_weights(layer_shapes, seed):
    """conv4 one-hot, conv5 random times 2^k.  conv4's cout j picks one (tap, input channel) with weight +-2^e, e in {-1, 0, 1}, zero bias:
    c4 = relu(+-2^e in[shifted]) is exact in bf16, zero padding included, so the fp64 c4 IS the device's.  cout j < 9 takes tap j, cout j
    input chunk j % 5: all 9 taps and all 5 chunks are covered.  A negative weight only goes to a channel of x (chunks 0, 1): c1..c3 are
    ReLU outputs, whose negative is all zeros."""
    w = random_weights(layer_shapes, seed)
    rng = np.random.default_rng(seed + 77)
    for name in dense_names(layer_shapes):
        k4 = np.zeros((3, 3, 64 + 3 * G, G), np.float32)
        taps = np.concatenate([rng.permutation(9), rng.integers(0, 9, G - 9)])
        for j in range(G):
            chunk = j % 5
            ch = 32 * chunk + int(rng.integers(0, 32))
            sign = -1.0 if (chunk < 2 and rng.random() < 0.5) else 1.0
            k4[taps[j] // 3, taps[j] % 3, ch, j] = sign * 2.0 ** int(rng.integers(-1, 2))
        w[f"{name}_conv4"] = (k4, np.zeros(G, np.float32))
        s = np.float32(2.0 ** K5_PROBE_CONV5[_dense_index(name)])
        k5, b5 = w[f"{name}_conv5"]
        w[f"{name}_conv5"] = (k5 * s, b5 * s)
    return w


def probe_conv4_weights(layer_shapes, seed):
    """conv4 random; conv5 zero except on the c4 slice of its input, where cout j < 32 takes the centre tap of c4 channel j and cout
    32 + j a seeded off-centre tap of channel j (all 8 used), weight 2^k, zero bias: out = skips + alpha 2^k c4[y + dy, x + dx, j].
    conv4's kernel is the random one; its random bias is shifted up by C4_BIAS_SHIFT, because half of an unshifted c4 is ReLU zeros and the
    median of the conv term would be zero whatever k is."""
    w = random_weights(layer_shapes, seed)
    rng = np.random.default_rng(seed + 78)
    off = [t for t in range(9) if t != 4]
    for name in dense_names(layer_shapes):
        k4, b4 = w[f"{name}_conv4"]
        w[f"{name}_conv4"] = (k4, (b4 + np.float32(C4_BIAS_SHIFT[_dense_index(name)])).astype(np.float32))
        k5 = np.zeros((3, 3, 64 + 4 * G, 64), np.float32)
        s = np.float32(2.0 ** K5_PROBE_CONV4[_dense_index(name)])
        taps = np.concatenate([rng.permutation(off), rng.choice(off, G - 8)])
        for j in range(G):
            k5[1, 1, 64 + 3 * G + j, j] = s
            k5[taps[j] // 3, taps[j] % 3, 64 + 3 * G + j, G + j] = s
        w[f"{name}_conv5"] = (k5, np.zeros(64, np.float32))
    return w


WEIGHT_SETS = {"random": random_weights, "probe_conv5": probe_conv5_weights, "probe_conv4": probe_conv4_weights}


def exact_integer_weights(layer_shapes, density, seed):
    """test_fused_tail_exact_integers' regime with every layer seeded by its own name: dense-block kernels hold small integers (-2..2) at
    `density`, biases -1..1; initial_conv is a centre tap of -1..1 with biases 0..2; everything else is small noise.  On inputs of -1, 0, 1
    every partial sum of the first block's growth convs is a small integer, exact in bf16 storage below 2^8 and in fp32 always."""
    import zlib
    w = {}
    for name, shape in layer_shapes:
        rng = np.random.default_rng([seed, zlib.crc32(name.encode())])
        k = np.zeros(shape, np.float32)
        if "dense" in name:
            nz = rng.random(shape) < density
            k[nz] = rng.integers(-2, 3, size=int(nz.sum()))
            b = rng.integers(-1, 2, size=shape[-1]).astype(np.float32)
        elif name == "initial_conv":
            k[1, 1, :, :] = rng.integers(-1, 2, size=shape[2:])
            b = rng.integers(0, 3, size=shape[-1]).astype(np.float32)
        else:
            k = (rng.standard_normal(shape) * 0.01).astype(np.float32)
            b = np.zeros(shape[-1], np.float32)
        w[name] = (k, b)
    return w


EXACT_DENSITY, EXACT_SEED = 0.06, 7          # the largest density of 0.02, 0.03, .. at which conv1 and conv2 of the first block stay below 2^8 on (7, 11, 24, 3)


def exact_integer_case():
    """-> (x [7, 11, 24, 3] of -1, 0, 1; the fp64 integers x0, c1, c2, c3 of rrdb_0_dense1 under exact_integer_weights(.., EXACT_DENSITY, EXACT_SEED))."""
    shapes = [("initial_conv", (3, 3, 3, 64))] + dense_block_shapes("rrdb_0_dense1")
    w = exact_integer_weights(shapes, EXACT_DENSITY, EXACT_SEED)
    x = np.random.default_rng(EXACT_SEED).integers(-1, 2, size=(7, 11, 24, 3)).astype(np.float32)
    feats = [conv(x, w["initial_conv"])]
    for k in (1, 2, 3):
        feats.append(growth_ref(feats, w, "rrdb_0_dense1", k))
    return x, feats
