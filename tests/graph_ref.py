"""The model graphs of csrc/api.hip, one op at a time, restated in fp64 from the reference graphs as oracle/models.py states them
(srcnn_forward, edsr_forward, esrgan_g_forward, discriminator_forward, vgg19_features) -- never from Model.ops().

Isolation
---------
table(kind, cfg, dtype) lists a graph's ops in graph order.  A row holds the op's name as sr_model_op_info reports it, the rows whose
outputs it reads (`src`, concatenated along the channels; -1 is the model input), the conv's layers, K, act, alpha, the skip rows
with their betas, clip, d2s, and for stride2_pick the stride.  eval_row() computes ONE row in fp64 from given input tensors:

  * fed with the previous rows' own fp64 outputs (chain()) the table is the reference graph: tests/test_graph_ops_cpu.py asserts
    equality with oracle.models.*_forward(dtype=float64) to 1e-12;
  * fed with the tensors the DEVICE wrote (a tap on every op, sr_model_set_tap) it is what that one op had to compute, so no
    error compounds through the network and a wrong tap, channel offset, skip source or layout shows in the op that made it.

Ops the device adds to the reference graph are rows of their own: `convert` (the input padded to one 16-byte slice of channels),
`to_blocked` (bf16, growth % 8 == 0: a copy of initial_conv into the first concat buffer) or the repeated `initial_conv` (the same
layer run a second time into that buffer), `stride2_pick` (a stride-2 SAME conv is the stride-1 conv followed by a pick of every
second pixel: phase 1 on an even axis, 0 on an odd one, which is Keras SAME padding: total padding 1 -> none before the first
pixel, 2 -> one), `vgg_preprocess`, `maxpool`.  The discriminator's gap / dense / dense have no tap: disc_head() restates them
from the last tapped map, with a bound.

The projection's packing scale
------------------------------
In a bf16 model the f | g | h projection of a SelfAttention layer is packed with f pre-multiplied by log2(e) (Builder::self_attention,
as sr_self_attention packs it): the tapped f channels are log2(e) * f, and the attention kernel works in the exp2 domain.  That is
part of the device's contract, so the projection row APPLIES the scale (kscale, here fp32(log2 e); device=True also rounds the
scaled kernel to bf16, which is what the device packs) and the attention row UNDOES it (keys = f' / kscale, natural softmax).  In the
free-running chain the two cancel to 1e-16; against the device the attention row reads the device's own f'.

Designed weights
----------------
weights(kind, cfg): init_weights(seed) rounded to bf16, then GAINS: powers of two on kernel and bias of the layers with a skip (a
residual conv under x + 0.1 conv moves the sum by less than a bf16 ulp of x with He / Glorot weights -- scaled so that the conv
term is at least the skip term in the median) and of the clipped / tanh output layers (with BIAS_ADD: the EDSR output is centred in
(0, 1)), chosen on this restatement alone (tests/test_graph_ops_cpu.py asserts the conditions; tools are not needed to re-derive
them: tune() below is the search).  Rows at or after the first gained row carry `scaled`: their bf16 contract takes the tensor's rms
as its absolute scale (dense_ref.check), because the fp32 accumulation error of a cancelled sum grows with the data.

The fp32 bound (derived, not measured)
--------------------------------------
A conv output is a sum of n = K^2 Cin products plus the bias, scaled by alpha, plus the scaled skips.  Summed in fp32 in any order
(MFMA chunks, split accumulators) the error is at most (n - 1) u sum|terms| to first order, u = 2^-24; the bias add, the alpha
multiply, each skip's multiply and add, and the final rounding are 8 more roundings at most, each of a value no larger than
T = |alpha| (conv(|x|, |w|) + |b|) + sum_i |beta_i skip_i|.  So |got - ref| <= (n + 8) 2^-24 T per element (bound_T computes T in
fp64).  ReLU, LeakyReLU, clip and tanh are 1-Lipschitz: the bound carries through them (for LeakyReLU and ReLU T is taken before the
activation).  tanh and the discriminator's sigmoid get one extra allowance for the device function itself (TANH_ALLOW,
SIGMOID_ALLOW: twice the error measured on an MI355X).
"""
import numpy as np

from oracle import models as M
from oracle import ops as O

import attention_ref as AR

U = 2.0 ** -24
KSCALE = float(np.float32(1.4426950408889634))      # what Builder::self_attention multiplies the f projection with (bf16 models)

# twice the worst error of the device's tanhf / sigmoid (expf and a division) measured on these outputs
TANH_ALLOW = 2.0 * 7.6e-8
SIGMOID_ALLOW = 2.0 * 3.4e-8

# ------------------------------------------------------------------------------------------------ configurations (issue section 3)
SRCNN_SHAPES = [(3, 19, 37), (2, 5, 3), (1, 24, 16)]
EDSR_CFGS = [(2, 2, 64), (3, 1, 64), (4, 1, 64), (3, 1, 48), (2, 1, 96)]              # scale, blocks, filters
EDSR_SHAPES = [(3, 19, 37), (2, 5, 3), (1, 48, 32), (2, 24, 16)]
ESRGAN_ATT_CFGS = [(2, 8, 1, True), (4, 32, 1, True)]                                 # scale, growth, RRDBs, attention
ESRGAN_ATT_SHAPES = [(2, 13, 21), (3, 5, 3), (1, 24, 16)]
ESRGAN_NOATT_CFGS = [(2, 12, 1, False), (2, 6, 1, False)]
ESRGAN_NOATT_SHAPES = [(2, 13, 21), (3, 5, 3)]
DISC_SHAPES = [(4, 22, 35), (3, 21, 36), (2, 48, 48), (2, 5, 8)]
VGG19_SHAPES = [(2, 37, 53), (1, 33, 47)]


def cases():
    """[(kind, cfg, dtypes, shapes)]"""
    both = ("f32", "bf16")
    out = [("srcnn", (), both, SRCNN_SHAPES)]
    out += [("edsr", c, both, EDSR_SHAPES) for c in EDSR_CFGS]
    out += [("esrgan_g", c, both, ESRGAN_ATT_SHAPES) for c in ESRGAN_ATT_CFGS]
    out += [("esrgan_g", c, both, ESRGAN_NOATT_SHAPES) for c in ESRGAN_NOATT_CFGS]
    out += [("esrgan_d", (), ("f32",), DISC_SHAPES), ("vgg19_features", (), ("f32",), VGG19_SHAPES)]
    return out


RES_SCALING = 0.1
SEEDS = {"srcnn": 8100, "edsr": 8200, "esrgan_g": 8300, "esrgan_d": 8400, "vgg19_features": 8500}

# log2 of the gain on kernel and bias, per (kind, cfg) and layer; chosen by tune() on the fp64 chain over all of the configuration's shapes
GAINS = {
    ("edsr", (2, 2, 64)): {"conv2d_2": 5, "conv2d_4": 5, "conv2d_5": -1},
    ("edsr", (3, 1, 64)): {"conv2d_2": 5},
    ("edsr", (4, 1, 64)): {"conv2d_2": 4},
    ("edsr", (3, 1, 48)): {"conv2d_2": 5},
    ("edsr", (2, 1, 96)): {"conv2d_2": 4},
    ("esrgan_g", (2, 8, 1, True)): {"rrdb_0_dense1_conv5": 3, "rrdb_0_dense2_conv5": 3, "rrdb_0_dense3_conv5": 4, "self_attention_trunk_v": 2},
    ("esrgan_g", (4, 32, 1, True)): {"rrdb_0_dense1_conv5": 3, "rrdb_0_dense2_conv5": 3, "rrdb_0_dense3_conv5": 4, "self_attention_trunk_v": 1,
                                     "self_attention_upsample_0_v": 1},
    ("esrgan_g", (2, 12, 1, False)): {"rrdb_0_dense1_conv5": 3, "rrdb_0_dense2_conv5": 3, "rrdb_0_dense3_conv5": 4},
    ("esrgan_g", (2, 6, 1, False)): {"rrdb_0_dense1_conv5": 3, "rrdb_0_dense2_conv5": 3, "rrdb_0_dense3_conv5": 4},
}
# added to the bias of the clipped output layer after its gain (EDSR: centres the output in (0, 1))
BIAS_ADD = 0.5


def model_kwargs(kind, cfg, dtype):
    """Constructor arguments of sr355.Model for a configuration."""
    kw = dict(compute_dtype=dtype)
    if kind == "edsr":
        kw.update(scale_factor=cfg[0], num_blocks=cfg[1], num_filters=cfg[2], res_scaling=RES_SCALING)
    elif kind == "esrgan_g":
        kw.update(scale_factor=cfg[0], growth_channels=cfg[1], num_blocks=cfg[2], use_attention=cfg[3])
    return kw


def layer_shapes(kind, cfg):
    if kind == "srcnn":
        return M.srcnn_layers()
    if kind == "edsr":
        return M.edsr_layers(cfg[0], 3, cfg[1], cfg[2])
    if kind == "esrgan_g":
        L = M.esrgan_g_layers(cfg[0], cfg[1], cfg[2])
        return L if cfg[3] else [l for l in L if "self_attention" not in l[0]]
    if kind == "esrgan_d":
        return M.discriminator_layers()
    if kind == "vgg19_features":
        return M.vgg19_extractor_layers()
    raise ValueError(kind)


def base_weights(kind, cfg):
    from sr355.weights import bf16_rounded, init_weights
    scheme = "he_normal" if kind == "vgg19_features" else "glorot_uniform"
    return bf16_rounded(init_weights(layer_shapes(kind, cfg), scheme=scheme, seed=SEEDS[kind] + sum(int(c) for c in cfg)))


def apply_gains(w, gains, clip_layer=None):
    w = dict(w)
    for name, k in gains.items():
        s = np.float32(2.0 ** k)
        w[name] = (w[name][0] * s, w[name][1] * s)
    if clip_layer is not None:
        w[clip_layer] = (w[clip_layer][0], (w[clip_layer][1] + np.float32(BIAS_ADD)).astype(np.float32))
    return w


_W = {}


def weights(kind, cfg):
    """{layer: (kernel, bias)} of a configuration, gains applied; kernels are bf16 values (both data types read the same numbers)."""
    if (kind, cfg) not in _W:
        t = table(kind, cfg, "f32")
        clip = [r["parts"][0][0] for r in t if r.get("clip")]
        _W[kind, cfg] = apply_gains(base_weights(kind, cfg), GAINS.get((kind, cfg), {}), clip[0] if clip else None)
    return _W[kind, cfg]


def model_input(kind, shape):
    """bf16-valued input: [0, 1) for SRCNN and EDSR, [-1, 1) for the generator, the discriminator and the VGG19 extractor."""
    from sr355.weights import round_to_bf16
    rng = np.random.default_rng(9000 + 10000 * shape[0] + 100 * shape[1] + shape[2])
    lo = 0.0 if kind in ("srcnn", "edsr") else -1.0
    return round_to_bf16(rng.uniform(lo, 1.0, tuple(shape) + (3,)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the tables
def _conv(name, src, cin, cout, K=3, act=None, alpha=1.0, skips=(), clip=False, d2s=1, parts=None, out=False, stage=None):
    return dict(name=name, kind="conv", src=list(src), cin=cin, parts=parts or [(name, cout)], K=K, act=act, alpha=alpha, skips=list(skips),
                clip=clip, d2s=d2s, C=cout // (d2s * d2s), out=out, stage=stage)


def _plain(kind, src, C, **kw):
    return dict(name=kind, kind=kind, src=[src], C=C, skips=[], out=False, **kw)


def slice_channels(dtype):
    """Channels of one 16-byte slice: what `convert` and `vgg_preprocess` pad the image to."""
    return 4 if dtype == "f32" else 8


def srcnn_table(dtype):
    """SRCNN_model.py:48-53 / srcnn_forward."""
    return [_plain("convert", -1, slice_channels(dtype)),
            _conv("conv2d", [0], 3, 96, K=9, act="relu"),
            _conv("conv2d_1", [1], 96, 32, K=1, act="relu"),
            _conv("conv2d_2", [2], 32, 3, K=5, out=True)]


def edsr_table(scale, nb, F, dtype):
    """edsr_forward: head, nb x (conv relu, conv * res_scaling + block input), conv + head, the d2s convs, the clipped output conv."""
    names = iter(["conv2d"] + [f"conv2d_{i}" for i in range(1, 2 * nb + 5)])
    t = [_plain("convert", -1, slice_channels(dtype)), _conv(next(names), [0], 3, F)]
    head = cur = 1
    for _ in range(nb):
        t.append(_conv(next(names), [cur], F, F, act="relu"))
        t.append(_conv(next(names), [len(t) - 1], F, F, alpha=RES_SCALING, skips=[(cur, 1.0)]))
        cur = len(t) - 1
    t.append(_conv(next(names), [cur], F, F, skips=[(head, 1.0)]))
    for r in ([scale] if scale in (2, 3) else [2, 2]):
        t.append(_conv(next(names), [len(t) - 1], F, F * r * r, d2s=r))
    t.append(_conv(next(names), [len(t) - 1], F, 3, clip=True, out=True))
    return t


def _sa_rows(t, name, x):
    """ESRGAN_model.py:48-70 on row x: the f | g | h projection (one 48-cout 1x1 conv), the attention op, _v + x."""
    t.append(_conv(f"{name}_f", [x], 64, 48, K=1, parts=[(f"{name}_f", 8), (f"{name}_g", 8), (f"{name}_h", 32)], stage=name + "/fgh"))
    t[-1]["proj"] = True
    t.append(dict(name="attention", kind="attention", src=[len(t) - 1], C=32, skips=[], out=False, stage=name + "/o"))
    t.append(_conv(f"{name}_v", [len(t) - 1], 32, 64, K=1, skips=[(x, 1.0)], stage=name))
    return len(t) - 1


def esrgan_g_table(scale, G, nb, attention, dtype):
    """esrgan_g_forward.  The first concat buffer's copy of initial_conv is `to_blocked` where the device keeps the concat buffers row-blocked
    (bf16, G % 8 == 0) and the layer run again otherwise; dense3's conv5 stores rrdb_in + 0.2 (x + 0.2 conv5) at once."""
    t = [_plain("convert", -1, slice_channels(dtype)), _conv("initial_conv", [0], 3, 64, stage="initial_conv")]
    if dtype == "bf16" and G % 8 == 0:
        t.append(_plain("to_blocked", 1, 64))
    else:
        t.append(_conv("initial_conv", [0], 3, 64))
    x = len(t) - 1
    for b in range(nb):
        r_in = x
        for d in (1, 2, 3):
            n = f"rrdb_{b}_dense{d}"
            feats = [x]
            for k in range(1, 5):
                t.append(_conv(f"{n}_conv{k}", feats, 64 + (k - 1) * G, G, act="relu"))
                feats = feats + [len(t) - 1]
            if d < 3:
                t.append(_conv(f"{n}_conv5", feats, 64 + 4 * G, 64, alpha=0.2, skips=[(x, 1.0)]))
            else:
                t.append(_conv(f"{n}_conv5", feats, 64 + 4 * G, 64, alpha=0.04, skips=[(r_in, 1.0), (x, 0.2)], stage=f"rrdb_{b}"))
            x = len(t) - 1
    t.append(_conv("trunk_conv", [x], 64, 64, skips=[(1, 1.0)], stage="trunk_add"))
    x = len(t) - 1
    if attention:
        x = _sa_rows(t, "self_attention_trunk", x)
    for i in range(int(np.log2(scale))):
        t.append(_conv(f"upsample_{i}_conv", [x], 64, 256, act="lrelu", d2s=2, stage=f"upsample_{i}"))
        x = len(t) - 1
        if i == 0 and attention:
            x = _sa_rows(t, "self_attention_upsample_0", x)
    t.append(_conv("final_conv1", [x], 64, 64, act="relu", stage="final_conv1"))
    t.append(_conv("final_conv2", [len(t) - 1], 64, 3, act="tanh", out=True))
    return t


def disc_table(dtype):
    """discriminator_forward(training=False): six LeakyReLU convs, the stride-2 ones (second, fourth, sixth) as stride-1 conv + stride2_pick; GAP and the
    two dense layers have no activation-buffer output (disc_head)."""
    t = [_plain("convert", -1, slice_channels(dtype))]
    cin = 3
    for i, (f, st) in enumerate(zip([64, 64, 64, 128, 128, 256], M.DISC_STRIDES)):
        t.append(_conv(f"disc_conv{i + 1}", [len(t) - 1], cin, f, act="lrelu"))
        cin = f
        if st == 2:
            t.append(_plain("stride2_pick", len(t) - 1, f, stride=2))
    t.append(dict(name="gap", kind="gap", src=[len(t) - 1], C=0, skips=[], out=False))
    t.append(dict(name="dense", kind="dense", src=[len(t) - 1], C=0, skips=[], out=False, layer="disc_dense1", act="lrelu"))
    t.append(dict(name="dense", kind="dense", src=[len(t) - 1], C=0, skips=[], out=True, layer="disc_output", act="sigmoid"))
    return t


def vgg19_table(dtype):
    """vgg19_features after _preprocess_vgg_input: sixteen ReLU convs, a pool after blocks 1-4; block5_conv4 is the output."""
    t = [_plain("vgg_preprocess", -1, slice_channels(dtype))]
    cin = 3
    for blk, n, f in M.VGG19_CFG:
        for k in range(1, n + 1):
            t.append(_conv(f"block{blk}_conv{k}", [len(t) - 1], cin, f, act="relu", out=(blk, k) == (5, 4)))
            cin = f
        if blk < 5:
            t.append(_plain("maxpool", len(t) - 1, f))
    return t


def table(kind, cfg, dtype):
    t = {"srcnn": lambda: srcnn_table(dtype), "edsr": lambda: edsr_table(*cfg, dtype), "esrgan_g": lambda: esrgan_g_table(*cfg, dtype),
         "esrgan_d": lambda: disc_table(dtype), "vgg19_features": lambda: vgg19_table(dtype)}[kind]()
    gains = GAINS.get((kind, cfg), {})
    scaled = False
    for r in t:
        r["gain"] = sum(gains.get(n, 0) for n, _ in r["parts"][:1]) if r["kind"] == "conv" else 0
        scaled = scaled or r["gain"] != 0
        r["scaled"] = scaled
        r["tap_c"] = 0 if (r["out"] or r["kind"] in ("gap", "dense")) else r["C"]
    return t


def pick_phase(n):
    """Keras SAME, K = 3, stride 2 on n pixels: out = ceil(n / 2), total padding (out - 1) 2 + 3 - n = 1 (n even) or 2 (n odd), floor(total / 2) of
    it in front: the first window is centred on pixel 1 (n even) or 0 (n odd)."""
    return 1 if n % 2 == 0 else 0


def out_hw(t, H, W):
    """[(h, w)] of every row's output."""
    hw = []
    for r in t:
        h, w = (H, W) if r["src"][0] < 0 else hw[r["src"][0]]
        if r["kind"] == "conv":
            h, w = h * r["d2s"], w * r["d2s"]
        elif r["kind"] == "maxpool":
            h, w = h // 2, w // 2
        elif r["kind"] == "stride2_pick":
            h, w = -(-h // 2), -(-w // 2)
        hw.append((h, w))
    return hw


# ------------------------------------------------------------------------------------------------ one row in fp64
def f64(a):
    return np.asarray(a, np.float64)


def row_kernel(r, w, kscale=1.0, device=False):
    """(HWIO kernel, bias) of a conv row in fp64: its parts side by side; a projection's f part times kscale (device: the scaled kernel rounded to
    bf16 and the bias scaled in fp32, as sr_model_finalize packs them)."""
    ks, bs = [], []
    for i, (n, _) in enumerate(r["parts"]):
        k, b = w[n]
        if r.get("proj") and i == 0 and kscale != 1.0:
            if device:
                k, b = O.round_bf16(np.float32(kscale) * np.asarray(k, np.float32)), np.float32(kscale) * np.asarray(b, np.float32)
            else:
                k, b = kscale * f64(k), kscale * f64(b)
        ks.append(f64(k))
        bs.append(f64(b))
    return np.concatenate(ks, axis=-1), np.concatenate(bs)


def _conv_in(r, ins):
    return np.concatenate([f64(a) for a in ins], axis=-1)[..., :r["cin"]]


def eval_row(r, ins, skips, w, kscale=1.0, device=False):
    """The output of row r in fp64, before any storage rounding, from the outputs of r['src'] (`ins`) and of its skip rows (`skips`)."""
    kind = r["kind"]
    if kind == "conv":
        k, b = row_kernel(r, w, kscale, device)
        y = O.conv2d(_conv_in(r, ins), k, b, act=None if r["act"] == "tanh" else r["act"], dtype=np.float64)
        if r["alpha"] != 1.0:
            y = y * np.float64(np.float32(r["alpha"]) if device else r["alpha"])
        for (_, beta), s in zip(r["skips"], skips):
            y = y + (f64(s) if beta == 1.0 else np.float64(np.float32(beta) if device else beta) * f64(s))
        if r["act"] == "tanh":
            y = np.tanh(y)
        if r["clip"]:
            y = np.clip(y, 0.0, 1.0)
        return O.depth_to_space(y, r["d2s"]) if r["d2s"] > 1 else y
    x = f64(ins[0])
    if kind == "convert":
        return np.concatenate([x, np.zeros(x.shape[:3] + (r["C"] - x.shape[3],))], axis=-1)
    if kind == "vgg_preprocess":
        y = O.vgg19_preprocess(x)
        return np.concatenate([y, np.zeros(y.shape[:3] + (r["C"] - y.shape[3],))], axis=-1)
    if kind == "to_blocked":
        return x
    if kind == "maxpool":
        return O.maxpool2x2(x)
    if kind == "stride2_pick":
        return x[:, pick_phase(x.shape[1])::2, pick_phase(x.shape[2])::2]
    if kind == "attention":
        return attention_parts(x, kscale)[0]
    if kind == "gap":
        return x.mean(axis=(1, 2))
    if kind == "dense":
        return O.dense(x, *w[r["layer"]], act=r["act"], dtype=np.float64)
    raise ValueError(kind)


def attention_parts(qkv, kscale):
    """The attention op on a [B, H, W, 48] f' | g | h tensor: keys = f' / kscale, natural softmax (attention_ref.core_fp64).
    -> (o [B, H, W, 32], A [B, N, 32] the scale of what was summed, kq = (k', q) as the core receives them [B, N, 8])."""
    B, H, W, _ = qkv.shape
    x = f64(qkv).reshape(B, H * W, 48)
    kp, q, v = x[..., 0:8], x[..., 8:16], x[..., 16:48]
    ref, A = AR.core_fp64(kp / kscale, q, v, np.e)
    return ref.reshape(B, H, W, 32), A, (kp, q)


def attention_bound(qkv, dtype, kscale):
    """attention_ref.bound per element for the attention row on the device's own f' | g | h: (ref, bound), both [B, H, W, 32]."""
    B, H, W, _ = qkv.shape
    ref, A, (kp, q) = attention_parts(qkv, kscale)
    bnd = AR.bound(ref.reshape(B, H * W, 32), A, dtype, AR.score_scale(kp, q), H * W)
    return ref, bnd.reshape(B, H, W, 32)


def conv_terms(r, ins, skips, w, kscale=1.0):
    """(|alpha * conv + bias term|, |sum beta_i skip_i|) of a conv row before activation and d2s: the dominance condition's two sides."""
    k, b = row_kernel(r, w, kscale)
    c = r["alpha"] * O.conv2d(_conv_in(r, ins), k, b, dtype=np.float64)
    s = sum(beta * f64(t) for (_, beta), t in zip(r["skips"], skips))
    return np.abs(c), np.abs(s)


def bound_T(r, ins, skips, w):
    """(n, T) of the fp32 bound (n + 8) 2^-24 T of a conv row, T laid out as the row's output (module docstring)."""
    k, b = row_kernel(r, w)
    T = abs(r["alpha"]) * O.conv2d(np.abs(_conv_in(r, ins)), np.abs(k), np.abs(b), dtype=np.float64)
    for (_, beta), s in zip(r["skips"], skips):
        T = T + abs(beta) * np.abs(f64(s))
    if r["d2s"] > 1:
        T = O.depth_to_space(T, r["d2s"])
    return r["K"] * r["K"] * r["cin"], T


def disc_head(last, w):
    """GAP -> Dense(LeakyReLU) -> Dense(sigmoid) of the last tapped map [B, h, w, 256] in fp64 with a first-order bound on fp32 arithmetic in that
    order (as test_classifier_ops_gpu.head_reference): sequential sums of hw and of 257 terms, LeakyReLU 1-Lipschitz, |dp| <= |dz| / 4.
    -> (p [B, 1], bound [B, 1] without the sigmoid's own allowance)."""
    B = last.shape[0]
    x = f64(last).reshape(B, -1, last.shape[-1])
    hw = x.shape[1]
    (w1, b1), (w2, b2) = [(f64(k), f64(b)) for k, b in (w["disc_dense1"], w["disc_output"])]
    g = x.mean(axis=1)
    dg = hw * U * np.abs(x).mean(axis=1) + U * np.abs(g)
    a1 = g @ w1 + b1
    d1 = dg @ np.abs(w1) + (w1.shape[0] + 1) * U * (np.abs(g) @ np.abs(w1) + np.abs(b1))
    h = np.where(a1 > 0, a1, 0.2 * a1)
    z = h @ w2 + b2
    dz = d1 @ np.abs(w2) + (w2.shape[0] + 1) * U * (np.abs(h) @ np.abs(w2) + np.abs(b2))
    p = 1.0 / (1.0 + np.exp(-z))
    return p, dz / 4.0 + U * p


# ------------------------------------------------------------------------------------------------ the free-running chain
def chain(t, x, w, kscale=1.0):
    """Every row from the previous rows' own fp64 outputs -> [output per row]."""
    outs = []
    for r in t:
        get = lambda i: x if i < 0 else outs[i]
        outs.append(eval_row(r, [get(i) for i in r["src"]], [get(i) for i, _ in r["skips"]], w, kscale))
    return outs


def oracle_forward(kind, cfg, x, w, parts=None):
    """oracle.models' forward of the configuration in fp64."""
    if kind == "srcnn":
        return M.srcnn_forward(x, w, dtype=np.float64)
    if kind == "edsr":
        return M.edsr_forward(x, w, cfg[0], cfg[1], RES_SCALING, dtype=np.float64)
    if kind == "esrgan_g":
        return M.esrgan_g_forward(x, w, cfg[0], cfg[2], dtype=np.float64, attention=cfg[3], parts=parts)
    if kind == "esrgan_d":
        return M.discriminator_forward(x, w, dtype=np.float64)
    if kind == "vgg19_features":
        return M.vgg19_features(O.vgg19_preprocess(x), w, dtype=np.float64)
    raise ValueError(kind)


_CHAIN = {}


def chain_of(kind, cfg, shape, dtype="bf16"):
    """(table, outputs) of the free-running chain for a case, computed once (kscale as the data type's model applies it)."""
    key = (kind, cfg, tuple(shape), dtype)
    if key not in _CHAIN:
        t = table(kind, cfg, dtype)
        _CHAIN[key] = (t, chain(t, model_input(kind, shape), weights(kind, cfg), KSCALE if dtype == "bf16" else 1.0))
    return _CHAIN[key]


# ------------------------------------------------------------------------------------------------ the search that chose GAINS
def tune(kind, cfg, shapes, inside=0.7):
    """Row by row over all shapes at once: a skip row gets the smallest power of two (of either sign) that makes the median |alpha conv| at least the
    median |skips| at every shape; a clipped / tanh output row the largest one that leaves `inside` of the elements strictly inside.  -> {layer: log2 gain}."""
    t = table(kind, cfg, "bf16" if kind in ("srcnn", "edsr", "esrgan_g") else "f32")
    w = base_weights(kind, cfg)
    clip = [r["parts"][0][0] for r in t if r.get("clip")]
    w = apply_gains(w, {}, clip[0] if clip else None)
    xs = [model_input(kind, s) for s in shapes]
    outs = [[] for _ in xs]
    gains = {}
    for r in t:
        ins = [[x if i < 0 else o[i] for i in r["src"]] for x, o in zip(xs, outs)]
        sks = [[x if i < 0 else o[i] for i, _ in r["skips"]] for x, o in zip(xs, outs)]
        if r["kind"] == "conv" and r["skips"]:
            need = 0.0
            for a, s in zip(ins, sks):
                c, k = conv_terms(r, a, s, w, KSCALE)
                need = max(need, float(np.median(k) / np.median(c)))
            g = int(np.ceil(np.log2(need)))
            if g:
                gains[r["name"]] = g
                w = apply_gains(w, {r["name"]: g})
        elif r["kind"] == "conv" and (r["clip"] or r["act"] == "tanh"):
            name = r["name"]
            for g in range(0, -24, -1):
                wt = dict(w)
                s = np.float32(2.0 ** g)
                b0 = np.float32(BIAS_ADD) if r["clip"] else np.float32(0)
                wt[name] = (w[name][0] * s, (w[name][1] - b0) * s + b0)
                ys = [eval_row(r, a, sk, wt, KSCALE) for a, sk in zip(ins, sks)]
                share = min(float(np.mean((y > 0) & (y < 1))) if r["clip"] else float(np.mean(np.abs(y) < 0.9)) for y in ys)
                if share >= inside:
                    break
            if g:
                gains[name] = g
            w = wt
        for a, sk, o in zip(ins, sks, outs):
            o.append(eval_row(r, a, sk, w, KSCALE))
    return gains
