"""Every op of the model graphs (csrc/api.hip build_srcnn, build_edsr, build_esrgan, build_discriminator, build_vgg19_features as sr_forward runs
them) per element, each from the DEVICE's own inputs: one forward per (model, data type, shape) with a tap on every op that has an activation
output (NaN-filled tap buffers), then every op recomputed in fp64 by tests/graph_ref.py from the tapped tensors it read.

  structure   Model.ops() names, channels and output sizes equal graph_ref.table() (written from oracle/models.py, not from the device);
  bf16        dense_ref.check: 2^-7 |round_bf16(ref)| + 3e-5 scale per element and rel-L2 <= 1e-3; scale = max(1, rms(ref)) at and after the first
              layer with a gain (graph_ref.GAINS), 1 before;
  fp32        the derived bound (n + 8) 2^-24 T (graph_ref module docstring), + TANH_ALLOW on the tanh output, + SIGMOID_ALLOW on the discriminator's;
  copies      convert (padding channels exactly zero), to_blocked, maxpool and stride2_pick bit for bit -- the pick against ref[:, p_h::2, p_w::2]
              with the Keras SAME phases (graph_ref.pick_phase);
  vgg_preprocess  2^-14 absolute (tests/test_classifier_ops_gpu.py's contract); attention: attention_ref.bound per element;
  discriminator head  GAP, Dense(LeakyReLU), Dense(sigmoid) have no tap: the model output from the last tapped map (graph_ref.disc_head).

A failure names the op, the count and the first (image, row, column, channel) indices; every op prints its worst err / bound as a RATIO line.
No op is skipped: all ops of a case are compared and the failures reported together.

Taps change only what the docs say: an untapped forward on the same model gives the same output bit for bit -- fp32 under the default mask (SRCNN: with
the two head convs as two kernels in both, a tap on conv2d being documented to split them), bf16 under FUSED_ALL without FUSED_RGB_TAIL, FUSED_ATTN_PROJ
and FUSED_SRCNN_1X1, the mask under which the same kernels run in both.

EDSR bf16, 64 filters: at whole 24 x 16 tiles the body convs ran on conv_stream, at ragged shapes on conv_rows (a tap does not take the persistent
kernel out of play: asserted on the tapped and on the untapped forward).

Growth widths 12 and 6 (concat buffers unblocked; growth slices at channel offsets 64 + k G): at G = 12 every offset is a multiple of 4 channels, the
epilogues' 4-channel vector stores are 8-byte (bf16) / 16-byte (fp32) aligned; at G = 6 conv_launch finds out_coff % 4 != 0 (70, 82) or Cout % 4 != 0 and
routes the conv to the per-element scalar epilogue.  Both are computed, and tested here like every other width.

Measured on an MI355X, worst RATIO per model and the mutants each test catches: DESIGN.md 4.1."""
import numpy as np
import pytest
import torch

import dense_ref as D
import graph_ref as G
from sr355 import Model
from tap_util import forward_tapped, host

pytestmark = pytest.mark.gpu

CASES = [(kind, cfg, dt, shape) for kind, cfg, dts, shapes in G.cases() for dt in dts for shape in shapes]


def case_id(k, cfg, dt, s):
    return f"{k}{'-' + 'x'.join(str(int(c)) for c in cfg) if cfg else ''}-{dt}-{'x'.join(map(str, s))}"


IDS = [case_id(*c) for c in CASES]


@pytest.fixture(autouse=True)
def restore_fused(ctx):
    yield
    ctx.set_fused(ctx.FUSED_ALL, 0)


_MODELS, _RUNS = {}, {}


def model_of(ctx, kind, cfg, dtype):
    key = (kind, cfg, dtype)
    if key not in _MODELS:
        m = Model(kind, ctx=ctx, **G.model_kwargs(kind, cfg, dtype))
        assert m.layer_shapes() == G.layer_shapes(kind, cfg)
        m.set_weights(G.weights(kind, cfg))
        _MODELS[key] = m
    return _MODELS[key]


def same_kernel_mask(ctx):
    return ctx.FUSED_ALL & ~(ctx.FUSED_RGB_TAIL | ctx.FUSED_ATTN_PROJ | ctx.FUSED_SRCNN_1X1)


def profiled(ctx, fn):
    ctx.profile_begin()
    try:
        y = fn()
        torch.cuda.synchronize()
    finally:
        ks = {r["kernel"]: r["launches"] for r in ctx.profile_end()}
    return y, ks


def run(ctx, kind, cfg, dtype, shape):
    """The tapped forward (default mask) and the untapped ones of a case, once: dict(t, ops, x, y, taps {row: fp32 array}, kernels, untapped_equal,
    untapped_kernels)."""
    key = (kind, cfg, dtype, shape)
    if key in _RUNS:
        return _RUNS[key]
    m = model_of(ctx, kind, cfg, dtype)
    t = G.table(kind, cfg, dtype)
    x = G.model_input(kind, shape)
    xd = ctx.to_device(x, torch.float32 if dtype == "f32" else torch.bfloat16)
    ops = m.ops()
    idx = [i for i, o in enumerate(ops) if o[1] > 0]
    ctx.set_fused(ctx.FUSED_ALL, 0)
    (y, taps), kernels = profiled(ctx, lambda: forward_tapped(m, xd, idx))
    if dtype == "f32" and kind != "srcnn":
        y2, kernels2 = profiled(ctx, lambda: m.forward(xd))
        same = torch.equal(y2, y)
    else:
        ctx.set_fused(same_kernel_mask(ctx), 0)
        ya, _ = forward_tapped(m, xd, idx)
        y2, kernels2 = profiled(ctx, lambda: m.forward(xd))
        same = torch.equal(y2, ya)
        if dtype == "f32":
            same = same and torch.equal(ya, y)                  # fp32 SRCNN: the tapped forward is that two-kernel path under any mask
        ctx.set_fused(ctx.FUSED_ALL, 0)
    _RUNS[key] = dict(t=t, ops=ops, x=x, y=host(y), taps={i: host(v) for i, v in taps.items()}, kernels=kernels, untapped_equal=same,
                      untapped_kernels=kernels2)
    return _RUNS[key]


@pytest.mark.parametrize("kind,cfg,dtype,shape", CASES, ids=IDS)
def test_structure_is_the_reference_graph(ctx, kind, cfg, dtype, shape):
    r = run(ctx, kind, cfg, dtype, shape)
    t, ops = r["t"], r["ops"]
    assert [o[0] for o in ops] == [row["name"] for row in t]
    assert [o[1] for o in ops] == [row["tap_c"] for row in t]
    hw = G.out_hw(t, shape[1], shape[2])
    for i, (o, row) in enumerate(zip(ops, t)):
        if row["tap_c"]:
            assert Model._op_hw(o, shape[1], shape[2]) == hw[i], (i, row["name"])
            assert r["taps"][i].shape == (shape[0],) + hw[i] + (row["tap_c"],)
    assert sorted(r["taps"]) == [i for i, row in enumerate(t) if row["tap_c"]]


def ratio_of(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q = np.where(np.isfinite(q), q, np.inf)
    return float(q.max()), ~(err <= bound)


def first_bad(bad):
    return [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:8]]


def compare_row(r, i, kind, cfg, dtype):
    """-> (worst err / bound, failure text or None) of row i against its fp64 restatement from the device's inputs."""
    t, w = r["t"], G.weights(kind, cfg)
    row = t[i]
    ks = G.KSCALE if dtype == "bf16" else 1.0
    dev = lambda j: r["x"] if j < 0 else r["taps"][j]
    got = (r["y"] if row["out"] else r["taps"][i]).astype(np.float64)
    ins, sks = [dev(j) for j in row["src"]], [dev(j) for j, _ in row["skips"]]
    k = row["kind"]
    if k in ("convert", "to_blocked", "maxpool", "stride2_pick"):
        ref = G.eval_row(row, ins, sks, w)
        bad = ~(got == ref) if got.shape == ref.shape else np.ones((1, 1, 1, 1), bool)
        return (np.inf if bad.any() else 0.0), (f"{int(bad.sum())} elements differ (bit-for-bit op), first {first_bad(bad)}" if bad.any() else None)
    if k == "vgg_preprocess":
        ref = G.eval_row(row, ins, sks, w)
        worst, bad = ratio_of(np.abs(got - ref), np.where(np.arange(ref.shape[-1]) < 3, 2.0 ** -14, 0.0) * np.ones_like(ref))
        return worst, (f"{int(bad.sum())} elements outside 2^-14, first {first_bad(bad)}" if bad.any() else None)
    if k == "attention":
        ref, bnd = D.memo(("attn", dtype), lambda q: G.attention_bound(q, dtype, ks), ins[0])
        worst, bad = ratio_of(np.abs(got - ref), bnd)
        return worst, (f"{int(bad.sum())} elements outside attention_ref.bound, worst {worst:.3g}, first {first_bad(bad)}" if bad.any() else None)
    assert k == "conv", k
    ref = D.memo(("ref", kind, cfg, dtype, i), lambda *a: G.eval_row(row, a[:len(ins)], a[len(ins):], w, ks, device=True), *ins, *sks)
    if got.shape != ref.shape:
        return np.inf, f"shape {got.shape} != {ref.shape}"
    if dtype == "bf16":
        c = D.check(got, ref, scale=max(1.0, D.rms(ref)) if row["scaled"] else 1.0)
        msg = None if c["ok"] else f"{c['count']} elements outside the bf16 contract, worst {c['worst']:.3g}, rel-L2 {c['rel_l2']:.3g}, first {c['first']}"
        return c["worst"], msg
    n, T = D.memo(("T", kind, cfg, i), lambda *a: G.bound_T(row, a[:len(ins)], a[len(ins):], w), *ins, *sks)
    bound = (n + 8) * G.U * T + (G.TANH_ALLOW if row["act"] == "tanh" else 0.0)
    err = np.abs(got - ref)
    worst, bad = ratio_of(err, bound)
    if row["act"] == "tanh":
        print(f"TANH {kind} {cfg}: worst |device - fp64| on the tanh output {err.max():.3e}, conv bound there {float(((n + 8) * G.U * T).max()):.3e}")
    return worst, (f"{int(bad.sum())} elements outside (n + 8) 2^-24 T, n = {n}, worst {worst:.3g}, first {first_bad(bad)}" if bad.any() else None)


@pytest.mark.parametrize("kind,cfg,dtype,shape", CASES, ids=IDS)
def test_every_op_per_element(ctx, kind, cfg, dtype, shape):
    r = run(ctx, kind, cfg, dtype, shape)
    t = r["t"]
    assert [o[0] for o in r["ops"]] == [row["name"] for row in t]
    cid, fails, worst_all = case_id(kind, cfg, dtype, shape), [], 0.0
    for i, row in enumerate(t):
        if row["kind"] in ("gap", "dense"):
            continue                                                    # no activation-buffer output: the head is checked below through the model output
        assert row["out"] or i in r["taps"], (i, row["name"])
        worst, msg = compare_row(r, i, kind, cfg, dtype)
        worst_all = max(worst_all, worst)
        print(f"RATIO {cid} op {i} {row['name']}: {worst:.4f}")
        if msg:
            fails.append(f"op {i} {row['name']}: {msg}")
    if kind == "esrgan_d":
        last = max(r["taps"])
        p, bound = G.disc_head(r["taps"][last], G.weights(kind, cfg))
        err = np.abs(r["y"].astype(np.float64) - p)
        worst, bad = ratio_of(err, bound + G.SIGMOID_ALLOW)
        worst_all = max(worst_all, worst)
        print(f"RATIO {cid} head gap+dense+dense: {worst:.4f}   (worst |device - fp64| {err.max():.3e}, derived bound {bound.max():.3e}, p in [{p.min():.3f}, {p.max():.3f}])")
        if bad.any():
            fails.append(f"discriminator head: {int(bad.sum())} outputs outside the bound, worst {worst:.3g}, first {first_bad(bad)}")
    print(f"RATIO {cid} worst of the case: {worst_all:.4f}")
    assert not fails, f"{cid}: " + "; ".join(fails)


@pytest.mark.parametrize("kind,cfg,dtype,shape", CASES, ids=IDS)
def test_taps_change_only_what_the_docs_say(ctx, kind, cfg, dtype, shape):
    r = run(ctx, kind, cfg, dtype, shape)
    assert np.isfinite(r["y"]).all()
    assert r["untapped_equal"]


EDSR64 = [(kind, cfg, dt, shape) for kind, cfg, dt, shape in CASES if kind == "edsr" and cfg[2] == 64 and dt == "bf16"]


@pytest.mark.parametrize("kind,cfg,dtype,shape", EDSR64, ids=[case_id(*c) for c in EDSR64])
def test_edsr_body_convs_run_on_the_kernel_the_shape_selects(ctx, kind, cfg, dtype, shape):
    """Whole 24 x 16 tiles: head-to-body convs (2 per block and the closing one) from 64 channels on conv_stream; ragged: none there, all on conv_rows."""
    r = run(ctx, kind, cfg, dtype, shape)
    body = 2 * cfg[1] + 1
    for ks in (r["kernels"], r["untapped_kernels"]):
        stream = sum(n for k, n in ks.items() if k.startswith("conv_stream"))
        rows = sum(n for k, n in ks.items() if k.startswith("conv_rows"))
        if shape[1] % 24 == 0 and shape[2] % 16 == 0:
            assert stream >= body, ks
        else:
            assert stream == 0 and rows >= body, ks


def test_device_tanh_error_on_these_outputs(ctx):
    """The device's tanhf alone, on the pre-activations of every final_conv2 of the cases: an fp32 conv whose kernel is the centre-tap identity
    returns tanhf(z) of its input exactly as the epilogue computes it (1 z + zeros is exact).  TANH_ALLOW is twice the worst error measured here on
    an MI355X; beyond 2^-20 it would be a finding, not an allowance."""
    k = np.zeros((3, 3, 3, 3), np.float32)
    k[1, 1] = np.eye(3, dtype=np.float32)
    worst = 0.0
    for kind, cfg, _, shapes in G.cases():
        if kind != "esrgan_g":
            continue
        for shape in shapes:
            t, outs = G.chain_of(kind, cfg, shape, "f32")
            row = dict(t[-1], act=None)
            z = G.eval_row(row, [outs[j] for j in row["src"]], [], G.weights(kind, cfg)).astype(np.float32)
            got = host(ctx.conv2d(ctx.to_device(z), k, np.zeros(3, np.float32), act="tanh")).astype(np.float64)
            worst = max(worst, float(np.abs(got - np.tanh(z.astype(np.float64))).max()))
    print(f"TANHF worst |tanhf(z) - tanh(z)| on the final_conv2 pre-activations: {worst:.3e}")
    assert worst <= 2.0 ** -20 and worst <= G.TANH_ALLOW, worst
