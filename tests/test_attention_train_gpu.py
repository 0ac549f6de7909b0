"""The streamed training attention (csrc/attention_train.hip: sr_attention_fwd_lse / sr_attention_bwd) against the fp64 materialised
reference of tests/attention_train_ref.py, at the edges of the 32-key sub-tile, the 64-row tile and the 128-row workgroup; then through
Tape(attention_impl="streamed"), one ESRGAN train step, and the condition that no [B,N,N] tensor is ever allocated."""
import numpy as np
import pytest
import torch

import attention_ref as R
import attention_train_ref as TR
from oracle import models as M
from oracle import ops as O
from oracle import train as OT
from sr355.weights import init_weights

pytestmark = pytest.mark.gpu

B = 2
SIZES = (1, 31, 32, 33, 127, 128, 129, 160, 257)
WIDE = float(np.sqrt(10.0))                        # scores span about +-80
CASES = [(n, 1.0) for n in SIZES] + [(33, WIDE), (257, WIDE)]


def _run(ctx, q, k, v, do):
    qd, kd, vd, dod = (ctx.to_device(a) for a in (q, k, v, do))
    o, lse = ctx.attention_fwd_lse(qd, kd, vd)
    dq, dk, dv = ctx.attention_bwd(qd, kd, vd, o, dod, lse)
    return {n: t.cpu().numpy() for n, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv))}


def _check(got, ref, q, k, v, label):
    """Every figure is printed before anything is asserted."""
    n = q.shape[1]
    k64, q64, v64 = (np.asarray(a, np.float64) for a in (k, q, v))
    _, A = R.core_fp64(k64, q64, v64, np.e)
    figures = {"o / bound": R.worst_ratio(got["o"], ref["o"], R.bound(ref["o"], A, "f32", R.score_scale(k64, q64), n)),
               "lse / tol": TR.lse_ratio(got["lse"], ref["lse"])}
    for name in ("dq", "dk", "dv"):
        figures[name + " rel-L2"] = TR.rel_l2(got[name], ref[name])
    print(label, {a: f"{b:.3g}" for a, b in figures.items()})
    assert got["o"].shape == (B, n, 32) and got["lse"].shape == (B, n) and got["dq"].shape == got["dk"].shape == (B, n, 8) and got["dv"].shape == (B, n, 32)
    assert figures["o / bound"] <= 1.0 and figures["lse / tol"] <= 1.0, (label, figures)
    for name in ("dq", "dk", "dv"):
        assert figures[name + " rel-L2"] <= TR.GRAD_TOL, (label, figures)


@pytest.mark.parametrize("n,sd", CASES)
def test_forward_lse_and_backward_against_fp64(ctx, n, sd):
    q, k, v, do = TR.gauss_case(1000 + n, B, n, sd)
    _check(_run(ctx, q, k, v, do), TR.forward_backward_fp64(q, k, v, do), q, k, v, f"N={n} sd={sd:.3g}")


def test_operands_of_a_fused_buffer_give_the_same_bits(ctx):
    """q, k, v as three dense tensors and as channel ranges f | g | h of one [B,N,64] buffer (row stride 64, image stride N * 64)."""
    n = 129
    q, k, v, do = TR.gauss_case(77, B, n, 1.0)
    dense = _run(ctx, q, k, v, do)
    buf = ctx.to_device(np.concatenate([k, q, v, np.full((B, n, 16), np.nan, np.float32)], axis=-1))
    kd, qd, vd = buf[..., 0:8], buf[..., 8:16], buf[..., 16:48]
    o, lse = ctx.attention_fwd_lse(qd, kd, vd)
    dq, dk, dv = ctx.attention_bwd(qd, kd, vd, o, ctx.to_device(do), lse)
    for name, t in (("o", o), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv)):
        assert np.array_equal(t.cpu().numpy(), dense[name]), name
    with pytest.raises(ValueError):
        ctx.attention_fwd_lse(qd, kd[:, :-1], vd)
    with pytest.raises(ValueError):
        ctx.attention_fwd_lse(buf[..., 0:16:2], kd, vd)


def test_abi_refuses_bad_sizes_strides_and_alignment(ctx):
    """The C entry points themselves (under the Python checks): SR_ERR_INVALID with a message, nothing launched."""
    from sr355 import _lib as L
    n = 33
    q, k, v, do = (ctx.to_device(a) for a in TR.gauss_case(3, B, n, 1.0))
    o, lse = ctx.attention_fwd_lse(q, k, v)
    p = lambda t, off=0: t.data_ptr() + off
    fwd = lambda *a: ctx.lib.sr_attention_fwd_lse(ctx.h, *a, ctx.stream())
    bwd = lambda *a: ctx.lib.sr_attention_bwd(ctx.h, *a, ctx.stream())
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    assert fwd(p(q), p(k), p(v), 8, 8, 32, B, n, p(o), p(lse)) == L.SR_OK
    for bad in ((p(q), p(k), p(v), 8, 8, 32, B, 0, p(o), p(lse)),           # no tokens
                (p(q), p(k), p(v), 8, 8, 32, 0, n, p(o), p(lse)),           # no images
                (p(q), p(k), p(v), 4, 8, 32, B, n, p(o), p(lse)),           # a row stride shorter than the row
                (p(q), p(k), p(v), 8, 8, 34, B, n, p(o), p(lse)),           # rows not 16-byte aligned
                (p(q, 4), p(k), p(v), 8, 8, 32, B, n, p(o), p(lse)),        # a pointer not 16-byte aligned
                (p(q), p(k), None, 8, 8, 32, B, n, p(o), p(lse))):
        assert fwd(*bad) == L.SR_ERR_INVALID and ctx.lib.sr_last_error(ctx.h)
    for bad in ((p(q), p(k), p(v), p(o), p(do), p(lse), 8, 8, 32, B, -1, p(dq), p(dk), p(dv)),
                (p(q), p(k), p(v), p(o), p(do), p(lse), 8, 6, 32, B, n, p(dq), p(dk), p(dv)),
                (p(q), p(k), p(v), p(o), p(do, 8), p(lse), 8, 8, 32, B, n, p(dq), p(dk), p(dv)),
                (p(q), p(k), p(v), p(o), p(do), None, 8, 8, 32, B, n, p(dq), p(dk), p(dv))):
        assert bwd(*bad) == L.SR_ERR_INVALID and ctx.lib.sr_last_error(ctx.h)
    with pytest.raises(ValueError):
        ctx.attention_bwd(q, k, v, o, do[:, :, :16].contiguous(), lse)


def test_backward_is_bit_identical_from_run_to_run(ctx):
    q, k, v, do = (ctx.to_device(a) for a in TR.gauss_case(5, B, 257, 1.0))
    o, lse = ctx.attention_fwd_lse(q, k, v)
    first = [t.cpu().numpy() for t in ctx.attention_bwd(q, k, v, o, do, lse)]
    again = [t.cpu().numpy() for t in ctx.attention_bwd(q, k, v, o, do, lse)]
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def test_zero_output_gradient_gives_exactly_zero_gradients(ctx):
    q, k, v, do = TR.gauss_case(6, B, 160, 1.0)
    got = _run(ctx, q, k, v, np.zeros_like(do))
    for name in ("dq", "dk", "dv"):
        assert not got[name].any(), name


def test_zero_queries_average_the_values(ctx):
    n = 129
    q, k, v, do = TR.gauss_case(8, B, n, 1.0)
    q = np.zeros_like(q)
    got, ref = _run(ctx, q, k, v, do), TR.forward_backward_fp64(q, k, v, do)
    v64 = v.astype(np.float64)
    mean, A = np.broadcast_to(v64.mean(axis=1, keepdims=True), v64.shape), np.broadcast_to(np.abs(v64).mean(axis=1, keepdims=True), v64.shape)
    ratio = R.worst_ratio(got["o"], mean, R.bound(mean, A, "f32", np.zeros((B, n, 1)), n))
    print("zero queries: o / bound", ratio, "dq rel-L2", TR.rel_l2(got["dq"], ref["dq"]))
    assert ratio <= 1.0
    assert np.abs(got["lse"] - np.log(n)).max() <= TR.LSE_TOL * max(1.0, np.log(n))
    assert TR.rel_l2(got["dq"], ref["dq"]) <= TR.GRAD_TOL


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("shape", [(2, 6, 5, 64), (1, 13, 11, 64)])
def test_attention_layer_forward_backward_streamed(ctx, shape):
    """test_attention_forward_backward_materialised with attention_impl="streamed": the layer and every gradient against oracle.train._sa_t in fp64."""
    from sr355 import gan_train as GT
    rng = np.random.default_rng(4)
    w = init_weights(M.self_attention_layers("sa"), seed=9)
    x = (0.5 * rng.standard_normal(shape)).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    t = GT.Tape(ctx, w, attention_impl="streamed")
    xv = GT.Var(ctx.to_device(x))
    y = t.attention(xv, "sa")
    assert _rel(y.v.cpu().numpy(), O.self_attention(x, *w["sa_f"], *w["sa_g"], *w["sa_h"], *w["sa_v"], dtype=np.float64)) <= 1e-5
    y.g = ctx.to_device(dy)
    t.backward()
    p = OT._params(w)
    xt = torch.tensor(x.astype(np.float64)).permute(0, 3, 1, 2).requires_grad_(True)
    OT._sa_t(p, xt, "sa").backward(torch.tensor(dy.astype(np.float64)).permute(0, 3, 1, 2))
    print(shape, "dx", _rel(xv.g.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy()),
          {n: (_rel(t.grads[n][0].cpu().numpy(), p[n][0].grad.numpy()), float(np.abs(t.grads[n][1].cpu().numpy() - p[n][1].grad.numpy()).max())) for n in w})
    assert _rel(xv.g.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy()) <= 2e-5
    for n in w:
        assert _rel(t.grads[n][0].cpu().numpy(), p[n][0].grad.numpy()) <= 5e-5, n
        if n.endswith("_f"):       # a key bias shifts every score of a row by the same amount: softmax ignores it, the gradient is exactly zero
            assert np.abs(t.grads[n][1].cpu().numpy()).max() <= 1e-5
        else:
            assert _rel(t.grads[n][1].cpu().numpy(), p[n][1].grad.numpy()) <= 5e-5, n


def test_esrgan_train_step_streamed(ctx):
    """test_esrgan_train_step's small configuration (x2, NB 1, G 8, batch 2 of 12 x 12) with the generator's SelfAttention layers streamed: losses, every
    generator gradient and the updated weights against oracle.train.esrgan_train_step_ref."""
    from sr355 import gan_train as GT
    scale, nb, G = 2, 1, 8
    gw = init_weights(M.esrgan_g_layers(scale, G, nb), seed=3000)
    gw = {n: ((k * 0.25, b * 0.25) if (n.endswith("_f") or n.endswith("_g")) else (k, b)) for n, (k, b) in gw.items()}     # moderate attention logits
    dw = init_weights(M.discriminator_layers(), seed=5000)
    vw = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=6000)
    vw = {n: (k * 0.05 if n == "block1_conv1" else k, b) for n, (k, b) in vw.items()}
    rng = np.random.default_rng(7)
    lr = rng.uniform(-1, 1, (2, 12, 12, 3)).astype(np.float32)
    hr = rng.uniform(-1, 1, (2, 12 * scale, 12 * scale, 3)).astype(np.float32)
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=True, g_lr=1e-4, d_lr=1e-5, u_seed=3, attention_impl="streamed")
    assert tr.generator_tape().attention_impl == "streamed"
    u0 = {n: v.copy() for n, v in tr.u.items()}
    out = tr.train_step(lr, hr)
    ref = OT.esrgan_train_step_ref(gw, dw, u0, vw, lr, hr, scale, nb, attention=True)
    for k, v in ref["losses"].items():
        assert abs(out[k] - v) <= 2e-4 * max(1.0, abs(v)), (k, out[k], v)
    for n, (rk, rb) in ref["d_grads"].items():
        assert _rel(tr.last_grads["d"][n][0], rk) <= 2e-4 and _rel(tr.last_grads["d"][n][1], rb) <= 2e-4, ("d", n)
    dy = tr.last_dy.cpu().numpy().astype(np.float64)
    off = np.abs(dy - ref["dy"]) > 1e-5 * np.abs(ref["dy"]).max()      # pixels on another branch of a loss network's kink (see test_esrgan_train_step)
    assert off.mean() <= 0.01, off.mean()
    assert _rel(np.where(off, 0, dy), np.where(off, 0, ref["dy"])) <= 1e-4
    ref = OT.esrgan_train_step_ref(gw, dw, u0, vw, lr, hr, scale, nb, attention=True, dy_override=dy)
    assert set(tr.last_grads["g"]) == set(ref["g_grads"])
    errs = sorted(((_rel(tr.last_grads["g"][n][0], ref["g_grads"][n][0]), n) for n in ref["g_grads"]), reverse=True)
    berrs = sorted(((float(np.abs(tr.last_grads["g"][n][1] - ref["g_grads"][n][1]).max() / max(np.abs(ref["g_grads"][n][1]).max(), 1e-3)), n)
                    for n in ref["g_grads"]), reverse=True)
    print("worst generator kernel / bias gradients", errs[:3], berrs[:3])
    assert errs[0][0] <= 2e-4, errs[:3]
    assert berrs[0][0] <= 2e-4, berrs[:3]
    for n in ref["gw"]:
        assert _rel(tr.gw[n][0] - gw[n][0], ref["gw"][n][0] - gw[n][0]) <= 5e-3, n


def test_streamed_layer_allocates_no_score_matrix(ctx):
    """A condition, not a measurement: one streamed layer forward + backward at N = 4096 raises the peak of allocated device memory by less than
    ONE N x N fp32 matrix (64 MiB); the materialised path holds at least three of them."""
    from sr355 import gan_train as GT
    H = W = 64
    n = H * W
    rng = np.random.default_rng(11)
    w = init_weights(M.self_attention_layers("sa"), seed=9)
    x = ctx.to_device((0.5 * rng.standard_normal((1, H, W, 64))).astype(np.float32))
    dy = ctx.to_device(rng.standard_normal((1, H, W, 64)).astype(np.float32))
    t = GT.Tape(ctx, w, attention_impl="streamed")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    xv = GT.Var(x)
    y = t.attention(xv, "sa")
    y.g = dy
    t.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("peak rise", rise / 2 ** 20, "MiB; one score matrix", n * n * 4 / 2 ** 20, "MiB")
    assert xv.g is not None and bool(torch.isfinite(xv.g).all())
    assert rise < n * n * 4, rise


def test_streamed_and_materialised_layers_agree(ctx):
    """On top of the oracle comparisons: dx of the two Tape paths at [2,24,24,64] within the sum of their oracle bounds."""
    from sr355 import gan_train as GT
    rng = np.random.default_rng(12)
    w = init_weights(M.self_attention_layers("sa"), seed=9)
    x = ctx.to_device((0.5 * rng.standard_normal((2, 24, 24, 64))).astype(np.float32))
    dy = ctx.to_device(rng.standard_normal((2, 24, 24, 64)).astype(np.float32))
    dx = {}
    for impl in GT.ATTENTION_IMPLS:
        t = GT.Tape(ctx, w, attention_impl=impl)
        xv = GT.Var(x)
        y = t.attention(xv, "sa")
        y.g = dy
        t.backward()
        dx[impl] = xv.g.cpu().numpy()
    print("streamed vs materialised dx", _rel(dx["streamed"], dx["materialised"]))
    assert _rel(dx["streamed"], dx["materialised"]) <= 4e-5
