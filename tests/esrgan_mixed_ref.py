"""Restated references for the bf16 mixed-precision RRDB trunk of ESRGAN's training step (sr355.gan_train.Tape.trunk_bf16), torch-CPU
in fp64, on the helpers of tests/edsr_mixed_ref.py.  The trunk is the part of the generator between the output of initial_conv (fp32 x0) and the input of
trunk_conv; inside it every stored tensor is bf16, rounded once after an fp64 epilogue; every trunk kernel is rounded once; biases, weight and bias
gradients and everything outside the trunk are never rounded.

  trunk_forward / trunk_backward   the contract, restated (their tapes carry the names the device's tape carries)
  MixedTrunk                       the two as one autograd function, so that the rest of the generator is plain fp64 autograd around it
  generator_t                      oracle.train.generator_forward_t with the trunk replaceable
  pixel_grads                      pixel-L1 loss and gradients of the whole generator, the trunk plain / restated / pinned to a device tape
  teacher_forced                   every tensor of a device tape recomputed from the device's own stored inputs of that stage
"""
import numpy as np
import torch

from edsr_mixed_ref import bf16_bits, conv64, conv_bound, one_minus_cos, rb, rel_l2, rot, t64, wgrad64  # noqa: F401  (re-exported for the tests)
from oracle import models as M
from oracle import train as OT
from sr355.weights import init_weights

SCALE, NB, G, C0 = 2, 2, 32, 64                    # the tests' generator: x2, two RRDBs (six dense blocks), 32 growth channels


def blocks(nb):
    """(b, d, layer prefix, a5, bx) of every dense block in forward order: conv5's alpha and the x-skip's coefficient (an RRDB's third block carries the
    RRDB's r_in + 0.2 * (.) folded into its epilogue)."""
    return [(b, d, f"rrdb_{b}_dense{d}", 0.04 if d == 3 else 0.2, 0.2 if d == 3 else 1.0) for b in range(nb) for d in (1, 2, 3)]


def trunk_names(nb):
    return [f"{n}_conv{k}" for _, _, n, _, _ in blocks(nb) for k in range(1, 6)]


def weight_sets(nb=NB, seed=4000):
    """he-normal initial weights (about half of every ReLU off), and the same with the growth convs' kernels times 0.25 and their biases 0.5: few ReLUs off.
    In both the output conv's kernel is times 0.05: he-normal weights drive the closing tanh into saturation (pixel loss 0.90 on targets in [-1, 1]), where it
    passes almost no gradient and what is left hangs on a few pixels; with an unsaturated output the pixel loss is 0.32 and the gradient is the network's."""
    w = init_weights(M.esrgan_g_layers(SCALE, G, nb), scheme="he_normal", seed=seed)
    w["final_conv2"] = ((w["final_conv2"][0] * np.float32(0.05)).astype(np.float32), w["final_conv2"][1])
    for n in w:                                    # moderate attention logits, as tests/test_train_gpu.py keeps them
        if n.endswith("_f") or n.endswith("_g"):
            w[n] = ((w[n][0] * np.float32(0.25)).astype(np.float32), (w[n][1] * np.float32(0.25)).astype(np.float32))
    on = dict(w)
    for n in trunk_names(nb):
        if not n.endswith("_conv5"):
            on[n] = ((w[n][0] * np.float32(0.25)).astype(np.float32), np.full_like(w[n][1], 0.5))
    return {"he_normal": w, "relu_on": on}


def batch(B=2, n=12, seed=5):
    """(lr, hr) in [-1, 1]."""
    from sr355.synth import make_pairs
    lr, hr = make_pairs(B, n, n, SCALE, seed)
    return (lr * 2.0 - 1.0).astype(np.float32), (hr * 2.0 - 1.0).astype(np.float32)


def _kb(weights, nb):
    return {n: rb(t64(weights[n][0])) for n in trunk_names(nb)}, {n: t64(weights[n][1]) for n in trunk_names(nb)}


# ---------------------------------------------------------------------------------------------------------------- the contract, restated
def trunk_forward(weights, x0, nb):
    """x0: fp64 tensor of the fp32 initial_conv output, NHWC -> (out fp64 holding bf16 values, tape {name: tensor})."""
    k, b = _kb(weights, nb)
    T = {}
    x = rb(x0)
    for bi, d, n, a5, bx in blocks(nb):
        if d == 1:
            r_in = x
        feats = [x]
        for j in range(1, 5):
            feats.append(rb(torch.relu(conv64(torch.cat(feats, dim=-1), k[f"{n}_conv{j}"], b[f"{n}_conv{j}"]))))
        F = T[f"F_{bi}_{d}"] = torch.cat(feats, dim=-1)
        v = a5 * conv64(F, k[f"{n}_conv5"], b[f"{n}_conv5"]) + bx * x
        x = rb(v + r_in) if d == 3 else rb(v)
    T["out"] = x
    return x, T


def trunk_backward(weights, T, dout, nb):
    """T: the forward tape; dout: fp64 tensor of the fp32 gradient of the trunk's output -> (d x0 fp64 holding bf16 values, grads {layer: (dw, db)}, T grown)."""
    k, _ = _kb(weights, nb)
    g = {}
    dR = T[f"dR_{nb - 1}"] = rb(dout)
    dY = dR
    for bi, d, n, a5, bx in reversed(blocks(nb)):
        F = T[f"F_{bi}_{d}"]
        Gb = T[f"G_{bi}_{d}_s5"] = rb(a5 * conv64(dY, rot(k[f"{n}_conv5"])))
        g[f"{n}_conv5"] = wgrad64(F, dY, a5)
        dzs = [None] * 4
        for j in range(4, 0, -1):
            cin = C0 + (j - 1) * G
            dz = dzs[j - 1] = torch.where(F[..., cin:cin + G] > 0, Gb[..., cin:cin + G], torch.zeros(()).double())
            g[f"{n}_conv{j}"] = wgrad64(F[..., :cin], dz)
            v = conv64(dz, rot(k[f"{n}_conv{j}"])) + Gb[..., :cin]
            if j > 1:
                Gb = T[f"G_{bi}_{d}_s{j}"] = torch.cat([rb(v), Gb[..., cin:]], dim=-1)
            else:
                dX = T[f"dX_{bi}_{d}"] = rb(v + bx * dY)
        T[f"dz_{bi}_{d}"] = torch.cat(dzs, dim=-1)
        dY = dX
        if d == 1:
            dR = dY = T[f"drin_{bi}"] = rb(dX + dR)
    return dR, g, T


class MixedTrunk(torch.autograd.Function):
    """The restated trunk inside an fp64 autograd graph: apply(x0 NCHW, nb, names, *kernels and biases in `names` order)."""

    @staticmethod
    def forward(ctx, x0, nb, names, *params):
        w = {n: (params[2 * i].detach(), params[2 * i + 1].detach()) for i, n in enumerate(names)}
        out, T = trunk_forward(w, x0.detach().permute(0, 2, 3, 1), nb)
        ctx.w, ctx.T, ctx.nb, ctx.names = w, T, nb, names
        return out.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, dout):
        dx, g, _ = trunk_backward(ctx.w, ctx.T, dout.permute(0, 2, 3, 1).float().double(), ctx.nb)      # (the incoming gradient is an fp32 tensor on the device)
        return (dx.permute(0, 3, 1, 2), None, None) + tuple(a for n in ctx.names for a in g[n])


class PinnedTrunk(torch.autograd.Function):
    """A device's trunk inside an fp64 autograd graph: its stored output going forward, its stored input gradient going back ("fed the same incoming
    gradient": the fp32 layers outside the trunk then see what the device's own layers saw)."""

    @staticmethod
    def forward(ctx, x0, out, dx):
        ctx.dx = dx
        return out

    @staticmethod
    def backward(ctx, dout):
        return ctx.dx, None, None


def generator_t(p, x, nb, attention, trunk, masks=None):
    """oracle.train.generator_forward_t (x2) with the trunk handed in: trunk(x0 NCHW) -> NCHW."""
    mk = (lambda n: masks.get(n)) if masks else (lambda n: None)
    x = OT._conv_s(x, *p["initial_conv"])
    x = x + OT._conv_s(trunk(x), *p["trunk_conv"])
    if attention:
        x = OT._sa_t(p, x, "self_attention_trunk")
    x = OT._d2s(OT._conv_s(x, *p["upsample_0_conv"]), 2)
    m = mk("upsample_0_conv")
    x = OT._masked_act(x, "lrelu", m) if m is not None else torch.nn.functional.leaky_relu(x, 0.2)
    if attention:
        x = OT._sa_t(p, x, "self_attention_upsample_0")
    x = OT._conv_s(x, *p["final_conv1"], act="relu", mask=mk("final_conv1"))
    return OT._conv_s(x, *p["final_conv2"], act="tanh")


def pixel_grads(weights, lr, hr, nb=NB, attention=True, mode="plain", pinned=None, masks=None):
    """mean |hr - G(lr)| and its gradients {layer: (dw, db)} in fp64.  mode "plain": oracle.train.generator_forward_t as it is; "mixed": the trunk is the
    restated contract; "pinned": the trunk is pinned = (out, d x0) of a device step, NHWC (its layers then get no gradient here)."""
    p = {n: (t64(k).requires_grad_(), t64(b).requires_grad_()) for n, (k, b) in weights.items()}
    x, t = t64(lr).permute(0, 3, 1, 2), t64(hr).permute(0, 3, 1, 2)
    if mode == "plain":
        y = OT.generator_forward_t(p, x, SCALE, nb, attention=attention, masks=masks)
    elif mode == "mixed":
        names = trunk_names(nb)
        y = generator_t(p, x, nb, attention, lambda x0: MixedTrunk.apply(x0, nb, names, *[a for n in names for a in p[n]]), masks)
    else:
        out, dx = (t64(a).permute(0, 3, 1, 2) for a in pinned)
        y = generator_t(p, x, nb, attention, lambda x0: PinnedTrunk.apply(x0, out, dx), masks)
    loss = (t - y).abs().mean()
    loss.backward()
    return float(loss.detach()), {n: (k.grad, b.grad) for n, (k, b) in p.items() if k.grad is not None}


def flat(grads, order):
    return torch.cat([t64(grads[n][s]).reshape(-1) for n in order for s in (0, 1)])


# ---------------------------------------------------------------------------------------------------------------- teacher forcing
def tape_names(nb):
    """Every name a device tape must carry."""
    names = {"x0_f32", "dout_f32", "out", f"dR_{nb - 1}"}
    for b, d, _, _, _ in blocks(nb):
        names |= {f"F_{b}_{d}", f"dz_{b}_{d}", f"dX_{b}_{d}"} | {f"G_{b}_{d}_s{j}" for j in (5, 4, 3, 2)}
        if d == 1:
            names.add(f"drin_{b}")
    return names


def teacher_forced(T, weights, nb):
    """T: {name: fp64 tensor of a device tape's values}.  Every stored tensor -- every channel slice of F and every stage of G taken separately --
    recomputed from the device's own stored inputs of that stage -> (convs [(label, device value, unrounded fp64 value, fp32 bound)],
    exact [(label, device value, fp64 reference to match bitwise)], grads {layer: (dw, db)}, covered: the taped names these checks read as outputs)."""
    k, b = _kb(weights, nb)
    convs, exact, g, covered = [], [], {}, {"x0_f32", "dout_f32"}
    bl = blocks(nb)

    def conv(label, got, xin, kk, bias, alpha=1.0, act=False, skips=()):
        v = conv64(xin, kk, bias)
        v = alpha * (torch.relu(v) if act else v)
        for s in skips:
            v = v + s
        convs.append((label, got, v, conv_bound(xin, kk, bias, alpha, skips)))

    # forward
    for i, (bi, d, n, a5, bx) in enumerate(bl):
        F = T[f"F_{bi}_{d}"]
        covered.add(f"F_{bi}_{d}")
        if i == 0:
            exact.append(("F_0_1[x0]", F[..., :C0], rb(T["x0_f32"])))
        for j in range(1, 5):
            cin = C0 + (j - 1) * G
            conv(f"F_{bi}_{d}[{j}]", F[..., cin:cin + G], F[..., :cin], k[f"{n}_conv{j}"], b[f"{n}_conv{j}"], act=True)
        last = i == len(bl) - 1
        nxt = T["out"] if last else T["F_%d_%d" % bl[i + 1][:2]][..., :C0]
        skips = (bx * F[..., :C0],) + ((T[f"F_{bi}_1"][..., :C0],) if d == 3 else ())
        conv("out" if last else "F_%d_%d[x]" % bl[i + 1][:2], nxt, F, k[f"{n}_conv5"], b[f"{n}_conv5"], alpha=a5, skips=skips)
    covered.add("out")
    # backward
    exact.append((f"dR_{nb - 1}", T[f"dR_{nb - 1}"], rb(T["dout_f32"])))
    covered.add(f"dR_{nb - 1}")
    dR = T[f"dR_{nb - 1}"]
    dY = dR
    for bi, d, n, a5, bx in reversed(bl):
        F = T[f"F_{bi}_{d}"]
        Gs = {j: T[f"G_{bi}_{d}_s{j}"] for j in (5, 4, 3, 2)}
        dz = T[f"dz_{bi}_{d}"]
        covered |= {f"G_{bi}_{d}_s{j}" for j in Gs} | {f"dz_{bi}_{d}", f"dX_{bi}_{d}"}
        conv(f"G_{bi}_{d}_s5", Gs[5], dY, rot(k[f"{n}_conv5"]), None, alpha=a5)
        g[f"{n}_conv5"] = wgrad64(F, dY, a5)
        for j in range(4, 0, -1):
            cin = C0 + (j - 1) * G
            before = Gs[j + 1]                                    # the stage whose slice j is complete
            dzj = dz[..., (j - 1) * G:j * G]
            exact.append((f"dz_{bi}_{d}[{j}]", dzj, torch.where(F[..., cin:cin + G] > 0, before[..., cin:cin + G], torch.zeros(()).double())))
            g[f"{n}_conv{j}"] = wgrad64(F[..., :cin], dzj)
            if j > 1:
                conv(f"G_{bi}_{d}_s{j}[:{cin}]", Gs[j][..., :cin], dzj, rot(k[f"{n}_conv{j}"]), None, skips=(before[..., :cin],))
                exact.append((f"G_{bi}_{d}_s{j}[{cin}:]", Gs[j][..., cin:], before[..., cin:]))      # the channels the accumulate does not own stay
            else:
                conv(f"dX_{bi}_{d}", T[f"dX_{bi}_{d}"], dzj, rot(k[f"{n}_conv1"]), None, skips=(before[..., :C0], bx * dY))
        dY = T[f"dX_{bi}_{d}"]
        if d == 1:
            exact.append((f"drin_{bi}", T[f"drin_{bi}"], rb(dY + dR)))
            covered.add(f"drin_{bi}")
            dR = dY = T[f"drin_{bi}"]
    return convs, exact, g, covered


def check_convs(convs, what=""):
    """The per-element bar of tests/test_edsr_mixed_gpu.py on [(label, device value, unrounded fp64 value v, fp32 bound)]: within 2^-8 |v| + bound of v;
    at most 1e-2 of the elements differ from rb(v), each by one bf16 step (counted on the bits where |v| >= 4 bound, so that the fp32 error cannot
    carry a value across zero).  Prints every figure, then asserts."""
    bits = lambda a: a.float().bfloat16().view(torch.int16).int()
    bad = []
    for label, got, v, bound in convs:
        ref = rb(v)
        excess = float(((got - v).abs() - (2.0 ** -8 * v.abs() + bound)).max())
        differ = got != ref
        share = float(differ.double().mean())
        counted = differ & (v.abs() >= 4 * bound)
        step = int((bits(got) - bits(ref)).abs()[counted].max()) if bool(counted.any()) else 0
        print(f"{what} {label}: worst |got - v| - bound {excess:.3e}; {share:.2e} of the elements differ from the rounded reference, by at most {step} step")
        if not (excess <= 0.0 and share <= 1e-2 and step <= 1):
            bad.append(label)
    assert not bad, bad
