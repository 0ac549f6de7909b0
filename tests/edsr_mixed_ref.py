"""Restated references for EDSR's bf16 mixed-precision training step (sr355.train.edsr_loss_and_grads_bf16; DESIGN.md, "Mixed-precision training"),
torch-CPU in fp64.  bf16 rounding is tensor.float().bfloat16(); the rounding points are the contract's: every conv kernel once, every stored
activation and activation gradient once after an fp64 epilogue, biases / target / loss / weight and bias gradients never."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import models as M
from sr355.weights import init_weights

F64 = torch.float64


def rb(t):
    """fp64 tensor -> nearest bf16 (through fp32, round to nearest even), as fp64."""
    return t.float().bfloat16().double()


def t64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().double()
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def bf16_bits(t):
    """bf16 tensor (any device) -> int16 NumPy array of its bits."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def conv64(x, w, b=None):
    """3x3 SAME conv, NHWC x, HWIO w, fp64."""
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(3, 2, 0, 1), b, padding=w.shape[0] // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def rot(w):
    """Kernel of the input-gradient conv: rotate by 180 degrees, swap the channel axes."""
    return w.flip(0, 1).permute(0, 1, 3, 2).contiguous()


def d2s(x, r):
    """tf.nn.depth_to_space (DCR): [B,H,W,r*r*C] -> [B,H*r,W*r,C]."""
    B, H, W, C = x.shape
    c = C // (r * r)
    return x.reshape(B, H, W, r, r, c).permute(0, 1, 3, 2, 4, 5).reshape(B, H * r, W * r, c)


def s2d(x, r):
    B, Hr, Wr, C = x.shape
    H, W = Hr // r, Wr // r
    return x.reshape(B, H, r, W, r, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H, W, r * r * C)


def wgrad64(x, dy, scale=1.0):
    """(dw HWIO [3,3,Cin,Cout], db [Cout]) of a 3x3 SAME conv in fp64."""
    B, H, W, _ = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    dw = torch.stack([torch.stack([torch.einsum("bhwi,bhwo->io", xp[:, ky:ky + H, kx:kx + W], dy) for kx in range(3)]) for ky in range(3)])
    return scale * dw, scale * dy.sum(dim=(0, 1, 2))


def layer_names(num_res_blocks):
    return ["conv2d"] + [f"conv2d_{i}" for i in range(1, 2 * num_res_blocks + 5)]


def weight_sets(scale, num_res_blocks=2, num_filters=64, seed=2000):
    """The two weight sets of the tests: he-normal initial weights (the clip and ReLU masks are busy), and the same with the last kernel times 0.02
    and the last bias 0.5, whose output stays inside (0, 1): the clip mask is idle."""
    w = init_weights(M.edsr_layers(scale=scale, num_res_blocks=num_res_blocks, num_filters=num_filters), scheme="he_normal", seed=seed)
    last = layer_names(num_res_blocks)[2 * num_res_blocks + 2 + (2 if scale == 4 else 1)]
    assert last == list(w)[-1]
    inside = dict(w)
    inside[last] = ((w[last][0] * np.float32(0.02)).astype(np.float32), np.full_like(w[last][1], 0.5))
    return {"he_normal": w, "inside": inside}


def batch(scale, B=2, n=12, seed=5):
    from sr355.synth import make_pairs
    return make_pairs(B, n, n, scale, seed)


def _graph(scale, num_res_blocks):
    names = layer_names(num_res_blocks)
    it = iter(names)
    head = next(it)
    blocks = [(i, next(it), next(it)) for i in range(1, num_res_blocks + 1)]
    body = next(it)
    ups = [(j, next(it), r) for j, r in enumerate([scale] if scale in (2, 3) else [2, 2], 1)]
    return head, blocks, body, ups, next(it)


def loss_grad64(pre, t):
    """(y, loss, unrounded dpre) in fp64 from the stored pre and the fp32 target."""
    y = pre.clamp(0.0, 1.0)
    d = y - t
    return y, (d * d).mean(), torch.where((pre >= 0) & (pre <= 1), 2.0 / d.numel() * d, torch.zeros_like(d))


def dpre_bits_ref(pre, t):
    """dpre as the contract states it: fp32 2 / N * (y - t) evaluated in NumPy's order, rounded to nearest even; 0 outside the clip range."""
    p = pre.float().numpy()
    tt = np.asarray(t, np.float32)
    y = np.clip(p, np.float32(0), np.float32(1))
    g = np.float32(2.0 / p.size) * (y - tt)
    g = np.where((p >= 0) & (p <= 1), g, np.float32(0)).astype(np.float32)
    return torch.from_numpy(g).bfloat16()


def mixed_step_ref(weights, x, t, scale, num_res_blocks, res_scaling):
    """The contract, restated: -> (tape {name: fp64 tensor holding bf16 values}, loss fp64, grads {layer: (dw, db)} fp64)."""
    head, blocks, body, ups, out = _graph(scale, num_res_blocks)
    k = {n: rb(t64(w[0])) for n, w in weights.items()}
    b = {n: t64(w[1]) for n, w in weights.items()}
    T, g = {}, {}
    t32 = np.asarray(t, np.float32)
    x, t = rb(t64(x)), t64(t32)
    T["x"] = x
    h0 = T["h0"] = rb(conv64(x, k[head], b[head]))
    cur, tape = h0, []
    for i, na, nb in blocks:
        tt = T[f"tt_{i}"] = rb(torch.relu(conv64(cur, k[na], b[na])))
        nxt = T[f"nxt_{i}"] = rb(res_scaling * conv64(tt, k[nb], b[nb]) + cur)
        tape.append((i, na, nb, cur, tt))
        cur = nxt
    bd = T["body"] = rb(conv64(cur, k[body], b[body]) + h0)
    up, ut = bd, []
    for j, nu, r in ups:
        v = T[f"up_{j}"] = rb(d2s(conv64(up, k[nu], b[nu]), r))
        ut.append((j, nu, up, r))
        up = v
    pre = T["pre"] = rb(conv64(up, k[out], b[out]))
    _, loss, _ = loss_grad64(pre, t)
    dpre = T["dpre"] = dpre_bits_ref(pre, t32).double()
    g[out] = wgrad64(up, dpre)
    d = T["d_out"] = rb(conv64(dpre, rot(k[out])))
    for j, nu, uin, r in reversed(ut):
        dv = T[f"dv_{j}"] = s2d(d, r)
        g[nu] = wgrad64(uin, dv)
        d = T[f"d_up_{j}"] = rb(conv64(dv, rot(k[nu])))
    d_h0 = d
    g[body] = wgrad64(cur, d)
    d = T["d_body"] = rb(conv64(d, rot(k[body])))
    for i, na, nb, cin, tt in reversed(tape):
        g[nb] = wgrad64(tt, d, res_scaling)
        du = T[f"du_{i}"] = rb(res_scaling * conv64(d, rot(k[nb])))
        dt = T[f"dt_{i}"] = torch.where(tt > 0, du, torch.zeros_like(du))
        g[na] = wgrad64(cin, dt)
        d = T[f"d_{i}"] = rb(conv64(dt, rot(k[na])) + d + (d_h0 if i == 1 else 0.0))
    g[head] = wgrad64(x, d)
    return T, loss, g


def autograd_ref(weights, x, t, scale, num_res_blocks, res_scaling):
    """Plain fp64 autograd on the unrounded weights and batch: -> (loss, grads {layer: (dw, db)})."""
    head, blocks, body, ups, out = _graph(scale, num_res_blocks)
    p = {n: (t64(w[0]).requires_grad_(), t64(w[1]).requires_grad_()) for n, w in weights.items()}
    x, t = t64(x), t64(t)
    h0 = conv64(x, *p[head])
    cur = h0
    for _, na, nb in blocks:
        cur = res_scaling * conv64(torch.relu(conv64(cur, *p[na])), *p[nb]) + cur
    up = conv64(cur, *p[body]) + h0
    for _, nu, r in ups:
        up = d2s(conv64(up, *p[nu]), r)
    y = conv64(up, *p[out]).clamp(0.0, 1.0)
    loss = ((y - t) ** 2).mean()
    loss.backward()
    return loss.detach(), {n: (kb[0].grad, kb[1].grad) for n, kb in p.items()}


def flat(grads, order):
    return torch.cat([t64(grads[n][s]).reshape(-1) for n in order for s in (0, 1)])


def one_minus_cos(a, b):
    return float(1.0 - torch.dot(a, b) / (a.norm() * b.norm()))


def rel_l2(got, ref):
    got, ref = t64(got), t64(ref)
    den = float(ref.norm())
    return float((got - ref).norm()) / den if den > 0 else float((got - ref).norm())


def conv_bound(xin, kk, bias, alpha=1.0, skips=()):
    """The fp32 dot-product bound of one stored conv output: (9 Cin + 2) 2^-24 S, S the same conv on absolute values."""
    S = abs(alpha) * conv64(xin.abs(), kk.abs(), None if bias is None else bias.abs())
    for s in skips:
        S = S + s.abs()
    return (9 * kk.shape[2] + 2) * 2.0 ** -24 * S


def teacher_forced(tape, weights, t, scale, num_res_blocks, res_scaling):
    """Every tensor of a device tape recomputed in fp64 from the DEVICE's own stored inputs of that step.  tape: {name: fp64 tensor of the device's bf16
    values}.  -> (convs [(name, unrounded fp64 value, fp32 bound)], exact [(name, fp64 reference to match bitwise)], grads {layer: (dw, db)} fp64)."""
    head, blocks, body, ups, out = _graph(scale, num_res_blocks)
    k = {n: rb(t64(w[0])) for n, w in weights.items()}
    b = {n: t64(w[1]) for n, w in weights.items()}
    T, convs, exact, g = tape, [], [], {}

    def fwd(name, xin, layer, alpha=1.0, act=False, skips=(), r=1):
        v = conv64(xin, k[layer], b[layer])
        v = alpha * (torch.relu(v) if act else v)
        for s in skips:
            v = v + s
        bound = conv_bound(xin, k[layer], b[layer], alpha, skips)
        convs.append((name, d2s(v, r) if r > 1 else v, d2s(bound, r) if r > 1 else bound))

    def bwd(name, dy, layer, alpha=1.0, skips=()):
        v = alpha * conv64(dy, rot(k[layer]))
        for s in skips:
            v = v + s
        convs.append((name, v, conv_bound(dy, rot(k[layer]), None, alpha, skips)))

    fwd("h0", T["x"], head)
    cur = T["h0"]
    for i, na, nb in blocks:
        fwd(f"tt_{i}", cur, na, act=True)
        fwd(f"nxt_{i}", T[f"tt_{i}"], nb, alpha=res_scaling, skips=(cur,))
        cur = T[f"nxt_{i}"]
    fwd("body", cur, body, skips=(T["h0"],))
    up = T["body"]
    for j, nu, r in ups:
        fwd(f"up_{j}", up, nu, r=r)
        up = T[f"up_{j}"]
    fwd("pre", up, out)
    exact.append(("dpre", dpre_bits_ref(T["pre"], t).double()))
    n_up = len(ups)
    g[out] = wgrad64(T[f"up_{n_up}"], T["dpre"])
    bwd("d_out", T["dpre"], out)
    d = T["d_out"]
    for j, nu, r in reversed(ups):
        exact.append((f"dv_{j}", s2d(d, r)))
        uin = T["body"] if j == 1 else T[f"up_{j - 1}"]
        g[nu] = wgrad64(uin, T[f"dv_{j}"])
        bwd(f"d_up_{j}", T[f"dv_{j}"], nu)
        d = T[f"d_up_{j}"]
    d_h0 = d
    g[body] = wgrad64(T[f"nxt_{num_res_blocks}"], d)
    bwd("d_body", d, body)
    d = T["d_body"]
    for i, na, nb in reversed(blocks):
        tt, cin = T[f"tt_{i}"], (T["h0"] if i == 1 else T[f"nxt_{i - 1}"])
        g[nb] = wgrad64(tt, d, res_scaling)
        bwd(f"du_{i}", d, nb, alpha=res_scaling)
        exact.append((f"dt_{i}", torch.where(tt > 0, T[f"du_{i}"], torch.zeros_like(tt))))
        g[na] = wgrad64(cin, T[f"dt_{i}"])
        bwd(f"d_{i}", T[f"dt_{i}"], na, skips=(d, d_h0) if i == 1 else (d,))
        d = T[f"d_{i}"]
    g[head] = wgrad64(T["x"], d)
    return convs, exact, g
