"""Restated references for training a G = 8 dense block on the LDS-resident kernels (csrc/dense_block_train.hip; sr355.gan_train.Tape.trunk_lds),
torch-CPU / NumPy, on the helpers of tests/edsr_mixed_ref.py and the parametric parts of tests/esrgan_mixed_ref.py (which fixes G = 32 elsewhere).

  pack_forward_np / pack_backward_np / unpack_*   the fragment layouts of csrc/dense_block_lds.h, restated from its rules
  block_forward / block_backward                  the arithmetic contract of one block (3.26's, nothing added), in fp64 or -- dtype=torch.float32 -- fp32
  forward_checks / backward_checks                every stored tensor recomputed in fp64 from the DEVICE's own stored inputs of that stage (teacher forcing)
  weight_sets / trunk_backward / pixel_grads      the trunk at G = 8 inside the generator, for the end-to-end tests
"""
import numpy as np
import torch

from edsr_mixed_ref import conv64, conv_bound, rb, rot, t64, wgrad64
from esrgan_mixed_ref import C0, PinnedTrunk, SCALE, _kb, blocks, generator_t, trunk_forward, trunk_names  # noqa: F401  (re-exported for the tests)
from oracle import models as M
from oracle import train as OT
from sr355.weights import init_weights

G, CC = 8, 96
CIN = [64, 72, 80, 88, 96]
COUT = [8, 8, 8, 8, 64]
# the forward kernel's own edge cases: (B, H, W, workgroup cap); the widest W at H = 24 is read from the library by the GPU test
CASES = [(5, 24, 24, 2), (3, 1, 1, 0), (4, 13, 21, 3), (2, 5, 31, 0), (2, 31, 5, 0)]


# ---------------------------------------------------------------------------------------------------------------- fragment layouts (dense_block_lds.h)
NFRAG_F, NFRAG_B, NBIAS = 207, 288, 128
NCHUNKS = [2, 3, 3, 3, 3]
FRAG0 = [0, 18, 45, 72, 99]
BBLOCKS = [4, 5, 5, 6, 6]                                   # ceil(cin / 16)
BFRAG0 = [108, 144, 189, 234, 0]


def bf16_bits_np(a):
    """fp32 array -> uint16 bf16 bits, round to nearest even (no NaNs here)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def pack_forward_np(ws):
    """ws: five (kernel HWIO fp32, bias) -> (fragments uint16 [207, 64, 8], bias fp32 [128]): fragment (tap, chunk c, cout block n) of conv k at
    FRAG0[k] + (tap * nc + c) * nb + n; lane l, element j = cin 32 c + 8 (l >> 4) + j, cout 16 n + (l & 15); zero beyond the conv's own cins / couts."""
    out = np.zeros((NFRAG_F, 64, 8), np.uint16)
    bias = np.zeros(NBIAS, np.float32)
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    for i, (k, b) in enumerate(ws):
        cin, cout, nc, nb = CIN[i], COUT[i], NCHUNKS[i], 1 if i < 4 else 4
        kb = bf16_bits_np(k).reshape(9, cin, cout)
        for tap in range(9):
            for c in range(nc):
                for n in range(nb):
                    ci, co = 32 * c + 8 * (l >> 4) + j, 16 * n + (l & 15) + 0 * j
                    ok = (ci < cin) & (co < cout)
                    out[FRAG0[i] + (tap * nc + c) * nb + n][ok] = kb[tap][ci[ok], co[ok]]
        bias[(16 * i if i < 4 else 64):(16 * i if i < 4 else 64) + cout] = b
    return out, bias


def pack_backward_np(ws):
    """-> uint16 [288, 64, 8]: the input-gradient fragments.  conv5: (tap, chunk c, block n) at (tap * 2 + c) * 6 + n, lane l, element j =
    kernel[8 - tap][cin 16 n + (l & 15)][cout 32 c + 8 (l >> 4) + j]; conv k < 5: (tap, block n) at BFRAG0[k] + tap * nb + n, lanes < 16 only,
    element j = kernel[8 - tap][cin 16 n + l][cout j], zero beyond the conv's cins."""
    out = np.zeros((NFRAG_B, 64, 8), np.uint16)
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    k5 = bf16_bits_np(ws[4][0]).reshape(9, 96, 64)
    for tap in range(9):
        for c in range(2):
            for n in range(6):
                out[(tap * 2 + c) * 6 + n] = k5[8 - tap][16 * n + (l & 15) + 0 * j, 32 * c + 8 * (l >> 4) + j]
    for i in range(4):
        cin, nb = CIN[i], BBLOCKS[i]
        kb = bf16_bits_np(ws[i][0]).reshape(9, cin, 8)
        for tap in range(9):
            for n in range(nb):
                ci = 16 * n + np.arange(16)
                ok = ci < cin
                out[BFRAG0[i] + tap * nb + n][:16][ok] = kb[8 - tap][ci[ok], :]
    return out


def unpack_backward_np(frags):
    """The kernels the input-gradient fragments encode, as uint16 HWIO arrays of the ROTATED, TRANSPOSED convs: conv5 [3,3,64,96], conv k [3,3,8,cin_k]; and
    whether everything the layout calls padding is zero."""
    outs, pad_zero = [], True
    for i in range(4):
        cin, nb = CIN[i], BBLOCKS[i]
        w = np.zeros((9, 8, 16 * nb), np.uint16)
        for tap in range(9):
            for n in range(nb):
                f = frags[BFRAG0[i] + tap * nb + n]
                w[tap][:, 16 * n:16 * n + 16] = f[:16].T
                pad_zero &= not f[16:].any()
        pad_zero &= not w[:, :, cin:].any()
        outs.append(w[:, :, :cin].reshape(3, 3, 8, cin))
    w = np.zeros((9, 64, 96), np.uint16)
    l, j = np.arange(64)[:, None], np.arange(8)[None, :]
    for tap in range(9):
        for c in range(2):
            for n in range(6):
                w[tap][32 * c + 8 * (l >> 4) + j, 16 * n + (l & 15) + 0 * j] = frags[(tap * 2 + c) * 6 + n]
    outs.append(w.reshape(3, 3, 64, 96))
    return outs, pad_zero


# ---------------------------------------------------------------------------------------------------------------- inputs
def block_weights(seed, conv5_gain=16.0):
    """Five (kernel, bias) of one block, he-normal; conv5 times 2^4 so that the skips do not hide it (tests/test_dense_block_gpu.py)."""
    rng = np.random.default_rng(seed)
    ws = []
    for i in range(5):
        k = rng.normal(0, np.sqrt(2.0 / (9 * CIN[i])), (3, 3, CIN[i], COUT[i])).astype(np.float32)
        if i == 4:
            k = (k * np.float32(conv5_gain)).astype(np.float32)
        ws.append((k, rng.normal(0, 0.1, COUT[i]).astype(np.float32)))
    return ws


def case_inputs(B, H, W, seed=0):
    """(x, r_in, dY): bf16-valued fp32 arrays [B,H,W,64]."""
    rng = np.random.default_rng(1000 * seed + 97 * B + 13 * H + W)
    mk = lambda: torch.from_numpy(rng.normal(0, 1, (B, H, W, 64)).astype(np.float32)).bfloat16().float().numpy()
    return mk(), mk(), mk()


# ---------------------------------------------------------------------------------------------------------------- the contract of one block
def _conv(x, w, b, dtype):
    if dtype == torch.float64:
        return conv64(x, w, b)
    y = torch.nn.functional.conv2d(x.to(dtype).permute(0, 3, 1, 2), w.to(dtype).permute(3, 2, 0, 1), None if b is None else b.to(dtype), padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def _r(t):
    return t.float().bfloat16().to(t.dtype)


def block_forward(ws, x, a5, bx, r_in=None, dtype=torch.float64):
    """-> (F [B,H,W,96], out [B,H,W,64]), bf16 values in `dtype`: slice k = bf16(relu(conv_k(F[:cin_k]) + b_k)); out = bf16(a5 (conv5(F) + b5) + bx x [+ r_in])."""
    k = [rb(t64(w[0])).to(dtype) for w in ws]
    b = [t64(w[1]).to(dtype) for w in ws]
    feats = [t64(x).to(dtype)]
    for i in range(4):
        feats.append(_r(torch.relu(_conv(torch.cat(feats, -1), k[i], b[i], dtype))))
    F = torch.cat(feats, -1)
    v = a5 * _conv(F, k[4], b[4], dtype) + bx * feats[0]
    if r_in is not None:
        v = v + t64(r_in).to(dtype)
    return F, _r(v)


def block_backward(ws, F, dY, a5, bx, dtype=torch.float64):
    """-> (stages {5, 4, 3, 2: G [B,H,W,96]}, dz [B,H,W,32], dX [B,H,W,64]): G = bf16(a5 dgrad(dY, conv5)); k = 4 .. 2: dz_k = G slice k where F slice k > 0,
    G[:cin_k] = bf16(dgrad(dz_k, conv_k) + G[:cin_k]); dX = bf16(dgrad(dz_1, conv1) + G[:64] + bx dY)."""
    k = [rb(t64(w[0])).to(dtype) for w in ws]
    F, dY = t64(F).to(dtype), t64(dY).to(dtype)
    Gb = _r(a5 * _conv(dY, rot(k[4]), None, dtype))
    stages, dzs = {5: Gb}, [None] * 4
    for j in range(4, 0, -1):
        cin = CIN[j - 1]
        dz = dzs[j - 1] = torch.where(F[..., cin:cin + G] > 0, Gb[..., cin:cin + G], torch.zeros((), dtype=dtype))
        v = _conv(dz, rot(k[j - 1]), None, dtype) + Gb[..., :cin]
        if j > 1:
            Gb = stages[j] = torch.cat([_r(v), Gb[..., cin:]], -1)
        else:
            dX = _r(v + bx * dY)
    return stages, torch.cat(dzs, -1), dX


def differing_share(a, b):
    return float((a.double() != b.double()).double().mean())


# ---------------------------------------------------------------------------------------------------------------- teacher forcing
def forward_checks(ws, F_dev, out_dev, a5, bx, r_in=None):
    """[(label, device value, unrounded fp64 value, fp32 bound)] for esrgan_mixed_ref.check_convs: every growth slice and the block output from the device's own F."""
    k = [rb(t64(w[0])) for w in ws]
    b = [t64(w[1]) for w in ws]
    F = t64(F_dev)
    convs = []
    for i in range(4):
        cin = CIN[i]
        v = torch.relu(conv64(F[..., :cin], k[i], b[i]))
        convs.append((f"F[{i + 1}]", F[..., cin:cin + G], v, conv_bound(F[..., :cin], k[i], b[i])))
    skips = (bx * F[..., :C0],) + ((t64(r_in),) if r_in is not None else ())
    v = a5 * conv64(F, k[4], b[4])
    for s in skips:
        v = v + s
    convs.append(("out", t64(out_dev), v, conv_bound(F, k[4], b[4], a5, skips)))
    return convs


def backward_checks(ws, F, dY, stages_dev, dz_dev, dX_dev, a5, bx):
    """stages_dev: [4,B,H,W,96] as the kernel dumps them (s5, s4, s3, s2; channels >= cin_k of stage k < 5 hold the dz already selected) -> (convs, exact
    [(label, device value, reference to match bitwise)])."""
    k = [rb(t64(w[0])) for w in ws]
    F, dY, dz, dX = t64(F), t64(dY), t64(dz_dev), t64(dX_dev)
    S = {5: t64(stages_dev[0]), 4: t64(stages_dev[1]), 3: t64(stages_dev[2]), 2: t64(stages_dev[3])}
    convs, exact = [], []
    convs.append(("G_s5", S[5], a5 * conv64(dY, rot(k[4])), conv_bound(dY, rot(k[4]), None, a5)))
    for j in range(4, 0, -1):
        cin = CIN[j - 1]
        before = S[j + 1]
        dzj = dz[..., (j - 1) * G:j * G]
        exact.append((f"dz[{j}]", dzj, torch.where(F[..., cin:cin + G] > 0, before[..., cin:cin + G], torch.zeros(()).double())))
        v = conv64(dzj, rot(k[j - 1])) + before[..., :cin]
        if j > 1:
            convs.append((f"G_s{j}[:{cin}]", S[j][..., :cin], v, conv_bound(dzj, rot(k[j - 1]), None, 1.0, (before[..., :cin],))))
            exact.append((f"G_s{j}[{cin}:{cin + G}]", S[j][..., cin:cin + G], dzj))                   # the plane selected in place
            exact.append((f"G_s{j}[{cin + G}:]", S[j][..., cin + G:], before[..., cin + G:]))         # what nobody owns stays
        else:
            convs.append(("dX", dX, v + bx * dY, conv_bound(dzj, rot(k[0]), None, 1.0, (before[..., :C0], bx * dY))))
    return convs, exact


# ---------------------------------------------------------------------------------------------------------------- the trunk at G = 8
def weight_sets(nb=2, seed=4100):
    """esrgan_mixed_ref.weight_sets at growth width 8: he_normal and relu_on."""
    w = init_weights(M.esrgan_g_layers(SCALE, G, nb), scheme="he_normal", seed=seed)
    w["final_conv2"] = ((w["final_conv2"][0] * np.float32(0.05)).astype(np.float32), w["final_conv2"][1])
    for n in w:
        if n.endswith("_f") or n.endswith("_g"):
            w[n] = ((w[n][0] * np.float32(0.25)).astype(np.float32), (w[n][1] * np.float32(0.25)).astype(np.float32))
    on = dict(w)
    for n in trunk_names(nb):
        if not n.endswith("_conv5"):
            on[n] = ((w[n][0] * np.float32(0.25)).astype(np.float32), np.full_like(w[n][1], 0.5))
    return {"he_normal": w, "relu_on": on}


def block_ws(weights, name):
    return [weights[f"{name}_conv{k}"] for k in range(1, 6)]


def trunk_backward(weights, T, dout, nb):
    """esrgan_mixed_ref.trunk_backward at G = 8, block by block through block_backward."""
    g = {}
    dR = T[f"dR_{nb - 1}"] = rb(dout)
    dY = dR
    for bi, d, n, a5, bx in reversed(blocks(nb)):
        F = T[f"F_{bi}_{d}"]
        ws = block_ws(weights, n)
        stages, dz, dX = block_backward(ws, F, dY, a5, bx)
        g[f"{n}_conv5"] = wgrad64(F, dY, a5)
        for j in range(1, 5):
            g[f"{n}_conv{j}"] = wgrad64(F[..., :CIN[j - 1]], dz[..., (j - 1) * G:j * G])
        T[f"dz_{bi}_{d}"], T[f"dX_{bi}_{d}"] = dz, dX
        dY = dX
        if d == 1:
            dR = dY = T[f"drin_{bi}"] = rb(dX + dR)
    return dR, g, T


class MixedTrunk(torch.autograd.Function):
    """The restated trunk inside an fp64 autograd graph (esrgan_mixed_ref.MixedTrunk with this file's backward)."""

    @staticmethod
    def forward(ctx, x0, nb, names, *params):
        w = {n: (params[2 * i].detach(), params[2 * i + 1].detach()) for i, n in enumerate(names)}
        out, T = trunk_forward(w, x0.detach().permute(0, 2, 3, 1), nb)
        ctx.w, ctx.T, ctx.nb, ctx.names = w, T, nb, names
        return out.permute(0, 3, 1, 2).contiguous()

    @staticmethod
    def backward(ctx, dout):
        dx, g, _ = trunk_backward(ctx.w, ctx.T, dout.permute(0, 2, 3, 1).float().double(), ctx.nb)
        return (dx.permute(0, 3, 1, 2), None, None) + tuple(a for n in ctx.names for a in g[n])


def pixel_grads(weights, lr, hr, nb, attention=True, mode="plain"):
    """mean |hr - G(lr)| and its gradients {layer: (dw, db)} in fp64; mode "plain": fp64 autograd of the graph; "mixed": the trunk is the restated contract."""
    p = {n: (t64(k).requires_grad_(), t64(b).requires_grad_()) for n, (k, b) in weights.items()}
    x, t = t64(lr).permute(0, 3, 1, 2), t64(hr).permute(0, 3, 1, 2)
    if mode == "plain":
        y = OT.generator_forward_t(p, x, SCALE, nb, attention=attention)
    else:
        names = trunk_names(nb)
        y = generator_t(p, x, nb, attention, lambda x0: MixedTrunk.apply(x0, nb, names, *[a for n in names for a in p[n]]))
    loss = (t - y).abs().mean()
    loss.backward()
    return float(loss.detach()), {n: (k.grad, b.grad) for n, (k, b) in p.items() if k.grad is not None}
