"""Restated references for the bf16 pieces of ESRGAN's VGG19 perceptual branch (include/sr355.h: sr_conv3x3_small_bf16), torch-CPU in fp64 on
the helpers of tests/edsr_mixed_ref.py.  The contract: fp32 kernels rounded to bf16 once, bf16 tensors between kernels, every stored tensor rounded once after an
fp64 epilogue, selects decided on the stored bits.

  SHAPES            the (B, H, W, Cin, Cout) the small-image conv is tested on
  conv_operands     ReLU'd N(0,1) images, a he-normal kernel, a small bias and a mask that carries every special bit pattern
  conv_small_ref    the unrounded fp64 value and the fp32 bound of one call
  positive_bits     the predicate `> 0` read off bf16 bits, as sr_relu_bwd_bf16 reads it
  check_conv        the per-element bound and the share cap of DESIGN.md 3.26, the share taken over the NON-ZERO elements
"""
import numpy as np
import torch

from edsr_mixed_ref import bf16_bits, conv64, conv_bound, one_minus_cos, rb, rel_l2, rot, t64  # noqa: F401  (re-exported for the tests)

BF16 = torch.bfloat16

# (B, H, W, Cin, Cout): a ragged 45-pixel tile over five images; VGG19's blocks 5, 4, 3; one K chunk; H != W with 3 and 2 chunks; 1 x 1 images, where every tap
# but the centre is padding; one image larger than a tile
SHAPES = [(5, 3, 3, 512, 512), (3, 6, 6, 512, 512), (2, 12, 12, 256, 256), (2, 12, 12, 128, 256), (5, 3, 3, 32, 32), (3, 5, 7, 96, 64), (7, 1, 1, 64, 32),
          (1, 12, 12, 32, 32)]

SPECIAL_BITS = [0x0000, -0x8000, 0x0001, -0x7FFF, 0x7F80, -0x0080, 0x7FC0, 0x007F]      # +0 -0 +/-subnormal +/-inf NaN subnormal


def shape_id(s):
    return "x".join(map(str, s))


def conv_operands(shape, rot_, seed=0):
    """-> (x bf16 [B,H,W,Cin] = relu(N(0,1)), w fp32 as the call takes it, bias fp32 [Cout], mask bf16 [B,H,W,Cout])."""
    B, H, W, cin, cout = shape
    rng = np.random.default_rng(1000 * seed + 7 * sum(shape) + int(rot_))
    x = torch.from_numpy(np.maximum(rng.standard_normal((B, H, W, cin)), 0.0).astype(np.float32)).to(BF16)
    wshape = (3, 3, cout, cin) if rot_ else (3, 3, cin, cout)
    w = (rng.standard_normal(wshape) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = rng.uniform(-0.05, 0.05, cout).astype(np.float32)
    mask = torch.from_numpy(rng.standard_normal((B, H, W, cout)).astype(np.float32)).to(BF16)
    mask.view(torch.int16)[0, 0, 0, :8] = torch.tensor(SPECIAL_BITS, dtype=torch.int16)
    return x, w, b, mask


def conv_small_ref(x, w, b, rot_, act):
    """-> (v, bound): the unrounded fp64 value of bf16(act(conv(x, bf16(w)) + b)) from the stored x, and (9 Cin + 2) 2^-24 S."""
    kk = rb(t64(w))
    if rot_:
        kk = rot(kk)
    bb = None if b is None else t64(b)
    v = conv64(t64(x), kk, bb)
    if act == "relu":
        v = torch.relu(v)
    return v, conv_bound(t64(x), kk, bb)


def positive_bits(t):
    """bf16 tensor -> bool: sign clear, not zero, not NaN (+inf counts)."""
    b = t.detach().cpu().contiguous().view(torch.int16).int()
    return (b > 0) & (b <= 0x7F80)


def check_conv(label, got, v, bound):
    """got: fp64 of the stored bf16.  Within 2^-8 |v| + bound of v everywhere; of the elements whose rounded reference is not zero at most 1e-2 differ from it,
    each by one bf16 step (steps counted where |v| >= 4 bound, so that the fp32 error cannot carry a value across zero).  Prints, then asserts."""
    bits = lambda a: a.float().bfloat16().view(torch.int16).int()
    ref = rb(v)
    excess = float(((got - v).abs() - (2.0 ** -8 * v.abs() + bound)).max())
    nz = ref != 0
    differ = (got != ref) & nz
    share = float(differ.sum()) / max(int(nz.sum()), 1)
    counted = differ & (v.abs() >= 4 * bound)
    step = int((bits(got) - bits(ref)).abs()[counted].max()) if bool(counted.any()) else 0
    print(f"{label}: worst |got - v| - bound {excess:.3e}; {share:.2e} of the non-zero elements differ from the rounded reference, by at most {step} step")
    assert excess <= 0.0 and share <= 1e-2 and step <= 1, label


# ---------------------------------------------------------------------------------------------------------------- the branch, restated
# perceptual_dtype="bf16" (sr355.gan_train.PerceptualBf16): one forward over [fake | hr], the loss, one backward over the fake half.
#   preprocess64 / hi_lo     caffe preprocessing in fp64 from the fp32 images, and its bf16 hi + lo pair
#   pool64 / pool_bwd64      MaxPooling2D(2,2) VALID and its gradient with the first-winner tie rule and the fused ReLU select
#   mse_grad_ref             the loss and its bf16 gradient with the fixed fp32 scale
#   branch_ref               the contract, restated -> (perc, d perc / d fake, tape)
#   branch_autograd          plain fp64 autograd of the unrounded network
#   teacher_forced           every tensor of a device tape recomputed from the device's own stored input of that stage
CAFFE_MEANS = (103.939, 116.779, 123.68)                      # BGR, as the fp32 constants the kernels hold


def vgg_weights(seed=6000):
    """Real VGG19 widths, seeded he-normal; block1_conv1 times 0.05 (its inputs are +-128 after caffe preprocessing: the features stay O(1))."""
    from oracle import models as M
    from sr355.weights import init_weights
    w = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=seed)
    return {n: ((k * np.float32(0.05)).astype(np.float32) if n == "block1_conv1" else k, b) for n, (k, b) in w.items()}


def images(B, n, seed):
    """(hr, fake) fp32 [B,n,n,3] in [-1,1]: smooth random images and a noisy copy."""
    from sr355.synth import make_pairs
    _, hr = make_pairs(B, n // 2, n // 2, 2, seed)
    hr = (hr * 2.0 - 1.0).astype(np.float32)
    rng = np.random.default_rng(seed)
    fake = np.clip(hr + 0.2 * rng.standard_normal(hr.shape), -1.0, 1.0).astype(np.float32)
    return hr, fake


def preprocess64(x):
    """fp64 tensor of the fp32 RGB image in [-1,1] -> v in BGR order, fp64."""
    means = torch.tensor(np.asarray(CAFFE_MEANS, np.float32).astype(np.float64))
    return (x.flip(-1) + 1.0) * 127.5 - means


def hi_lo(v):
    hi = rb(v)
    return torch.cat([hi, rb(v - hi)], dim=-1)


def _windows(x):
    B, H, W, C = x.shape
    oh, ow = H // 2, W // 2
    x = x[:, :2 * oh, :2 * ow]
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]])      # (0,0) (0,1) (1,0) (1,1): the kernels' order


def pool64(x):
    return _windows(x).max(dim=0).values


def pool_bwd64(x, dy):
    """dy at the FIRST element of each window that equals its maximum, and only where that element is positive; zero elsewhere and in a dropped row / column."""
    w = _windows(x)
    eq = w == w.max(dim=0).values
    first = eq & (eq.long().cumsum(0) == 1)
    g = torch.where(first & (w > 0), dy.unsqueeze(0).expand_as(w), torch.zeros(()).double())
    dx = torch.zeros_like(x)
    oh, ow = x.shape[1] // 2, x.shape[2] // 2
    for i, (a, b) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        dx[:, a:2 * oh:2, b:2 * ow:2] = g[i]
    return dx


def mse_grad_ref(feats):
    """feats fp64 of bf16 [2B,...] -> (perc fp64, dff fp64 of bf16): fp32(2 / n) * fp32(ff - fr), each rounded on its own, then to bf16; +0 where ff <= 0."""
    B = feats.shape[0] // 2
    ff, fr = feats[:B], feats[B:]
    d = ff - fr
    c = torch.tensor(np.float32(2.0 / d.numel()))
    g = (c * (ff.float() - fr.float())).bfloat16().double()
    return (d * d).mean(), torch.where(ff > 0, g, torch.zeros(()).double())


def _routes(H, W, B=None):
    from sr355.gan_train import perceptual_routes
    return perceptual_routes(H, W, B)


def branch_ref(weights, hr, fake):
    """The contract, restated -> (perc fp64, d perc / d fake fp64 holding fp32 values, tape {name: fp64 tensor})."""
    B, H, W, _ = fake.shape
    routes = _routes(H, W)
    T = {}
    h = T["pre"] = hi_lo(preprocess64(torch.cat([t64(fake), t64(hr)])))
    acts = []
    for i, (name, _, _, _, _, _, pooled, _) in enumerate(routes):
        k, b = rb(t64(weights[name][0])), t64(weights[name][1])
        if i == 0:
            k = torch.cat([k, k], dim=2)
        h = T[name] = rb(torch.relu(conv64(h, k, b)))
        acts.append(h)
        if pooled:
            h = T[name + "_pool"] = pool64(h)
    perc, g = mse_grad_ref(h)
    T["d_" + routes[-1][0]] = g
    zero = torch.zeros(()).double()
    for i in range(len(routes) - 1, 0, -1):
        name, prev, prev_pooled = routes[i][0], routes[i - 1][0], routes[i - 1][6]
        a_prev = acts[i - 1][:B]
        g = rb(conv64(g, rot(rb(t64(weights[name][0])))))
        if prev_pooled:
            T["d_" + prev + "_pool"] = g
            g = pool_bwd64(a_prev, g)
        else:
            g = torch.where(a_prev > 0, g, zero)
        T["d_" + prev] = g
    dv = T["d_pre"] = rb(conv64(g, rot(rb(t64(weights["block1_conv1"][0])))))
    return perc, (torch.tensor(np.float32(127.5)) * dv.flip(-1).float()).double(), T


def branch_autograd(weights, hr, fake):
    """Plain fp64 autograd on the unrounded weights and images -> (perc, d perc / d fake, ff, fr)."""
    x = t64(fake).requires_grad_()

    def feats(img):
        h = preprocess64(img)
        for name, _, _, _, _, _, pooled, _ in _routes(*fake.shape[1:3]):
            h = torch.relu(conv64(h, t64(weights[name][0]), t64(weights[name][1])))
            if pooled:
                h = pool64(h)
        return h
    ff, fr = feats(x), feats(t64(hr))
    perc = ((ff - fr) ** 2).mean()
    perc.backward()
    return perc.detach(), x.grad, ff.detach(), fr.detach()


def perc_bound(weights, hr, fake, ref_tape):
    """What bf16 itself may move perc by, to first order and without cancellation: perc = mean(d^2), d = ff - fr, so |delta perc| / perc <= 2 |delta d| / |d| <=
    2 (|ff_ref - ff_64| + |fr_ref - fr_64|) / |ff_64 - fr_64| with the restated reference's own feature errors.  Two realisations of the one contract differ by
    less than either differs from fp64: they round alike except where the fp32 summation order carries a value across a rounding boundary (at most 1e-2 of a
    tensor's elements, by 2^-8, against every element by up to 2^-9)."""
    _, _, ff, fr = branch_autograd(weights, hr, fake)
    B = fake.shape[0]
    last = ref_tape[_routes(*fake.shape[1:3])[-1][0]]
    return 2.0 * float((last[:B] - ff).norm() + (last[B:] - fr).norm()) / float((ff - fr).norm())


def teacher_forced(tape, weights, B, H, W):
    """tape: {name: fp64 of the device's stored tensor} -> (convs [(label, got, v, bound)] for check_conv, exact [(label, got, want)] for torch.equal)."""
    routes = _routes(H, W, B)
    convs, exact = [], []
    zero = torch.zeros(()).double()
    h = tape["pre"]
    for i, (name, _, _, _, _, _, pooled, _) in enumerate(routes):
        k, b = rb(t64(weights[name][0])), t64(weights[name][1])
        if i == 0:
            k = torch.cat([k, k], dim=2)
        convs.append((name, tape[name], torch.relu(conv64(h, k, b)), conv_bound(h, k, b)))
        h = tape[name]
        if pooled:
            exact.append((name + "_pool", tape[name + "_pool"], pool64(h)))
            h = tape[name + "_pool"]
    last = routes[-1][0]
    exact.append(("d_" + last, tape["d_" + last], mse_grad_ref(tape[last])[1]))
    for i in range(len(routes) - 1, 0, -1):
        name, prev, prev_pooled, route = routes[i][0], routes[i - 1][0], routes[i - 1][6], routes[i][7]
        a_prev = tape[prev][:B]
        kk = rot(rb(t64(weights[name][0])))
        g = tape["d_" + name]
        v, bound = conv64(g, kk), conv_bound(g, kk, None)
        if prev_pooled:
            convs.append(("d_" + prev + "_pool", tape["d_" + prev + "_pool"], v, bound))
            exact.append(("d_" + prev, tape["d_" + prev], pool_bwd64(a_prev, tape["d_" + prev + "_pool"])))
        elif route == "small":                                   # the select is fused: the stored tensor is the masked one
            keep = a_prev > 0
            convs.append(("d_" + prev, tape["d_" + prev], torch.where(keep, v, zero), torch.where(keep, bound, zero)))
        else:
            convs.append(("dx_" + name, tape["dx_" + name], v, bound))
            exact.append(("d_" + prev, tape["d_" + prev], torch.where(a_prev > 0, tape["dx_" + name], zero)))
    kk = rot(rb(t64(weights["block1_conv1"][0])))
    g = tape["d_block1_conv1"]
    convs.append(("d_pre", tape["d_pre"], conv64(g, kk), conv_bound(g, kk, None)))
    return convs, exact
