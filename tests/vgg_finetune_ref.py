"""Reference for FineTunedVGG16's fine_tune_base mode (sr355/vgg_train.py): torch autograd over the trained tail of the VGG16 base (3x3 SAME
convs + ReLU, 2x2 max-pools), GlobalAveragePooling2D, Dropout with GIVEN keep masks, Dense 256 ReLU, Dropout, Dense softmax, and the loss
mean sparse categorical cross-entropy (probabilities clipped to [1e-7, 1 - 1e-7]) + l2_reg * sum(dense kernel^2) -- in fp64, or in fp32 to
measure what fp32 arithmetic alone does to the same numbers.

`pin` takes the ReLU branches and the max-pool selections of ANOTHER evaluation of the same graph (oracle/train.py's _masked_act practice):
two correct forward passes that differ in their last bits disagree about a branch where a pre-activation is within rounding of zero, or
about a window's maximum where two entries nearly tie, and each such element moves a gradient by a whole unit; pinned, the comparison is
about arithmetic.  The test that pins also counts how many branches differ from the reference's own, so a wrong forward cannot hide.

Tensors are NHWC NumPy arrays at the interface; kernels are Keras HWIO.
"""
import numpy as np
import torch
import torch.nn.functional as F

BASE = ("input_1", "block1_conv1", "block1_conv2", "block1_pool", "block2_conv1", "block2_conv2", "block2_pool", "block3_conv1", "block3_conv2",
        "block3_conv3", "block3_pool", "block4_conv1", "block4_conv2", "block4_conv3", "block4_pool", "block5_conv1", "block5_conv2",
        "block5_conv3", "block5_pool")
_WIDTH = {"block1": 64, "block2": 128, "block3": 256, "block4": 512, "block5": 512}


def vgg16_layer_shapes(num_classes=2):
    """[(layer, kernel shape)] in the inference model's parameter order (Model.layer_shapes() without a device)."""
    out, cin = [], 3
    for name in BASE:
        if "_conv" in name:
            cout = _WIDTH[name.split("_")[0]]
            out.append((name, (3, 3, cin, cout)))
            cin = cout
    return out + [("dense", (512, 256)), ("predictions", (256, num_classes))]


def seeded_weights(num_classes=2, seed=4000):
    """FineTunedVGG16.setup_model's seeded he-normal initialisation, without a device."""
    from sr355.weights import init_weights
    return init_weights(vgg16_layer_shapes(num_classes), scheme="he_normal", seed=seed)


def tail_of(first_conv):
    return list(BASE[BASE.index(first_conv):])


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def _conv(x, k, b):
    """x NCHW, k HWIO -> the 3x3 SAME stride-1 conv's pre-activation."""
    return F.conv2d(x, k.permute(3, 2, 0, 1), b, padding=1)


def _windows(x):
    """NCHW -> [B,C,h,w,4]: the 2x2 windows (floor) in the order (0,0) (0,1) (1,0) (1,1)."""
    h, w = x.shape[2] // 2, x.shape[3] // 2
    return torch.stack([x[:, :, 0:2 * h:2, 0:2 * w:2], x[:, :, 0:2 * h:2, 1:2 * w:2], x[:, :, 1:2 * h:2, 0:2 * w:2], x[:, :, 1:2 * h:2, 1:2 * w:2]], -1)


def pool_selection(a_nhwc):
    """ReLU output NHWC -> (index int64 [B,h,w,C] of each window's first maximum in the order above, bool: that maximum is positive)."""
    win = _windows(torch.as_tensor(np.asarray(a_nhwc)).permute(0, 3, 1, 2))
    m = win.max(-1, keepdim=True).values
    eq = win == m
    first = eq & (eq.cumsum(-1) == 1)
    return first.to(torch.int64).argmax(-1).permute(0, 2, 3, 1).numpy(), (m[..., 0] > 0).permute(0, 2, 3, 1).numpy()


def _pool(x, sel):
    """Max-pool whose gradient goes to entry `sel` (int64 [B,C,h,w]) of every window."""
    return torch.gather(_windows(x), -1, sel.unsqueeze(-1))[..., 0]


def forward_frozen(x_nhwc, weights, layers, dtype=torch.float64):
    """The frozen layers `layers` (names of BASE, in order) on x NHWC -> NHWC NumPy in `dtype`."""
    with torch.no_grad():
        x = _t(x_nhwc, dtype).permute(0, 3, 1, 2)
        for name in layers:
            if name.endswith("_pool"):
                x = F.max_pool2d(x, 2)
            elif "_conv" in name:
                x = torch.relu(_conv(x, _t(weights[name][0], dtype), _t(weights[name][1], dtype)))
        return x.permute(0, 2, 3, 1).contiguous().numpy()


def tail_head(x_nhwc, layers, weights, labels, keep0=None, keep1=None, keep_scale=1.0, l2_reg=0.0, dtype=torch.float64, pin=None, grad=True):
    """One evaluation of tail + head.  layers: tail_of(first trained conv); weights {layer: (kernel, bias)}; keep0 [n,512] / keep1 [n,256] 0/1
    keep masks or None.  pin: {"relu": {conv: bool NHWC}, "sel": {pool: int64 [B,h,w,C]}} from another evaluation (missing entries: own).
    -> dict: loss (without and with the l2 term: "cce", "loss"), "acc", "probs", "acts" {conv: ReLU output NHWC}, "relu" {conv: bool NHWC},
    "sel" {pool: (index, positive)}, "grads" {layer: (dk, db)} for every conv of the tail and the two Dense layers."""
    pin = pin or {}
    names = [n for n in layers if "_conv" in n] + ["dense", "predictions"]
    p = {n: [_t(weights[n][0], dtype).clone().requires_grad_(grad), _t(weights[n][1], dtype).clone().requires_grad_(grad)] for n in names}
    x = _t(x_nhwc, dtype).permute(0, 3, 1, 2)
    out = {"acts": {}, "relu": {}, "sel": {}}
    for name in layers:
        if name.endswith("_pool"):
            own, positive = pool_selection(x.detach().permute(0, 2, 3, 1).numpy())
            out["sel"][name] = (own, positive)
            sel = pin.get("sel", {}).get(name, own)
            x = _pool(x, torch.as_tensor(np.asarray(sel), dtype=torch.int64).permute(0, 3, 1, 2))
        else:
            z = _conv(x, *p[name])
            own = (z.detach() > 0).permute(0, 2, 3, 1).numpy()
            out["relu"][name] = own
            mask = pin.get("relu", {}).get(name, own)
            x = z * _t(mask, dtype).permute(0, 3, 1, 2)
            out["acts"][name] = x.detach().permute(0, 2, 3, 1).numpy()
    g = x.mean(dim=(2, 3))
    x0 = g if keep0 is None else g * (_t(keep0, dtype) * keep_scale)
    a1 = torch.relu(x0 @ p["dense"][0] + p["dense"][1])
    x1 = a1 if keep1 is None else a1 * (_t(keep1, dtype) * keep_scale)
    probs = torch.softmax(x1 @ p["predictions"][0] + p["predictions"][1], dim=1)
    y = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    py = probs[torch.arange(len(y)), y]
    cce = -torch.log(torch.clamp(py, 1e-7, 1.0 - 1e-7)).mean()
    loss = cce + l2_reg * (p["dense"][0] ** 2).sum()
    out.update(cce=float(cce.detach()), loss=float(loss.detach()), probs=probs.detach().numpy(), feats=g.detach().numpy(),
               acc=float((probs.argmax(1) == y).double().mean()))
    if grad:
        loss.backward()
        out["grads"] = {n: (k.grad.numpy(), b.grad.numpy()) for n, (k, b) in p.items()}
    return out


def tail_conv_grad_numpy(x, dz):
    """The direct fp64 tap sum of a 3x3 SAME conv's kernel gradient: dW[ky,kx,ci,co] = sum over b, y, x of x[b, y+ky-1, x+kx-1, ci] dz[b,y,x,co]."""
    x, dz = np.asarray(x, np.float64), np.asarray(dz, np.float64)
    B, H, W, _ = x.shape
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    dw = np.zeros((3, 3, x.shape[3], dz.shape[3]))
    for ky in range(3):
        for kx in range(3):
            for b in range(B):
                for yy in range(H):
                    for xx in range(W):
                        dw[ky, kx] += np.outer(xp[b, yy + ky, xx + kx], dz[b, yy, xx])
    return dw


class _Adam:
    """keras Adam (dense update, epsilon 1e-7) on torch tensors of one dtype."""

    def __init__(self, params, lr):
        self.lr, self.t = lr, 0
        self.m = {n: [torch.zeros_like(a) for a in pair] for n, pair in params.items()}
        self.v = {n: [torch.zeros_like(a) for a in pair] for n, pair in params.items()}

    def apply(self, params, grads):
        self.t += 1
        lr_t = self.lr * np.sqrt(1.0 - 0.999 ** self.t) / (1.0 - 0.9 ** self.t)
        for n, pair in params.items():
            for s in (0, 1):
                g = torch.as_tensor(grads[n][s], dtype=pair[s].dtype)
                self.m[n][s] = 0.9 * self.m[n][s] + 0.1 * g
                self.v[n][s] = 0.999 * self.v[n][s] + 0.001 * g * g
                pair[s] -= lr_t * self.m[n][s] / (torch.sqrt(self.v[n][s]) + 1e-7)


def fit(X, y, Xv, yv, weights, first_conv, learning_rate=1e-3, l2_reg=0.0, batch_size=4, epochs=2, seed=42, dtype=torch.float64):
    """FineTunedVGG16.fit with fine_tune_base, without augmentation or dropout, as Keras would run it: per epoch a permutation from
    default_rng(seed), batches in that order, one Adam over tail convs + head, the epoch's loss / accuracy as sample-weighted means of the
    batches' values before their update, validation with the epoch's final weights.  The frozen prefix is evaluated once, in `dtype`.
    -> (history dict, final weights {layer: (kernel, bias)} of the trained layers)."""
    layers = tail_of(first_conv)
    frozen = list(BASE[:BASE.index(first_conv)])
    P, Pv = forward_frozen(X, weights, frozen, dtype), forward_frozen(Xv, weights, frozen, dtype)
    names = [n for n in layers if "_conv" in n] + ["dense", "predictions"]
    w = {n: [_t(weights[n][0], dtype).clone(), _t(weights[n][1], dtype).clone()] for n in names}
    opt = _Adam(w, learning_rate)
    rng = np.random.default_rng(seed)
    y, yv = np.asarray(y), np.asarray(yv)
    hist = {k: [] for k in ("loss", "accuracy", "val_loss", "val_accuracy", "lr")}
    for _ in range(epochs):
        order = rng.permutation(len(X))
        tot = np.zeros(2)
        for i in range(0, len(order), batch_size):
            idx = order[i:i + batch_size]
            cur = {n: (a.numpy(), b.numpy()) for n, (a, b) in w.items()}
            r = tail_head(P[idx], layers, cur, y[idx], l2_reg=l2_reg, dtype=dtype)
            tot += [r["loss"] * len(idx), r["acc"] * len(idx)]
            opt.apply(w, r["grads"])
        cur = {n: (a.numpy(), b.numpy()) for n, (a, b) in w.items()}
        rv = tail_head(Pv, layers, cur, yv, l2_reg=l2_reg, dtype=dtype, grad=False)
        for k, v in zip(hist, (tot[0] / len(X), tot[1] / len(X), rv["loss"], rv["acc"], learning_rate)):
            hist[k].append(float(v))
    return hist, {n: (a.numpy().copy(), b.numpy().copy()) for n, (a, b) in w.items()}


# ---- the cases the CPU and the GPU tests share (same seeds: the CPU test bounds the reference's own fp32 error on what the GPU test runs)
STEP_CASES = [(4, 128), (6, 128), (4, 32), (6, 32)]              # (train_last_n_layers, input size)
FIRST_CONV = {4: "block5_conv1", 6: "block4_conv3"}


def step_inputs(n_last, hw, B=2):
    """-> (images [B,hw,hw,3], labels, keep0 uint8 [B,512], keep1 uint8 [B,256]) of the one-step tests."""
    rng = np.random.default_rng(1000 * n_last + hw)
    X = rng.uniform(0, 1, (B, hw, hw, 3)).astype(np.float32)
    y = rng.integers(0, 2, B)
    return X, y, (rng.random((B, 512)) < 0.8).astype(np.uint8), (rng.random((B, 256)) < 0.8).astype(np.uint8)


def fit_inputs(hw=32):
    """-> (X [8,...], y, Xv [4,...], yv) of the two-epoch fit: 2 batches of 4."""
    rng = np.random.default_rng(77)
    return (rng.uniform(0, 1, (8, hw, hw, 3)).astype(np.float32), rng.integers(0, 2, 8),
            rng.uniform(0, 1, (4, hw, hw, 3)).astype(np.float32), rng.integers(0, 2, 4))


FIT = dict(first_conv="block5_conv1", learning_rate=1e-4, l2_reg=1e-3, batch_size=4, epochs=2, seed=5)
