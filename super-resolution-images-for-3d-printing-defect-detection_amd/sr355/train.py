"""Keras `model.fit` for the SRCNN and EDSR graphs on MI355X (reference: SRCNN_model.py:55-98, EDSR_model.py:127-176).

What the reference delegates to Keras is restated here as host orchestration over the C ABI: forward convs (the MFMA kernels, fp32 as
the reference trains), loss = mean_squared_error, the backward pass layer by layer -- input gradients are the SAME forward kernels on
180-degree-rotated, channel-swapped weights, weight / bias gradients the fp32-MFMA wgrad kernel, activations / clip / depth_to_space
their element-wise or permutation inverses (csrc/train_ops.hip) -- and Adam exactly as Keras applies it (optimizer_v2 dense update:
lr_t = lr sqrt(1 - b2^t) / (1 - b1^t); var -= lr_t m / (sqrt(v) + eps); EDSR: per-variable clip-by-norm 1.0, eps 1e-8), plus the two
callbacks that change the result (EarlyStopping with restore_best_weights, ReduceLROnPlateau) and the two that only record
(epoch time, device memory).  Two places for the update, chosen by the model's `update` keyword: "host" (the default) keeps optimiser state and
master weights on the host (28 931 / 1.37 M parameters) -- every step uploads the weights into a fresh ParamBucket, downloads every gradient and
runs `Adam.apply` in NumPy; "device" keeps ONE ParamBucket and a DeviceAdam for the whole fit -- gradients are gathered into a flat bucket,
clipped per variable (EDSR, sr_clip_by_norm_bucket) and applied by sr_adam, and the host reads one block of per-step statistics per epoch plus
the weights for validation and the callbacks.  The training data is either the loader's host arrays, indexed and uploaded per step, or the
`.X` / `.Y` views of a device-resident sr355.patches.PatchPairs, from which each step's batch is cut by one launch; the batches are the same
bits either way.
"""
import time

import numpy as np
import torch

from . import _lib as L


def _rot(w):
    """Kernel of the input-gradient conv: rotate by 180 degrees, swap the channel axes (HWIO -> HW O I)."""
    return np.ascontiguousarray(w[::-1, ::-1].transpose(0, 1, 3, 2))


class ParamBucket:
    """A parameter dict {layer: (kernel, bias)} on the device as ONE flat fp32 tensor `flat` in parameter order -- every layer's kernel then
    its bias, in dict order -- with views of it per array: `dev[layer][slot]`, and `devcache` (id(host array) -> (host array, view)) for a
    Tape.  The host arrays `arrays` are views of one host buffer; whoever writes `flat` sets `stale`, and `host()` downloads it on the next
    read.  conv / dgrad run on the views through sr_conv2d_dev (packed into MFMA fragment order by a device kernel, no host re-pack per call)."""

    def __init__(self, ctx, weights):
        self.ctx = ctx
        weights = {n: [np.asarray(a, np.float32) for a in pair] for n, pair in weights.items()}
        self.shapes = {n: [a.shape for a in pair] for n, pair in weights.items()}
        self._hflat = self.flatten(weights)
        self.flat = ctx.to_device(self._hflat)
        self.arrays, self.dev = self.split(self._hflat), self.split(self.flat)
        self.devcache = {id(a): (a, v) for n in self.dev for a, v in zip(self.arrays[n], self.dev[n])}
        self.stale = False

    def flatten(self, weights):
        """{layer: (kernel, bias)} with this bucket's layer names and shapes -> one fp32 host array in parameter order."""
        if set(weights) != set(self.shapes):
            raise ValueError("parameter dict: layer names differ from the bucket's")
        parts = []
        for n, shapes in self.shapes.items():
            for a, shape in zip(weights[n], shapes):
                a = np.asarray(a, np.float32)
                if a.shape != shape:
                    raise ValueError(f"{n}: shape {a.shape} != {shape}")
                parts.append(a.ravel())
        return np.concatenate(parts)

    def split(self, flat):
        """A flat host array or device tensor in parameter order -> {layer: (kernel, bias)} of views into it."""
        out, o = {}, 0
        for n, shapes in self.shapes.items():
            pair = []
            for shape in shapes:
                size = int(np.prod(shape))
                pair.append(flat[o:o + size].reshape(shape))
                o += size
            out[n] = tuple(pair)
        return out

    def host(self):
        """`arrays`, refreshed from the device first when `flat` has moved on."""
        if self.stale:
            self._hflat[:] = self.flat.cpu().numpy()
            self.stale = False
        return self.arrays

    def load(self, weights):
        """New values for every array (same layer names and shapes), on the host and on the device."""
        self._hflat[:] = self.flatten(weights)
        self.flat.copy_(self.ctx.to_device(self._hflat))
        self.stale = False

    def gather(self, grads):
        """{layer: [dk, db]} device tensors -> one flat device tensor in parameter order (zeros where the loss does not reach a variable:
        its moments and value then stay put, as Keras' skipping of None gradients leaves them)."""
        if isinstance(grads, FlatGrads):                             # written in place into views of one flat tensor: nothing to gather
            return grads.flat
        parts = []
        for n, views in self.dev.items():
            g = grads.get(n)
            for s, v in enumerate(views):
                parts.append(torch.zeros(v.numel(), dtype=torch.float32, device=v.device) if g is None or g[s] is None else g[s].reshape(-1))
        return torch.cat(parts)

    def conv(self, x, name, **kw):
        k, b = self.dev[name]
        return self.ctx.conv2d_dev(x, k, b, k.shape[3], **kw)

    def dgrad(self, dy, name):
        k = self.dev[name][0]
        return self.ctx.conv2d_dev(dy, k, None, k.shape[2], rot=True)


class FlatGrads(dict):
    """{layer: (dw, db)} whose tensors are the views of ONE flat fp32 device tensor `flat` in a ParamBucket's parameter order: the kernels wrote the
    gradients straight into the bucket the optimiser reads (ParamBucket.gather hands `flat` on)."""

    def __init__(self, bucket):
        self.flat = torch.zeros_like(bucket.flat)                   # (zeros where no kernel writes: a variable the loss does not reach)
        super().__init__(bucket.split(self.flat))


def as_bucket(ctx, w):
    """A *_loss_and_grads weight argument -> ParamBucket: the caller's own (device update: one bucket for the whole fit) or a fresh upload of a
    host weight dict."""
    return w if isinstance(w, ParamBucket) else ParamBucket(ctx, w)


def _next_lr_t(opt):
    """Advance an Adam's step count -> that step's bias-corrected rate lr sqrt(1 - b2^t) / (1 - b1^t) in fp32 (both Adams below)."""
    opt.t += 1
    return np.float32(opt.lr * np.sqrt(1.0 - opt.b2 ** opt.t) / (1.0 - opt.b1 ** opt.t))


class Adam:
    """keras.optimizers.Adam (TF 2.10 optimizer_v2), dense update, fp32 state."""

    def __init__(self, weights, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None):
        self.lr, self.b1, self.b2, self.eps, self.clipnorm = float(learning_rate), beta_1, beta_2, epsilon, clipnorm
        self.t = 0
        self.scales_log = None          # a list: every apply() appends its clip factors, fp32 [variables] in parameter order (1 = not clipped)
        self.m = {n: [np.zeros_like(k), np.zeros_like(b)] for n, (k, b) in weights.items()}
        self.v = {n: [np.zeros_like(k), np.zeros_like(b)] for n, (k, b) in weights.items()}

    def apply(self, weights, grads):
        lr_t = _next_lr_t(self)
        out, scales = {}, []
        for n, (k, b) in weights.items():
            if n not in grads:                                     # a variable the loss does not reach: Keras skips None gradients
                out[n] = (k, b)
                scales += [np.float32(1.0)] * 2
                continue
            new = []
            for slot, (var, g) in enumerate(((k, grads[n][0]), (b, grads[n][1]))):
                g = np.asarray(g, np.float32)
                scales.append(np.float32(1.0))
                if self.clipnorm is not None:                      # tf.clip_by_norm per variable
                    nrm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
                    if nrm > self.clipnorm:
                        scales[-1] = np.float32(self.clipnorm / nrm)
                        g = g * np.float32(self.clipnorm / nrm)
                m = self.m[n][slot] = np.float32(self.b1) * self.m[n][slot] + np.float32(1.0 - self.b1) * g
                v = self.v[n][slot] = np.float32(self.b2) * self.v[n][slot] + np.float32(1.0 - self.b2) * g * g
                new.append((var - lr_t * m / (np.sqrt(v) + np.float32(self.eps))).astype(np.float32))
            out[n] = (new[0], new[1])
        if self.scales_log is not None:
            self.scales_log.append(np.array(scales, np.float32))
        return out


class DeviceAdam:
    """The same optimiser with its state on the device: parameters, both moments and the gradient are flat fp32 buckets and one fused kernel
    (sr_adam) updates them in place -- no parameter leaves the GPU between steps.  Bit for bit the update of `Adam.apply` on the same numbers
    (the kernel rounds every operation separately, in NumPy's order).  clipnorm with clip_table (Context.clip_table of the parameters' bucket):
    tf.clip_by_norm per variable first, in place in flat_grads (sr_clip_by_norm_bucket; its fp64 norm is summed in another order than NumPy's, so a
    clip factor may differ from the host's by one fp32 ulp)."""

    def __init__(self, ctx, flat_weights, learning_rate=1e-3, beta_1=0.9, beta_2=0.999, epsilon=1e-7, clipnorm=None, clip_table=None):
        self.ctx, self.lr, self.b1, self.b2, self.eps = ctx, float(learning_rate), beta_1, beta_2, epsilon
        self.t = 0
        self.m, self.v = torch.zeros_like(flat_weights), torch.zeros_like(flat_weights)
        if (clipnorm is None) != (clip_table is None):
            raise ValueError("DeviceAdam: clipnorm and clip_table go together")
        self.clipnorm, self.clip_table = clipnorm, clip_table
        self.scales_log = None          # a list: every apply() appends its clip factors, fp32 device [variables] (no host read)

    def apply(self, flat_weights, flat_grads, grad_scale=1.0):
        if self.clipnorm is not None:
            scales = self.ctx.clip_by_norm_bucket(flat_grads, self.clip_table, self.clipnorm)
            if self.scales_log is not None:
                self.scales_log.append(scales)
        self.ctx.adam_step(flat_weights, flat_grads, self.m, self.v, _next_lr_t(self), self.b1, self.b2, self.eps, grad_scale)


# ---------------------------------------------------------------------------------------------------------------- graphs
def srcnn_loss_and_grads(ctx, w, x, t):
    """SRCNN_model.py:48-53 + mean_squared_error.  w: host weight dict, or the fit's ParamBucket.  x, t device fp32 [B,H,W,3].
    -> (prediction, loss tensor [1], {layer: (dw, db)})."""
    dw = as_bucket(ctx, w)
    a1 = dw.conv(x, "conv2d", act="relu")
    a2 = dw.conv(a1, "conv2d_1", act="relu")
    y = dw.conv(a2, "conv2d_2")
    loss = ctx.mse(t, y)
    g = {}
    dy = ctx.eltwise(L.ELT_AXPBY, y, t, 2.0 / y.numel(), -2.0 / y.numel())
    g["conv2d_2"] = ctx.conv2d_wgrad(a2, dy, 5)
    d2 = ctx.eltwise(L.ELT_RELU_BWD, dw.dgrad(dy, "conv2d_2"), a2)
    g["conv2d_1"] = ctx.conv2d_wgrad(a1, d2, 1)
    d1 = ctx.eltwise(L.ELT_RELU_BWD, dw.dgrad(d2, "conv2d_1"), a1)
    g["conv2d"] = ctx.conv2d_wgrad(x, d1, 9)
    return y, loss, g


def edsr_loss_and_grads(ctx, w, x, t, scale=2, num_res_blocks=16, res_scaling=0.1):
    """EDSR_model.py:55-125 + mean_squared_error (the compile step ignores its loss argument, :137)."""
    names = ["conv2d"] + [f"conv2d_{i}" for i in range(1, 2 * num_res_blocks + 5)]
    it = iter(names)
    n_head = next(it)
    dw = as_bucket(ctx, w)
    h0 = dw.conv(x, n_head)
    cur, blocks = h0, []
    for _ in range(num_res_blocks):
        na, nb = next(it), next(it)
        tt = dw.conv(cur, na, act="relu")
        nxt = dw.conv(tt, nb, alpha=res_scaling, skip1=cur, beta1=1.0)
        blocks.append((na, nb, cur, tt))
        cur = nxt
    n_body = next(it)
    body = dw.conv(cur, n_body, skip1=h0, beta1=1.0)
    ups, up = [], body
    for r in ([scale] if scale in (2, 3) else [2, 2]):
        nu = next(it)
        v = dw.conv(up, nu, d2s=r)
        ups.append((nu, up, r))
        up = v
    n_out = next(it)
    pre = dw.conv(up, n_out)
    y = ctx.eltwise(L.ELT_CLIP01, pre)
    loss = ctx.mse(t, y)
    g = {}
    dy = ctx.eltwise(L.ELT_AXPBY, y, t, 2.0 / y.numel(), -2.0 / y.numel())
    dpre = ctx.eltwise(L.ELT_CLIP01_BWD, dy, pre)
    g[n_out] = ctx.conv2d_wgrad(up, dpre, 3)
    d = dw.dgrad(dpre, n_out)
    for nu, uin, r in reversed(ups):
        dv = ctx.space_to_depth(d, r)
        g[nu] = ctx.conv2d_wgrad(uin, dv, 3)
        d = dw.dgrad(dv, nu)
    d_h0 = d                                                  # global skip: body = conv(cur) + h0
    g[n_body] = ctx.conv2d_wgrad(cur, d, 3)
    d = dw.dgrad(d, n_body)
    for na, nb, cin, tt in reversed(blocks):
        du = ctx.eltwise(L.ELT_AXPBY, d, None, res_scaling, 0.0)
        g[nb] = ctx.conv2d_wgrad(tt, du, 3)
        dt = ctx.eltwise(L.ELT_RELU_BWD, dw.dgrad(du, nb), tt)
        g[na] = ctx.conv2d_wgrad(cin, dt, 3)
        d = ctx.eltwise(L.ELT_AXPBY, d, dw.dgrad(dt, na), 1.0, 1.0)
    d = ctx.eltwise(L.ELT_AXPBY, d, d_h0, 1.0, 1.0)
    g[n_head] = ctx.conv2d_wgrad(x, d, 3)
    return y, loss, g


def edsr_loss_and_grads_bf16(ctx, bucket, x, t, scale=2, num_res_blocks=16, res_scaling=0.1, tape=None):
    """edsr_loss_and_grads in bf16 mixed precision ("Mixed-precision training").  bucket: the fit's ParamBucket -- fp32 master weights; every conv
    kernel is rounded to bf16 once per step, for its forward and its rotated input-gradient use, by ONE pack launch.  x: the input batch, rounded to bf16
    here when it is fp32; t: the fp32 target, never rounded.  Every activation and activation gradient between kernels is a bf16 tensor written with one
    rounding after an fp32 epilogue; weight and bias gradients are fp32, written into views of one flat tensor in the bucket's order (a FlatGrads).
    tape: a list that receives (name, tensor) for every stored tensor, by reference, in the order they are made:
      x, h0, tt_i / nxt_i per block i = 1.., body, up_j per up-sampling conv j = 1.., pre, dpre, d_out, then per up-sampling conv in reverse dv_j / d_up_j,
      d_body, then per block in reverse du_i (res_scaling * dgrad, before the mask) / dt_i / d_i (d_1 is the head conv's output gradient, both skips added).
    -> (y fp32 = clip(pre), loss fp32 [1], FlatGrads)."""
    if not isinstance(bucket, ParamBucket):
        raise ValueError("edsr_loss_and_grads_bf16: the weights must be a ParamBucket (train_dtype='bf16' needs update='device')")
    if num_res_blocks < 1:
        raise ValueError("edsr_loss_and_grads_bf16: at least one residual block")
    rec = tape.append if tape is not None else (lambda item: None)
    names = ["conv2d"] + [f"conv2d_{i}" for i in range(1, 2 * num_res_blocks + 5)]
    it = iter(names)
    n_head = next(it)
    dev = bucket.dev
    packs = getattr(bucket, "_packs_bf16", None)
    if packs is None:                                                # every layer's forward use, and the input-gradient use of all but the head
        uses = [(dev[n][0], dev[n][1], False) for n in dev] + [(dev[n][0], None, True) for n in dev if n != n_head]
        packs = bucket._packs_bf16 = ctx.pack_list(uses)
    ctx.conv_prepack_bf16(packs)

    def conv(a, name, **kw):
        k, b = dev[name]
        return ctx.conv2d_dev_bf16(a, k, b, k.shape[3], **kw)

    def dgrad(dy, name, **kw):
        k = dev[name][0]
        return ctx.conv2d_dev_bf16(dy, k, None, k.shape[2], rot=True, **kw)

    g = FlatGrads(bucket)

    def wgrad(name, a, dy, s=1.0):
        ctx.conv2d_wgrad_bf16(a, dy, 3, scale=s, out=g[name])

    x = x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)
    rec(("x", x))
    h0 = conv(x, n_head)
    rec(("h0", h0))
    cur, blocks = h0, []
    for i in range(1, num_res_blocks + 1):
        na, nb = next(it), next(it)
        tt = conv(cur, na, act="relu")
        nxt = conv(tt, nb, alpha=res_scaling, skip1=cur, beta1=1.0)
        rec((f"tt_{i}", tt))
        rec((f"nxt_{i}", nxt))
        blocks.append((i, na, nb, cur, tt))
        cur = nxt
    n_body = next(it)
    body = conv(cur, n_body, skip1=h0, beta1=1.0)
    rec(("body", body))
    ups, up = [], body
    for j, r in enumerate([scale] if scale in (2, 3) else [2, 2], 1):
        nu = next(it)
        v = conv(up, nu, d2s=r)
        rec((f"up_{j}", v))
        ups.append((j, nu, up, r))
        up = v
    n_out = next(it)
    pre = conv(up, n_out)
    rec(("pre", pre))
    y, loss, dpre = ctx.mse_clip_grad_bf16(pre, t)
    rec(("dpre", dpre))
    wgrad(n_out, up, dpre)
    d = dgrad(dpre, n_out)
    rec(("d_out", d))
    for j, nu, uin, r in reversed(ups):
        dv = ctx.space_to_depth_bf16(d, r)
        rec((f"dv_{j}", dv))
        wgrad(nu, uin, dv)
        d = dgrad(dv, nu)
        rec((f"d_up_{j}", d))
    d_h0 = d                                                  # global skip: body = conv(cur) + h0
    wgrad(n_body, cur, d)
    d = dgrad(d, n_body)
    rec(("d_body", d))
    for i, na, nb, cin, tt in reversed(blocks):
        wgrad(nb, tt, d, res_scaling)                         # no stored res_scaling * d: the factor is applied to the finished fp32 sums
        du = dgrad(d, nb, alpha=res_scaling)
        rec((f"du_{i}", du))
        dt = ctx.relu_bwd_bf16(du, tt)
        rec((f"dt_{i}", dt))
        wgrad(na, cin, dt)
        d = dgrad(dt, na, skip1=d, beta1=1.0, skip2=d_h0 if i == 1 else None, beta2=1.0 if i == 1 else 0.0)
        rec((f"d_{i}", d))
    wgrad(n_head, x, d)
    return y, loss, g


# ---------------------------------------------------------------------------------------------------------------- fit
class History:
    def __init__(self, keys):
        self.history = {k: [] for k in keys}
        self.epoch = []


class EpochTimeTracker:
    """EpochTimeCallback (callbacks.py:21-42); the custom ESRGAN loop's manual tracker (callbacks.py:104-121)."""
    def __init__(self):
        self.epoch_times_sec = []
        self._t0 = None

    def mean_time_value(self):
        return float(np.mean(self.epoch_times_sec))

    def begin_epoch(self):
        self._t0 = time.perf_counter()

    def end_epoch(self):
        if self._t0 is not None:
            self.epoch_times_sec.append(time.perf_counter() - self._t0)
            self._t0 = None


class EpochMemoryTracker:
    """EpochMemoryCallback (callbacks.py:44-, 123-176): device memory held by libsr355, MB, from its allocator counters in place of
    tf.config.experimental.get_memory_info."""
    def __init__(self, ctx):
        self.gpu_mean_current_mb = []
        self.gpu_peak_mb = []
        self.ctx, self._begin = ctx, None

    def as_dict(self):
        return {"gpu_mean_current_mb": float(np.mean(self.gpu_mean_current_mb)), "gpu_peak_mb": float(np.max(self.gpu_peak_mb))}

    def begin_epoch(self):
        self._begin = self.ctx.mem_info()

    def end_epoch(self):
        end, begin = self.ctx.mem_info(), self._begin or self.ctx.mem_info()
        self.gpu_mean_current_mb.append((begin["current"] + end["current"]) / 2.0 / (1024.0 * 1024.0))
        self.gpu_peak_mb.append(max(begin["peak"], end["peak"]) / (1024.0 * 1024.0))
        self._begin = None


class PlateauCallbacks:
    """The two callbacks on val_loss that change a fit's result, in Keras' order at the end of an epoch: ReduceLROnPlateau(factor, lr_patience,
    min_lr; mode min, min_delta 1e-4, cooldown 0) on `optimizer.lr`, then EarlyStopping(es_patience, min_delta 0, restore_best_weights=True)."""

    def __init__(self, optimizer, es_patience, lr_patience, lr_factor, min_lr, verbose):
        self.opt, self.es_patience, self.verbose = optimizer, es_patience, verbose
        self.lr_patience, self.lr_factor, self.min_lr = lr_patience, lr_factor, min_lr
        self.best, self.best_w, self.es_wait, self.lr_wait, self.lr_best = np.inf, None, 0, 0, np.inf

    def end_epoch(self, ep, val_loss, weights):
        """-> None to go on, or the weights to stop with (a copy of the best epoch's)."""
        if val_loss < self.lr_best - 1e-4:
            self.lr_best, self.lr_wait = val_loss, 0
        else:
            self.lr_wait += 1
            if self.lr_wait >= self.lr_patience and self.opt.lr > self.min_lr:
                self.opt.lr = max(self.opt.lr * self.lr_factor, self.min_lr)
                self.lr_wait = 0
                if self.verbose:
                    print(f"Epoch {ep + 1}: ReduceLROnPlateau reducing learning rate to {self.opt.lr}.")
        if self.best_w is None:  # Keras snapshots the weights at the first epoch even when val_loss is NaN / never improves
            self.best_w = {n: (a.copy(), b.copy()) for n, (a, b) in weights.items()}
        if val_loss < self.best:
            self.best, self.es_wait = val_loss, 0
            self.best_w = {n: (a.copy(), b.copy()) for n, (a, b) in weights.items()}
            return None
        self.es_wait += 1
        if self.es_wait < self.es_patience:
            return None
        if self.verbose:
            print(f"Epoch {ep + 1}: early stopping; restoring model weights from the end of the best epoch.")
        return self.best_w


def fit(ctx, weights, loss_and_grads, predict, optimizer, X_train, Y_train, X_val, Y_val, batch_size=16, epochs=50, es_patience=3,
        lr_patience=2, lr_factor=0.5, min_lr=1e-7, shuffle=True, seed=42, verbose=True):
    """model.fit(X, Y, batch_size, epochs, validation_data, callbacks=[EarlyStopping(val_loss, patience, restore_best_weights=True),
    ReduceLROnPlateau(val_loss, factor, patience, min_lr), EpochTimeCallback, EpochMemoryCallback]).
    weights: {layer: (kernel, bias)} host fp32 with an `Adam` (host update), or a ParamBucket with a `DeviceAdam` over its flat tensor (device
    update: the bucket is trained in place; per epoch the host reads the steps' loss / sum psnr / sum ssim in one copy and the weights for
    validation and the callbacks).  (X_train, Y_train) and (X_val, Y_val): arrays, or the .X / .Y views of one sr355.patches.PatchPairs each --
    the epoch's order then goes up once and every batch is one gather launch; the order comes from the same generator calls, so the batches
    are the array path's.  -> (updated copy of the weights as a host dict, History, EpochTimeTracker, EpochMemoryTracker)."""
    from .patches import views_dataset
    ds_train, ds_val = views_dataset(X_train, Y_train, "(X_train, Y_train)"), views_dataset(X_val, Y_val, "(X_val, Y_val)")
    if ds_train is None:
        X_train, Y_train = np.asarray(X_train, np.float32), np.asarray(Y_train, np.float32)
    if ds_val is None:
        X_val, Y_val = np.asarray(X_val, np.float32), np.asarray(Y_val, np.float32)
    bucket = weights if isinstance(weights, ParamBucket) else None
    if (bucket is not None) != isinstance(optimizer, DeviceAdam):
        raise ValueError("fit: a ParamBucket trains with a DeviceAdam, a host weight dict with an Adam")
    hist, tcb, mcb = History(("loss", "psnr", "ssim", "val_loss", "val_psnr", "val_ssim", "lr")), EpochTimeTracker(), EpochMemoryTracker(ctx)
    callbacks = PlateauCallbacks(optimizer, es_patience, lr_patience, lr_factor, min_lr, verbose)
    rng = np.random.default_rng(seed)
    n, n_val = len(X_train), len(X_val)
    spans = [(i, min(i + batch_size, n)) for i in range(0, n, batch_size)]
    order_val = ds_val.set_order(np.arange(n_val)) if ds_val is not None and n_val else None
    stats = ctx.empty((max(len(spans), 1), 3), torch.float32) if bucket is not None else None
    for ep in range(epochs):
        mcb.begin_epoch()
        tcb.begin_epoch()
        order = rng.permutation(n) if shuffle else np.arange(n)
        order_dev = ds_train.set_order(order) if ds_train is not None and n else None
        tot = np.zeros(3, np.float64)
        for s, (i, j) in enumerate(spans):
            if ds_train is not None:
                x, t = ds_train.batch(order_dev, i, j - i)
            else:
                idx = order[i:j]
                x, t = ctx.to_device(X_train[idx]), ctx.to_device(Y_train[idx])
            y, loss, grads = loss_and_grads(ctx, weights, x, t)
            if bucket is None:
                tot += [float(loss.item()) * (j - i), float(ctx.psnr(t, y).sum().item()), float(ctx.ssim(t, y).sum().item())]
                host_g = {name: (dw.cpu().numpy(), db.cpu().numpy()) for name, (dw, db) in grads.items()}
                weights = optimizer.apply(weights, host_g)
            else:
                stats[s, 0:1].copy_(loss)
                stats[s, 1].copy_(ctx.psnr(t, y).sum())
                stats[s, 2].copy_(ctx.ssim(t, y).sum())
                optimizer.apply(bucket.flat, bucket.gather(grads))
                bucket.stale = True
        if bucket is not None:
            st = stats.cpu().numpy()                                     # the epoch's statistics, one copy; then the host path's fp64 sums
            for s, (i, j) in enumerate(spans):
                tot += [float(st[s, 0]) * (j - i), float(st[s, 1]), float(st[s, 2])]
        host_w = dict(bucket.host()) if bucket is not None else weights   # (a new dict per epoch: predict() reloads the model when it sees one)
        vt = np.zeros(3, np.float64)
        for i in range(0, n_val, batch_size):
            if ds_val is not None:
                x, t = ds_val.batch(order_val, i, min(batch_size, n_val - i))
            else:
                x, t = ctx.to_device(X_val[i:i + batch_size]), ctx.to_device(Y_val[i:i + batch_size])
            y = predict(ctx, host_w, x)
            vt += [float(ctx.mse(t, y).item()) * len(x), float(ctx.psnr(t, y).sum().item()), float(ctx.ssim(t, y).sum().item())]
        torch.cuda.synchronize(ctx.torch_device)
        tr, va = tot / max(n, 1), vt / max(n_val, 1)
        for key, val in zip(("loss", "psnr", "ssim", "val_loss", "val_psnr", "val_ssim"), list(tr) + list(va)):
            hist.history[key].append(float(val))
        hist.history["lr"].append(optimizer.lr)
        hist.epoch.append(ep)
        tcb.end_epoch()
        mcb.end_epoch()
        if verbose:
            print(f"Epoch {ep + 1}/{epochs} - loss: {tr[0]:.4f} - psnr: {tr[1]:.4f} - ssim: {tr[2]:.4f} - val_loss: {va[0]:.4f} - "
                  f"val_psnr: {va[1]:.4f} - val_ssim: {va[2]:.4f} - lr: {optimizer.lr:.2e}")
        best_w = callbacks.end_epoch(ep, va[0], host_w)
        if best_w is not None:
            if bucket is not None:
                bucket.load(best_w)
            weights = best_w
            break
    if bucket is not None:
        weights = {name: (k.copy(), b.copy()) for name, (k, b) in bucket.host().items()}
    return weights, hist, tcb, mcb


# ---------------------------------------------------------------------------------------------------------------- classifier head
def head_forward(g, w, training=False, dropout_rate=0.0, rng=None):
    """GAP features [N,512] -> Dropout -> Dense256 ReLU -> Dropout -> Dense softmax (VGG16_model.py:84-97), host fp32/fp64.
    -> (probabilities, cache for head_backward)."""
    k1, b1 = w["dense"]
    k2, b2 = w["predictions"]
    keep = 1.0 - dropout_rate
    m0 = m1 = None
    x0 = g
    if training and dropout_rate > 0:
        m0 = (rng.random(g.shape) < keep) / keep
        x0 = g * m0
    z1 = x0 @ k1 + b1
    a1 = np.maximum(z1, 0)
    x1 = a1
    if training and dropout_rate > 0:
        m1 = (rng.random(a1.shape) < keep) / keep
        x1 = a1 * m1
    z2 = x1 @ k2 + b2
    z2 = z2 - z2.max(axis=1, keepdims=True)
    e = np.exp(z2)
    p = e / e.sum(axis=1, keepdims=True)
    return p, (x0, z1, x1, m1)


def sparse_cce(p, y, eps=1e-7):
    """keras sparse_categorical_crossentropy on probabilities (clipped to [eps, 1-eps]) -> (mean loss, accuracy)."""
    pc = np.clip(p[np.arange(len(y)), y], eps, 1.0 - eps)
    return float(np.mean(-np.log(pc))), float(np.mean(np.argmax(p, axis=1) == y))


def head_backward(p, y, cache, w, l2_reg=0.0):
    """Gradients of mean sparse-CCE (+ l2_reg * sum(dense kernel^2), VGG16_model.py:90-92) w.r.t. the two Dense layers."""
    x0, z1, x1, m1 = cache
    n = len(y)
    dz2 = p.copy()
    dz2[np.arange(n), y] -= 1.0
    dz2 /= n
    k2 = w["predictions"][0]
    g = {"predictions": (x1.T @ dz2, dz2.sum(axis=0))}
    dx1 = dz2 @ k2.T
    da1 = dx1 * m1 if m1 is not None else dx1
    dz1 = da1 * (z1 > 0)
    g["dense"] = (x0.T @ dz1 + 2.0 * l2_reg * w["dense"][0], dz1.sum(axis=0))
    return g


def fit_head(features, w, X_train_batches, y_train, X_val, y_val, learning_rate=1e-3, batch_size=32, epochs=50, dropout_rate=0.2,
             l2_reg=0.0, seed=42, verbose=True):
    """model.fit of the frozen-base classifier (VGG16_model.py:111-157): Adam, sparse categorical cross-entropy, accuracy,
    EarlyStopping(val_loss, patience 3, restore_best_weights) and ReduceLROnPlateau(val_loss, 0.5, patience 2, min_lr 1e-7).
    features(images) -> [n,512] GAP features (the device runs the frozen conv base); X_train_batches(epoch) yields (images, labels)
    batches of one epoch (shuffled / augmented by the caller).  -> (head weights, History)."""
    head = {n: (np.asarray(w[n][0], np.float32), np.asarray(w[n][1], np.float32)) for n in ("dense", "predictions")}
    opt = Adam(head, learning_rate, epsilon=1e-7)
    rng = np.random.default_rng(seed)
    hist = History(("loss", "accuracy", "val_loss", "val_accuracy", "lr"))
    callbacks = PlateauCallbacks(opt, 3, 2, 0.5, 1e-7, verbose)
    g_val = features(X_val)
    for ep in range(epochs):
        tot, n_seen = np.zeros(2, np.float64), 0
        for xb, yb in X_train_batches(ep):
            yb = np.asarray(yb, np.int64)
            p, cache = head_forward(features(xb).astype(np.float32), head, True, dropout_rate, rng)
            loss, acc = sparse_cce(p, yb)
            if l2_reg > 0:
                loss += l2_reg * float(np.sum(head["dense"][0].astype(np.float64) ** 2))
            tot += [loss * len(yb), acc * len(yb)]
            n_seen += len(yb)
            grads = head_backward(p, yb, cache, head, l2_reg)
            head = opt.apply(head, {n: (a.astype(np.float32), b.astype(np.float32)) for n, (a, b) in grads.items()})
        pv, _ = head_forward(g_val.astype(np.float32), head)
        vl, va = sparse_cce(pv, np.asarray(y_val, np.int64))
        if l2_reg > 0:
            vl += l2_reg * float(np.sum(head["dense"][0].astype(np.float64) ** 2))
        tr = tot / max(n_seen, 1)
        for key, val in zip(("loss", "accuracy", "val_loss", "val_accuracy", "lr"), (tr[0], tr[1], vl, va, opt.lr)):
            hist.history[key].append(float(val))
        hist.epoch.append(ep)
        if verbose:
            print(f"Epoch {ep + 1}/{epochs} - loss: {tr[0]:.4f} - accuracy: {tr[1]:.4f} - val_loss: {vl:.4f} - val_accuracy: {va:.4f} - lr: {opt.lr:.2e}")
        best_w = callbacks.end_epoch(ep, vl, head)
        if best_w is not None:
            head = best_w
            break
    return head, hist


_NP2TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


def upload_packed(ctx, arrays):
    """{name: host array (fp32 / int32 / uint8)} -> {name: device tensor} through ONE host-to-device copy: the arrays are packed into one
    byte buffer (256-byte aligned sections) and the device tensors are typed views of its upload."""
    arrays = {k: np.ascontiguousarray(a) for k, a in arrays.items()}
    offs, o = {}, 0
    for k, a in arrays.items():
        offs[k] = o
        o += (a.nbytes + 255) // 256 * 256
    buf = np.zeros(max(o, 256), np.uint8)
    for k, a in arrays.items():
        buf[offs[k]:offs[k] + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = ctx.to_device(buf)
    return {k: dev[offs[k]:offs[k] + a.nbytes].view(_NP2TORCH[a.dtype]).reshape(a.shape) for k, a in arrays.items()}


def fit_head_device(ctx, features, w, draw_epoch, n_train, g_val, y_val, learning_rate=1e-3, batch_size=32, epochs=50, dropout_rate=0.2,
                    l2_reg=0.0, seed=42, verbose=True, trainer=None):
    """fit_head on the device: the same fit (VGG16_model.py:111-157), history, print lines and callbacks, with the head in one flat device
    bucket (ParamBucket) trained by sr_dense_head_step + DeviceAdam.  draw_epoch(ep) -> {name: host array} of the epoch, one row per training
    sample in the epoch's order, with at least "labels" (int32); the dropout keep masks are drawn here on fit_head's own generator, in its order
    (m0 [n_b,512] then m1 [n_b,256] per batch), and everything goes up in one copy per epoch.  features(dev, i, j) -> fp32 device [j-i,512] GAP
    features of the epoch's samples i..j-1 (dev: the uploaded arrays).  g_val fp32 device [n_val,512].  The host reads the per-batch statistics
    and the head (131 842 parameters at two classes, for EarlyStopping) once per epoch.  -> (head weights, History).
    trainer (a vgg_train.VGGFineTuner built on w): the same fit of ITS bucket -- trainable convs and head under its one DeviceAdam.  features()
    then returns what trainer.step consumes (the frozen prefix's activations), g_val is a callable that returns the validation features under
    the epoch's weights, the callbacks see, snapshot and restore the whole bucket, and every layer of it is returned."""
    head = {n: (np.asarray(w[n][0], np.float32), np.asarray(w[n][1], np.float32)) for n in ("dense", "predictions")}
    num_classes = head["predictions"][0].shape[1]
    y_val = np.asarray(y_val, np.int64).reshape(-1)
    if len(y_val) and (y_val.min() < 0 or y_val.max() >= num_classes):
        raise ValueError(f"labels must lie in [0, {num_classes})")
    if trainer is None:
        bucket = ParamBucket(ctx, head)
        opt = DeviceAdam(ctx, bucket.flat, learning_rate, epsilon=1e-7)
        grads = torch.empty_like(bucket.flat)
        head_flat = bucket.flat
    else:
        bucket, opt, head_flat = trainer.bucket, trainer.opt, trainer.head
    rng = np.random.default_rng(seed)
    hist = History(("loss", "accuracy", "val_loss", "val_accuracy", "lr"))
    callbacks = PlateauCallbacks(opt, 3, 2, 0.5, 1e-7, verbose)
    keep = 1.0 - dropout_rate
    spans = [(i, min(i + batch_size, n_train)) for i in range(0, n_train, batch_size)]
    n_val = len(y_val) if callable(g_val) else int(g_val.shape[0])
    yv = ctx.to_device(y_val.astype(np.int32))
    stats = ctx.empty((len(spans) + 1, 3), torch.float64)
    work = ctx.dense_head_workspace(max(batch_size, n_val, 1), num_classes)
    for ep in range(epochs):
        plan = dict(draw_epoch(ep))
        if dropout_rate > 0:
            m0, m1 = [], []
            for i, j in spans:
                m0.append(rng.random((j - i, 512)) < keep)
                m1.append(rng.random((j - i, 256)) < keep)
            plan["keep0"], plan["keep1"] = np.concatenate(m0).astype(np.uint8), np.concatenate(m1).astype(np.uint8)
        dev = upload_packed(ctx, plan)
        for s, (i, j) in enumerate(spans):
            k0, k1 = (dev["keep0"][i:j], dev["keep1"][i:j]) if dropout_rate > 0 else (None, None)
            if trainer is None:
                ctx.dense_head_step(features(dev, i, j), dev["labels"][i:j], bucket.flat, num_classes, stats[s], work, grads, k0, k1, 1.0 / keep, l2_reg)
                opt.apply(bucket.flat, grads)
            else:
                trainer.step(features(dev, i, j), dev["labels"][i:j], stats[s], work, k0, k1, 1.0 / keep, l2_reg)
        if n_val:
            ctx.dense_head_step(g_val() if callable(g_val) else g_val, yv, head_flat, num_classes, stats[len(spans)], work)
        bucket.stale = True
        weights = bucket.host()
        st = stats.cpu().numpy()
        tot, n_seen = np.zeros(2, np.float64), 0
        for s, (i, j) in enumerate(spans):
            nb = j - i
            loss, acc = st[s, 0] / nb, st[s, 1] / nb
            if l2_reg > 0:
                loss += l2_reg * st[s, 2]
            tot += [loss * nb, acc * nb]
            n_seen += nb
        vl, va = (st[-1, 0] / n_val, st[-1, 1] / n_val) if n_val else (np.nan, np.nan)
        if l2_reg > 0:
            vl += l2_reg * st[-1, 2]
        tr = tot / max(n_seen, 1)
        for key, val in zip(("loss", "accuracy", "val_loss", "val_accuracy", "lr"), (tr[0], tr[1], vl, va, opt.lr)):
            hist.history[key].append(float(val))
        hist.epoch.append(ep)
        if verbose:
            print(f"Epoch {ep + 1}/{epochs} - loss: {tr[0]:.4f} - accuracy: {tr[1]:.4f} - val_loss: {vl:.4f} - val_accuracy: {va:.4f} - lr: {opt.lr:.2e}")
        best_w = callbacks.end_epoch(ep, vl, weights)
        if best_w is not None:
            bucket.load(best_w)
            break
    return {n: (k.copy(), b.copy()) for n, (k, b) in bucket.host().items()}, hist
