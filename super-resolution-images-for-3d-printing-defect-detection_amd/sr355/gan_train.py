"""ESRGAN._train_step on MI355X (reference: ESRGAN_model.py:475-533; networks :212-399, losses :401-473, optimisers :176-195).

One training step = discriminator update (BCE on D(real) vs 1 and D(G(lr)) vs 0) then generator update (BCE(1, D(fake)) + 1.0 x
perceptual + 100 x L1 + 1.0 x spectral), both Adam with a staircase learning-rate decay, D's SpectralNormalization wrappers
renormalising their kernels in place on each of the three training=True calls.

The forward and backward passes are host orchestration over the C ABI's single ops, fp32 as the reference trains:
  * convs: the MFMA forward kernels; input gradients are the same kernels on 180-degree-rotated, channel-swapped weights; kernel / bias
    gradients the fp32-MFMA wgrad kernel (csrc/train_ops.hip);
  * SelfAttention of the small training patches is materialised by default (sr_matmul + row softmax) so that its backward is six GEMMs and a
    softmax-backward kernel; attention_impl="streamed" runs it through sr_attention_fwd_lse / sr_attention_bwd instead, which keep no
    [B,N,N] tensor (csrc/attention_train.hip); pooling / stride-2 sampling / depth_to_space / activations / the (W,C)-FFT loss have their own adjoint kernels;
  * a minimal reverse-mode tape (below) keeps the graph bookkeeping out of the kernels; torch is used for memory only (cat / slice /
    flip / expand: data movement).
ESRGANTrainer.train_step is ONE body for both homes of the discriminator's tiny vectors -- its [B,256] dense head, BCE on [B,1], spectral-norm
power iteration, Adam.  It talks to a discriminator object: three critic() calls (one training=True call each: renormalise, six convs
(disc_trunk), head, BCE, backward) and one update().  HostDiscriminator (discriminator="host", the default) keeps them on the host in NumPy
and uploads its parameters after every renormalisation; DeviceDiscriminator (discriminator="device") keeps the parameters, u and Adam's
moments in flat device buckets: one launch renormalises all eight kernels (sr_spectral_norm_bucket), two run the head with its loss and
backward (sr_disc_head_step), and the step's six loss scalars come back in one copy (csrc/disc_train.hip).
The generator's parameters are device-resident in both modes; kernels are packed into MFMA fragment order on the device per layer call
(sr_conv2d_dev); the tape bookkeeping stays on the host.  cfg3's throughput is the `cfg3 ESRGAN _train_step` row of bench.py --full
(sr355/bench_rows.py cfg3_train_step), and tools/bench_train.py measures it alone, in either mode.
train_dtype="bf16" (opt-in; ESRGANTrainer, ESRGAN) runs the RRDB trunk of the taped training pass in bf16 mixed precision -- Tape.trunk_bf16, one tape op
on bf16 concat buffers with fp32 master weights and gradients; everything outside the trunk, and the default, stay fp32 (DESIGN.md 3.26;
tools/bench_esrgan_mixed.py measures it against the fp32 trainer).
dense_block_impl="lds" (opt-in, with train_dtype="bf16", growth width 8, patches up to 24 x 24) runs every dense block of that trunk as one forward and one backward
kernel whose concat tensor and its gradient live in a CU's LDS -- Tape.trunk_lds, the same arithmetic contract (tools/bench_dense_block_train.py).
perceptual_dtype="bf16" (opt-in; independent of the options above) runs train_step's VGG19 perceptual term and its gradient in bf16 mixed precision -- PerceptualBf16:
one forward over [fake | hr], one backward over fake, frozen weights packed once (tools/bench_perceptual_mixed.py).
"""
import contextlib

import numpy as np
import torch

from . import _lib as L
from .train import Adam, DeviceAdam, FlatGrads, ParamBucket, _rot


# ----------------------------------------------------------------------------------------------------------------- tape
ATTENTION_IMPLS = ("materialised", "streamed")


def check_attention_impl(value):
    """How the tape runs SelfAttention's core: "materialised" (the default: beta = softmax(g f^T) as a [B, N, N] tensor, its backward six GEMMs)
    or "streamed" (sr_attention_fwd_lse / sr_attention_bwd: O(B N) state, no [B, N, N] tensor)."""
    if value not in ATTENTION_IMPLS:
        raise ValueError(f"attention_impl must be one of {ATTENTION_IMPLS}, got {value!r}")
    return value


TRAIN_DTYPES = ("f32", "bf16")


def check_train_dtype(value):
    """What the taped training pass stores inside the RRDB trunk: "f32" (the default, the reference's training) or "bf16" (bf16 activations and activation
    gradients between the trunk's kernels, fp32 everywhere else: Tape.trunk_bf16)."""
    if value not in TRAIN_DTYPES:
        raise ValueError(f"train_dtype must be one of {TRAIN_DTYPES}, got {value!r}")
    return value


DENSE_BLOCK_IMPLS = ("layers", "lds")


def check_dense_block_impl(value, train_dtype="bf16"):
    """How the bf16 trunk runs a dense block: "layers" (the default: conv by conv on the virtual-concat buffer, Tape.trunk_bf16) or "lds" (one forward and one
    backward kernel per block on an LDS-resident image, Tape.trunk_lds: growth width 8, patches up to 24 x 24).  "lds" is bf16 arithmetic: it needs train_dtype="bf16"."""
    if value not in DENSE_BLOCK_IMPLS:
        raise ValueError(f"dense_block_impl must be one of {DENSE_BLOCK_IMPLS}, got {value!r}")
    if value == "lds" and train_dtype != "bf16":
        raise ValueError(f"dense_block_impl='lds' runs the trunk in bf16 mixed precision: it needs train_dtype='bf16', got train_dtype={train_dtype!r}")
    return value


def trunk_blocks(num_rrdb):
    """The trunk's dense blocks in forward order."""
    return [f"rrdb_{b}_dense{d}" for b in range(num_rrdb) for d in (1, 2, 3)]


def _trunk_walk(weights, num_rrdb, check):
    """The trunk's conv layers in forward order; check(layer name, k, kernel shape) raises for the first layer that a trunk implementation cannot take."""
    layers = [(f"{n}_conv{k}", k) for n in trunk_blocks(num_rrdb) for k in range(1, 6)]
    for layer, k in layers:
        check(layer, k, tuple(weights[layer][0].shape))
    return [layer for layer, _ in layers]


def trunk_layers_lds(weights, num_rrdb):
    """The trunk's conv layers in forward order; ValueError naming the first layer that is not a 64-channel dense block of growth width 8's (the LDS-resident kernels)."""
    def check(layer, k, got):
        want = (3, 3, 64 + 8 * (k - 1), 8 if k < 5 else 64)
        if got != want:
            what = f"{got[3]} growth channels" if k < 5 and got[:3] == want[:3] else f"a kernel of shape {got}"
            raise ValueError(f"dense_block_impl='lds': {layer} has {what}; the LDS-resident dense-block kernels take 64-channel blocks of growth width 8 "
                             f"(kernel {want}); train this graph with dense_block_impl='layers'")
    return _trunk_walk(weights, num_rrdb, check)


def lds_patch_check(ctx, H, W):
    """ValueError where an H x W patch does not fit the LDS-resident training kernels (there is no other path behind dense_block_impl='lds')."""
    if not ctx.dense_block_train_fits(H, W):
        raise ValueError(f"dense_block_impl='lds': a patch of H = {H}, W = {W} does not fit the LDS-resident dense-block kernels, which take (H + 2)(W + 2) <= "
                         f"{ctx.dense_block_train_max_pixels()} (24 x 24); train larger patches with dense_block_impl='layers'")


def trunk_layers(weights, num_rrdb):
    """The trunk's conv layers in forward order; ValueError where a dense block's growth width is not a whole number of the bf16 conv kernels' 32-channel chunks."""
    def check(layer, k, got):
        if got[3] % 32 != 0:
            what, hint = ("growth", " (growth_channels must be a multiple of 32; train this graph with train_dtype='f32')") if k < 5 else ("output", "")
            raise ValueError(f"train_dtype='bf16': {layer} has {got[3]} {what} channels; the bf16 conv kernels work in chunks of 32 channels{hint}")
    return _trunk_walk(weights, num_rrdb, check)


def lds_pack_plan(ctx, dev, num_rrdb):
    """(table, fwd, bias, bwd, {block name: row}): what packs the trunk's dense blocks for the LDS-resident kernels -- ctx.dense_block_pack_dev(table, fwd, bias, bwd)
    fills the three buffers from the weights as they stand then.  dev(layer name) -> (fp32 device kernel, fp32 device bias)."""
    names = trunk_blocks(num_rrdb)
    layers = [[dev(f"{n}_conv{k}") for k in range(1, 6)] for n in names]
    table = ctx.dense_block_pack_table([([k for k, _ in block], [b for _, b in block]) for block in layers])
    return (table,) + ctx.dense_block_pack_buffers(len(names)) + ({n: i for i, n in enumerate(names)},)


class Var:
    __slots__ = ("v", "g", "need")

    def __init__(self, v, need=True):
        self.v, self.g, self.need = v, None, need


class Tape:
    """Reverse-mode bookkeeping: ops push a closure; backward() runs them last-to-first.  Parameter gradients land in `grads`
    ({layer: [dk, db]}, summed over uses) when `wgrad` is on."""

    def __init__(self, ctx, weights, wgrad=True, devcache=None, attention_impl="materialised", trunk_dtype="f32", flat_grads=None, dense_block_impl="layers"):
        self.ctx, self.w, self.wgrad = ctx, weights, wgrad
        self.attention_impl = check_attention_impl(attention_impl)
        self.trunk_dtype = check_train_dtype(trunk_dtype)      # "bf16": generator_forward runs the RRDB trunk as ONE op on bf16 buffers (trunk_bf16)
        self.dense_block_impl = check_dense_block_impl(dense_block_impl, trunk_dtype)      # "lds": ... by trunk_lds instead
        self.lds_packs = None                                   # (fwd, bias, bwd, {block name: row}) of sr_dense_block_pack_dev: a trainer's, packed once per step; None: trunk_lds packs
        self.trunk_stages = False                               # tests: with trunk_tape, trunk_lds also records the G_b_d_s* stages (the backward kernel's stage dump)
        # A FlatGrads of the parameter bucket: the trunk's weight-gradient kernels write straight into its views, the fp32 layers' gradients are copied into
        # theirs, and `grads` holds the views of the layers written so far; ParamBucket.gather then hands the flat tensor on as it is.
        self.flat = flat_grads
        self.trunk_tape = None                                  # tests: a list here receives (name, tensor) for every tensor trunk_bf16 stores
        self.ops, self.grads = [], {}
        self.masks = None                                       # diagnostics: a dict here collects {layer: activation > 0} of every ReLU / LeakyReLU conv
        self.dev = devcache if devcache is not None else {}     # id(host array) -> (host array, device tensor): one upload per array
        self.conv_wgrad = ctx.conv2d_wgrad                      # (x, dz, k) -> (dw, db): a trainer may route small maps to another kernel

    def _dev(self, a):
        hit = self.dev.get(id(a))
        if hit is None or hit[0] is not a:
            hit = (a, self.ctx.to_device(np.ascontiguousarray(a, np.float32)))
            self.dev[id(a)] = hit
        return hit[1]

    def _acc(self, var, g):
        if not var.need:
            return
        var.g = g if var.g is None else self.ctx.eltwise(L.ELT_AXPBY, var.g, g, 1.0, 1.0)

    def _pgrad(self, name, dw, db):
        if self.flat is not None:
            vw, vb = self.flat[name]
            first = name not in self.grads
            vw.copy_(dw if first else self.ctx.eltwise(L.ELT_AXPBY, vw, dw, 1.0, 1.0))
            vb.copy_(db if first else self.ctx.eltwise(L.ELT_AXPBY, vb, db, 1.0, 1.0))
            self.grads[name] = [vw, vb]
        elif name in self.grads:
            self.grads[name][0] = self.ctx.eltwise(L.ELT_AXPBY, self.grads[name][0], dw, 1.0, 1.0)
            self.grads[name][1] = self.ctx.eltwise(L.ELT_AXPBY, self.grads[name][1], db, 1.0, 1.0)
        else:
            self.grads[name] = [dw, db]

    # ---- ops
    def conv(self, x, name, act="linear", d2s=1, kernel=None):
        """Keras Conv2D SAME stride 1 (+ activation, + depth_to_space for the upsample blocks)."""
        ctx = self.ctx
        k, b = kernel if kernel is not None else self.w[name]
        kd = self._dev(k)
        y = Var(ctx.conv2d_dev(x.v, kd, self._dev(b), k.shape[3], act=act, d2s=d2s))
        if self.masks is not None and act in ("relu", "lrelu"):
            self.masks[name] = y.v > 0

        def bwd():
            if y.g is None:
                return
            dz = y.g
            if act == "relu":
                dz = ctx.eltwise(L.ELT_RELU_BWD, dz, y.v)
            elif act == "lrelu":
                dz = ctx.eltwise(L.ELT_LRELU_BWD, dz, y.v)
            elif act == "tanh":
                dz = ctx.eltwise(L.ELT_TANH_BWD, dz, y.v)
            if d2s > 1:
                dz = ctx.space_to_depth(dz, d2s)                   # activation is element-wise: its mask commutes with the shuffle
            if self.wgrad:
                dw, db = self.conv_wgrad(x.v, dz, k.shape[0])
                self._pgrad(name, dw, db)
            if x.need:
                self._acc(x, ctx.conv2d_dev(dz, kd, None, k.shape[2], rot=True))
        self.ops.append(bwd)
        return y

    def cat(self, xs):
        if len(xs) == 1:
            return xs[0]
        y = Var(torch.cat([x.v for x in xs], dim=-1).contiguous())
        sizes = [x.v.shape[-1] for x in xs]

        def bwd():
            if y.g is None:
                return
            o = 0
            for x, c in zip(xs, sizes):
                self._acc(x, y.g[..., o:o + c].contiguous())
                o += c
        self.ops.append(bwd)
        return y

    def dense_block(self, x, name, growth):
        """ESRGAN._dense_block (ESRGAN_model.py:212-254) as ONE tape op on a virtual-concat buffer: F = [x | f1 | f2 | f3 | f4] lives in one
        [B,H,W,64+4g] tensor, conv k reads its channel prefix and writes slice k (sr_conv2d_dev_views); returns x + 0.2 * conv5(F).  Backward: the
        gradient of F is one buffer too -- conv5's input gradient fills it, every growth conv's accumulates into its prefix IN PLACE (skip = output
        range), ReLU masks and weight gradients read their slices where they lie.  Round 3 built F by four torch.cat copies and took the gradient apart
        by ~14 slice copies and as many accumulate launches per block."""
        ctx = self.ctx
        B, H, W, C0 = x.v.shape
        g = int(growth)
        Ct = C0 + 4 * g
        F = ctx.empty((B, H, W, Ct))
        ctx.eltwise_view(L.ELT_AXPBY, x.v, 0, None, 0, F, 0, C0, 1.0, 0.0)
        ws = [self.w[f"{name}_conv{k}"] for k in range(1, 6)]
        for k in range(1, 5):
            kk, bb = ws[k - 1]
            cin = C0 + (k - 1) * g
            ctx.conv2d_dev_view(F, 0, cin, self._dev(kk), self._dev(bb), g, F, cin, act="relu")
            if self.masks is not None:
                self.masks[f"{name}_conv{k}"] = F[..., cin:cin + g] > 0
        k5, b5 = ws[4]
        y = Var(ctx.empty((B, H, W, C0)))
        ctx.conv2d_dev_view(F, 0, Ct, self._dev(k5), self._dev(b5), C0, y.v, 0, alpha=0.2, skip_buf=F, skip_coff=0, beta1=1.0)      # x + 0.2 * conv5

        def bwd():
            if y.g is None:
                return
            G = ctx.empty((B, H, W, Ct))
            dz5 = ctx.eltwise(L.ELT_AXPBY, y.g, None, 0.2, 0.0)
            if self.wgrad:
                self._pgrad(f"{name}_conv5", *ctx.conv2d_wgrad_view(F, 0, Ct, dz5, 0, C0, 3))
            ctx.conv2d_dev_view(dz5, 0, C0, self._dev(k5), None, Ct, G, 0, rot=True)                        # fills every channel of G
            dz = ctx.empty((B, H, W, g))
            for k in range(4, 0, -1):
                kk, _ = ws[k - 1]
                cin = C0 + (k - 1) * g
                ctx.eltwise_view(L.ELT_RELU_BWD, G, cin, F, cin, dz, 0, g)                                 # slice k of G is complete: convs k+1..5 have added to it
                if self.wgrad:
                    self._pgrad(f"{name}_conv{k}", *ctx.conv2d_wgrad_view(F, 0, cin, dz, 0, g, 3))
                ctx.conv2d_dev_view(dz, 0, g, self._dev(kk), None, cin, G, 0, rot=True, skip_buf=G, skip_coff=0, beta1=1.0)   # G[..., :cin] += dgrad
            if x.need:
                dx = ctx.empty((B, H, W, C0))
                ctx.eltwise_view(L.ELT_AXPBY, G, 0, y.g, 0, dx, 0, C0, 1.0, 1.0)                           # + the skip path's share
                self._acc(x, dx)
        self.ops.append(bwd)
        return y

    def _trunk_mixed(self, x, num_rrdb, tape, growth, forward, backward):
        """The RRDB trunk (ESRGAN_model.py:212-300: num_rrdb x three dense blocks, each RRDB closed by r_in + 0.2 * x) as ONE tape op in bf16 mixed precision
        (DESIGN.md 3.26), written once for trunk_bf16 and trunk_lds.  They say how ONE block runs: growth {block: growth width}; forward(name, F, nxt, r_in, a5, bx)
        fills F's growth slices and nxt[..., :64] = a5 * conv5(F) + bx * F[..., :64] (+ r_in[..., :64] unless None); backward(b, d, name, F, dY, a5, bx, rec) -> (dz, dX),
        dz_k being channel slice k - 1, and records its G stages through rec unless None.
        x: the fp32 output of initial_conv; returns the fp32 input of trunk_conv (a widening, exact).  Every tensor in between is bf16: each kernel widens to fp32,
        accumulates and applies its whole epilogue in fp32 and rounds once on store.  F = [x | f1 | f2 | f3 | f4] is one buffer per dense block; a block's output
        x + 0.2 * conv5 -- for an RRDB's third block r_in + 0.2 * (x + 0.2 * conv5), r_in being slice 0 of the RRDB's first F -- is slice 0 of the NEXT block's F.
        Backward, per block: the five layers' weight and bias gradients by one grouped launch, written into the flat gradient bucket (conv5's scaled by a5: there is
        no stored a5 * dY).  Per RRDB one add: d r_in = dX1 + dR.
        With `tape` (default: the tape's `trunk_tape`) a list, every stored tensor is appended as (name, tensor) -- x0_f32 (the fp32 input), F_b_d, out, dout_f32 (the
        fp32 gradient arriving), dR_last, then per block in reverse G_b_d_s5 / _s4 / _s3 / _s2 (G after conv5's input gradient and after each in-place accumulate),
        dz_b_d, dX_b_d and per RRDB drin_b."""
        ctx = self.ctx
        BF = torch.bfloat16
        B, H, W, C0 = x.v.shape
        tape = self.trunk_tape if tape is None else tape
        rec = tape.append if tape is not None else None
        note = rec or (lambda item: None)                       # here a record is a reference; a block's backward pays for its records, so it is told (rec)
        names = trunk_blocks(num_rrdb)
        widths = [C0 + 4 * growth[n] for n in names] + [C0]     # channels of every block's F, and of the trunk's output
        blocks = []                                             # (b, d, name, F, a5, bx)
        F = ctx.empty((B, H, W, widths[0]), BF)
        F[..., :C0].copy_(x.v)                                  # the one rounding of x0, into slice 0 of the first F
        note(("x0_f32", x.v))
        for i, name in enumerate(names):
            b, d = i // 3, i % 3 + 1
            if d == 1:
                r_in = F
            nxt = ctx.empty((B, H, W, widths[i + 1]), BF)
            a5, bx = (0.2, 1.0) if d < 3 else (0.04, 0.2)       # the third block: r_in + 0.2 * (x + 0.2 * conv5) in one epilogue, one rounding
            forward(name, F, nxt, r_in if d == 3 else None, a5, bx)
            if self.masks is not None:
                g = growth[name]
                for k in range(1, 5):
                    self.masks[f"{name}_conv{k}"] = F[..., C0 + (k - 1) * g:C0 + k * g] > 0
            note((f"F_{b}_{d}", F))
            blocks.append((b, d, name, F, a5, bx))
            F = nxt
        note(("out", F))
        y = Var(F.float())

        def bwd():
            if y.g is None:
                return
            dR = y.g.to(BF)                                     # the one rounding of the gradient entering the trunk
            note(("dout_f32", y.g))
            note((f"dR_{num_rrdb - 1}", dR))
            dY = dR
            for b, d, name, F, a5, bx in reversed(blocks):
                dz, dX = backward(b, d, name, F, dY, a5, bx, rec)
                if self.wgrad:
                    g, Ct = dz.shape[3] // 4, F.shape[3]
                    jobs = [(F, 0, C0 + (k - 1) * g, dz, (k - 1) * g, g, 1.0) + tuple(self.flat[f"{name}_conv{k}"]) for k in range(1, 5)]
                    jobs.append((F, 0, Ct, dY, 0, C0, a5) + tuple(self.flat[f"{name}_conv5"]))
                    ctx.conv2d_wgrad_group_bf16(jobs)
                    for k in range(1, 6):
                        self.grads[f"{name}_conv{k}"] = list(self.flat[f"{name}_conv{k}"])
                note((f"dz_{b}_{d}", dz))
                note((f"dX_{b}_{d}", dX))
                dY = dX
                if d == 1:
                    d_rin = ctx.empty((B, H, W, C0), BF)
                    ctx.eltwise_view_bf16(L.ELT_AXPBY, dX, 0, dR, 0, d_rin, 0, C0, 1.0, 1.0)
                    note((f"drin_{b}", d_rin))
                    dR = dY = d_rin
            if x.need:
                self._acc(x, dR.float())
        self.ops.append(bwd)
        return y

    def trunk_bf16(self, x, num_rrdb, tape=None):
        """_trunk_mixed with every dense block conv by conv on channel views of its concat buffer, at any growth width the bf16 conv kernels take.  Forward: conv k
        reads its channel prefix and writes slice k.  Backward: G = a5 * dgrad(dY, conv5) fills a buffer of F's shape; for k = 4..2 dz_k = G slice k where F slice k > 0,
        G[..., :cin_k] += dgrad(dz_k) in place; dX = dgrad(dz_1) + G[..., :64] + bx * dY.  A recorded G stage is a clone."""
        ctx, dev = self.ctx, self._dev
        if self.flat is None and self.wgrad:
            raise ValueError("trunk_bf16: the weight gradients need a FlatGrads to write into")
        C0 = x.v.shape[3]
        growth = {n: self.w[f"{n}_conv1"][0].shape[3] for n in trunk_blocks(num_rrdb)}

        def forward(name, F, nxt, r_in, a5, bx):
            g = growth[name]
            for k in range(1, 5):
                kk, bb = self.w[f"{name}_conv{k}"]
                cin = C0 + (k - 1) * g
                ctx.conv2d_dev_view_bf16(F, 0, cin, dev(kk), dev(bb), g, F, cin, act="relu")
            k5, b5 = self.w[f"{name}_conv5"]
            skip2, beta2 = (None, 0.0) if r_in is None else ((r_in, 0), 1.0)
            ctx.conv2d_dev_view_bf16(F, 0, C0 + 4 * g, dev(k5), dev(b5), C0, nxt, 0, alpha=a5, skip1=(F, 0), beta1=bx, skip2=skip2, beta2=beta2)

        def backward(b, d, name, F, dY, a5, bx, rec):
            B, H, W, Ct = F.shape
            g = growth[name]
            G = ctx.empty((B, H, W, Ct), F.dtype)
            ctx.conv2d_dev_view_bf16(dY, 0, C0, dev(self.w[f"{name}_conv5"][0]), None, Ct, G, 0, rot=True, alpha=a5)       # fills every channel of G
            if rec:
                rec((f"G_{b}_{d}_s5", G.clone()))
            dz = ctx.empty((B, H, W, 4 * g), F.dtype)           # dz_k is slice k - 1
            dX = ctx.empty((B, H, W, C0), F.dtype)
            for k in range(4, 0, -1):
                kk = dev(self.w[f"{name}_conv{k}"][0])
                cin = C0 + (k - 1) * g
                ctx.eltwise_view_bf16(L.ELT_RELU_BWD, G, cin, F, cin, dz, (k - 1) * g, g)                          # slice k of G is complete: convs k+1..5 have added to it
                if k > 1:
                    ctx.conv2d_dev_view_bf16(dz, (k - 1) * g, g, kk, None, cin, G, 0, rot=True, skip1=(G, 0), beta1=1.0)       # G[..., :cin] += dgrad
                    if rec:
                        rec((f"G_{b}_{d}_s{k}", G.clone()))
                else:
                    ctx.conv2d_dev_view_bf16(dz, 0, g, kk, None, C0, dX, 0, rot=True, skip1=(G, 0), beta1=1.0, skip2=(dY, 0), beta2=bx)
            return dz, dX
        return self._trunk_mixed(x, num_rrdb, tape, growth, forward, backward)

    def pack_lds(self, num_rrdb):
        """(fwd, bias, bwd, {block name: row}): the trunk's dense blocks packed for the LDS-resident kernels from the tape's device weights, by one launch."""
        trunk_layers_lds(self.w, num_rrdb)
        plan = lds_pack_plan(self.ctx, lambda n: tuple(self._dev(a) for a in self.w[n]), num_rrdb)
        self.ctx.dense_block_pack_dev(*plan[:4])
        return plan[1:]

    def trunk_lds(self, x, num_rrdb, tape=None):
        """_trunk_mixed at growth width 8 with every dense block as ONE forward and ONE backward kernel on an LDS-resident image: the same contract,
        the same stored tensors (F per block, dz, dX) and the same grouped weight-gradient launch; G, the gradient of F, never reaches HBM.  `tape` as there; the
        G_b_d_s* stages are recorded only with `trunk_stages` (the kernel's stage dump; channels >= cin_k of stage k hold dz already selected)."""
        ctx = self.ctx
        if self.flat is None and self.wgrad:
            raise ValueError("trunk_lds: the weight gradients need a FlatGrads to write into")
        lds_patch_check(ctx, x.v.shape[1], x.v.shape[2])
        fwd, bias, bwd, row = self.lds_packs if self.lds_packs is not None else self.pack_lds(num_rrdb)

        def forward(name, F, nxt, r_in, a5, bx):
            i = row[name]
            skip2, beta2 = (None, 0.0) if r_in is None else ((r_in, 0), 1.0)
            ctx.dense_block_fwd_bf16(fwd[i], bias[i], F, nxt, skip2=skip2, alpha=a5, beta1=bx, beta2=beta2)

        def backward(b, d, name, F, dY, a5, bx, rec):
            B, H, W, Ct = F.shape
            dz = ctx.empty((B, H, W, 32), F.dtype)              # dz_k is slice k - 1
            dX = ctx.empty((B, H, W, Ct - 32), F.dtype)
            stages = ctx.empty((4, B, H, W, Ct), F.dtype) if rec and self.trunk_stages else None
            ctx.dense_block_bwd_bf16(bwd[row[name]], dY, F, a5, bx, dz, dX, stages=stages)
            if stages is not None:
                for j, k in enumerate((5, 4, 3, 2)):
                    rec((f"G_{b}_{d}_s{k}", stages[j]))
            return dz, dX
        return self._trunk_mixed(x, num_rrdb, tape, dict.fromkeys(trunk_blocks(num_rrdb), 8), forward, backward)

    def axpby(self, a, b, alpha, beta):
        y = Var(self.ctx.eltwise(L.ELT_AXPBY, a.v, b.v, alpha, beta))

        def bwd():
            if y.g is None:
                return
            self._acc(a, y.g if alpha == 1.0 else self.ctx.eltwise(L.ELT_AXPBY, y.g, None, alpha, 0.0))
            self._acc(b, y.g if beta == 1.0 else self.ctx.eltwise(L.ELT_AXPBY, y.g, None, beta, 0.0))
        self.ops.append(bwd)
        return y

    def attention(self, x, name):
        """SelfAttention.call (ESRGAN_model.py:48-70): s = g f^T, beta = softmax(s), o = beta h, y = x + v(o).  attention_impl "materialised" keeps
        beta as a [B,N,N] tensor; "streamed" keeps o and one softmax statistic per query and recomputes beta tile by tile in the backward kernels."""
        ctx = self.ctx
        B, H, W, C = x.v.shape
        N = H * W
        f, g, h = self.conv(x, name + "_f"), self.conv(x, name + "_g"), self.conv(x, name + "_h")
        f3, g3, h3 = f.v.reshape(B, N, -1), g.v.reshape(B, N, -1), h.v.reshape(B, N, -1)
        if self.attention_impl == "streamed":
            o3, lse = ctx.attention_fwd_lse(g3, f3, h3)                       # [B,N,32], [B,N]
            o = Var(o3.reshape(B, H, W, -1))

            def bwd():
                if o.g is None:
                    return
                dg, df, dh = ctx.attention_bwd(g3, f3, h3, o3, o.g.reshape(B, N, -1), lse)
                self._acc(h, dh.reshape(h.v.shape))
                self._acc(g, dg.reshape(g.v.shape))
                self._acc(f, df.reshape(f.v.shape))
        else:
            beta = ctx.softmax_rows_(ctx.matmul(g3, f3, trans_b=True))            # [B,N,N]
            o = Var(ctx.matmul(beta, h3).reshape(B, H, W, -1))

            def bwd():
                if o.g is None:
                    return
                do = o.g.reshape(B, N, -1)
                dbeta = ctx.matmul(do, h3, trans_b=True)                           # [B,N,N]
                self._acc(h, ctx.matmul(beta, do, trans_a=True).reshape(h.v.shape))
                ds = ctx.softmax_bwd(beta, dbeta)
                self._acc(g, ctx.matmul(ds, f3).reshape(g.v.shape))
                self._acc(f, ctx.matmul(ds, g3, trans_a=True).reshape(f.v.shape))
        self.ops.append(bwd)
        ov = self.conv(o, name + "_v")
        return self.axpby(x, ov, 1.0, 1.0)

    def pick2(self, x):
        y = Var(self.ctx.spatial_op(L.SP_PICK2, x.v))
        H, W = x.v.shape[1:3]

        def bwd():
            if y.g is not None:
                self._acc(x, self.ctx.zero_insert2(y.g, H, W))
        self.ops.append(bwd)
        return y

    def maxpool(self, x):
        y = Var(self.ctx.spatial_op(L.SP_MAXPOOL2, x.v))

        def bwd():
            if y.g is not None:
                self._acc(x, self.ctx.maxpool2_bwd(x.v, y.g))
        self.ops.append(bwd)
        return y

    def backward(self):
        for op in reversed(self.ops):
            op()
        self.ops = []


# ----------------------------------------------------------------------------------------------------------------- networks
# dense blocks on one virtual-concat buffer per block (Tape.dense_block) where the growth width is a whole number of the fp32 conv's 16-channel chunks
# (G = 32: yes; the notebook's G = 8: the cat path)


def generator_forward(t, x, scale, num_rrdb, attention=True):
    """ESRGAN_model.py:303-345 on the tape; x Var [B,h,w,3] in [-1,1]."""
    x = t.conv(x, "initial_conv")
    trunk = x
    if t.trunk_dtype == "bf16":
        x, num_rrdb = (t.trunk_lds if t.dense_block_impl == "lds" else t.trunk_bf16)(x, num_rrdb), 0
    for b in range(num_rrdb):
        r_in = x
        for d in (1, 2, 3):
            n = f"rrdb_{b}_dense{d}"
            growth = t.w[f"{n}_conv1"][0].shape[3]
            if growth % 16 == 0:
                x = t.dense_block(x, n, growth)
                continue
            feats = [x]
            for k in range(1, 5):
                feats.append(t.conv(t.cat(feats), f"{n}_conv{k}", act="relu"))
            x = t.axpby(x, t.conv(t.cat(feats), f"{n}_conv5"), 1.0, 0.2)
        x = t.axpby(r_in, x, 1.0, 0.2)
    x = t.axpby(trunk, t.conv(x, "trunk_conv"), 1.0, 1.0)
    if attention:
        x = t.attention(x, "self_attention_trunk")
    s, i = scale, 0
    while s > 1:
        x = t.conv(x, f"upsample_{i}_conv", act="lrelu", d2s=2)
        if i == 0 and attention:
            x = t.attention(x, "self_attention_upsample_0")
        s >>= 1
        i += 1
    x = t.conv(x, "final_conv1", act="relu")
    return t.conv(x, "final_conv2", act="tanh")


DISC_STRIDES = [1, 2, 1, 2, 1, 2]
DISC_LAYERS = [f"disc_conv{i}" for i in range(1, 7)] + ["disc_dense1", "disc_output"]


def spectral_normalize(kernel, u):
    """tfa SpectralNormalization.normalize_weights, one power iteration -> (kernel / sigma, new u)."""
    w = kernel.reshape(-1, kernel.shape[-1]).astype(np.float64)
    u = u.reshape(1, -1).astype(np.float64)
    l2n = lambda a: a / np.sqrt(max(float(np.sum(a * a)), 1e-12))
    v = l2n(u @ w.T)
    u = l2n(v @ w)
    sigma = float((v @ w @ u.T).item())
    return (kernel / np.float32(sigma)).astype(np.float32), u.astype(np.float32)


def disc_trunk(t, x):
    """The six convs of ESRGAN_model.py:347-377 on the tape (the strided ones as a stride-1 conv and a pick of every second pixel)
    -> Var [B,H/8,W/8,256], the map the head pools."""
    h = x
    for i, st in enumerate(DISC_STRIDES):
        h = t.conv(h, f"disc_conv{i + 1}", act="lrelu")
        if st == 2:
            h = t.pick2(h)
    return h


VGG19_CFG = [(1, 2, 64), (2, 2, 128), (3, 4, 256), (4, 4, 512), (5, 4, 512)]


def vgg19_features(t, x):
    """ESRGAN_model.py:379-408 on the tape (frozen: run it on a Tape with wgrad=False); x Var in [-1,1]."""
    ctx = t.ctx
    pre = Var(ctx.spatial_op(L.SP_VGG_PREPROCESS, x.v))

    def bwd():
        if pre.g is not None and x.need:      # (x+1)*127.5 with RGB -> BGR: the adjoint flips the channels back and scales
            t._acc(x, ctx.eltwise(L.ELT_AXPBY, torch.flip(pre.g, dims=[-1]).contiguous(), None, 127.5, 0.0))
    t.ops.append(bwd)
    h = pre
    for blk, n, _ in VGG19_CFG:
        for k in range(1, n + 1):
            h = t.conv(h, f"block{blk}_conv{k}", act="relu")
            if (blk, k) == (5, 4):
                return h
        h = t.maxpool(h)
    return h


PERCEPTUAL_DTYPES = ("f32", "bf16")


def check_perceptual_dtype(value):
    """The arithmetic of _train_step's VGG19 perceptual term: "f32" (the reference's) or "bf16" (PerceptualBf16)."""
    if value not in PERCEPTUAL_DTYPES:
        raise ValueError(f"perceptual_dtype must be one of {PERCEPTUAL_DTYPES}, got {value!r}")
    return value


SMALL_CONV_WINS_TINY, SMALL_CONV_WINS_PIXELS, SMALL_CONV_WINS_TOTAL = 9, 36, 1008


def small_conv_wins(h, w, cin, cout, images):
    """Where sr_conv3x3_small_bf16 is the fastest of the three conv routes per launch (tools/bench_perceptual_mixed.py, profiles/perceptual_mixed_aba.txt,
    DESIGN.md 3.29), channel counts multiples of 32: images of at most 3 x 3 pixels at any batch (measured from 144 to 2304 pixels per call: 0.29-0.60 of the
    best other route), and images of at most 6 x 6 pixels while the call has at most 1008 pixels (measured on 6 x 6 at 288 .. 1008: 0.68-0.78; at 1152 and 2304,
    where the grid no longer fits the CUs in one round, 1.05-1.11).  Image sizes between 3 x 3 and 6 x 6 were not measured: they take the 6 x 6 rule.  The
    kernel itself takes images up to 144 pixels and any batch; on 12 x 12 images sr_conv2d_dev_bf16 measured 1.35-2.96 x faster and keeps those calls."""
    if cin % 32 or cout % 32:
        return False
    return h * w <= SMALL_CONV_WINS_TINY or (h * w <= SMALL_CONV_WINS_PIXELS and images * h * w <= SMALL_CONV_WINS_TOTAL)


def perceptual_routes(H, W, B=None):
    """The sixteen convs of the extractor on a batch of B HR patches of H x W -> [(layer, h, w, cin, cout, forward route, pooled, input-gradient route)]: the
    layer's image size and channels, the kernel of its forward over the 2 B images [fake | hr] and of its input gradient over the B images of fake -- "small"
    (sr_conv3x3_small_bf16 where small_conv_wins) or "conv2d" (sr_conv2d_dev_bf16) -- and whether a 2 x 2 max-pool follows.  B None: the image-size rule alone."""
    out, h, w, cin = [], int(H), int(W), 3
    fwd_images, bwd_images = (1, 1) if B is None else (2 * int(B), int(B))
    for blk, n, cout in VGG19_CFG:
        if h < 1 or w < 1:
            raise ValueError(f"perceptual_dtype='bf16': HR patches of {H} x {W} leave no pixel for block{blk} of VGG19")
        for k in range(1, n + 1):
            route = lambda images, ci, co: "small" if small_conv_wins(h, w, ci, co, images) else "conv2d"
            out.append((f"block{blk}_conv{k}", h, w, cin, cout, route(fwd_images, cin, cout), k == n and blk < 5, route(bwd_images, cout, cin)))
            cin = cout
        h, w = h // 2, w // 2
    return out


class PerceptualBf16:
    """perceptual_dtype="bf16": mean((VGG19(fake) - VGG19(hr))^2) at block5_conv4 and its gradient w.r.t. fake in bf16 mixed precision -- fp32
    master weights rounded to bf16 once, bf16 activations and activation gradients, fp32 accumulation and epilogues, one rounding per stored tensor.  ONE forward
    over the batch [fake | hr], one loss launch pair, one backward over the fake half; every ReLU gradient is a select fused into the kernel that writes the tensor
    (the small-image conv's mask operand, the pool's backward, the loss) except behind an sr_conv2d_dev_bf16 input gradient that follows another conv.
    `bucket`: the frozen VGG19's ParamBucket.  The packs of the small-image kernel live here for as long as the weights do; the few large-image layers are listed
    by pack_uses() for the step's sr_conv_prepack_bf16."""

    def __init__(self, ctx, bucket):
        self.ctx, self.dev = ctx, bucket.dev
        k, _ = self.dev["block1_conv1"]
        self.k6 = torch.cat([k, k], dim=2).contiguous()        # the hi + lo entry: the layer's kernel twice along Cin
        self._handles = {}
        self.tape = None                                        # tests: a list here receives (name, tensor) for every tensor the branch stores

    def handle(self, name, rot):
        if (name, rot) not in self._handles:
            self._handles[(name, rot)] = self.ctx.conv3x3_small_pack(self.dev[name][0], rot=rot)
        return self._handles[(name, rot)]

    def pack_uses(self, B, H, W):
        """pack_list entries of the calls sr_conv2d_dev_bf16 runs on a batch of B HR patches of H x W: forward and input-gradient uses."""
        uses = []
        for i, (name, _, _, _, _, route, _, route_bwd) in enumerate(perceptual_routes(H, W, B)):
            kd, bd = self.dev[name]
            if i == 0:
                uses += [(self.k6, bd, False), (kd, None, True)]
                continue
            uses += [(kd, bd, False)] if route == "conv2d" else []
            uses += [(kd, None, True)] if route_bwd == "conv2d" else []
        return uses

    def _keep(self, name, t):
        if self.tape is not None:
            self.tape.append((name, t))
        return t

    def __call__(self, hr_t, fake):
        """hr_t, fake fp32 [B,H,W,3] in [-1,1] -> (perc fp32 [1] device tensor, d perc / d fake fp32 [B,H,W,3])."""
        ctx, dev = self.ctx, self.dev
        B, H, W, _ = fake.shape
        routes = perceptual_routes(H, W, B)
        h = self._keep("pre", ctx.vgg_preprocess_bf16(fake, hr_t))
        acts = []
        for i, (name, _, _, _, cout, route, pooled, _) in enumerate(routes):
            kd, bd = dev[name]
            if i == 0:
                h = ctx.conv2d_dev_bf16(h, self.k6, bd, cout, act="relu")
            elif route == "small":
                h = ctx.conv3x3_small_bf16(h, None, bd, cout, act="relu", packed=self.handle(name, False))
            else:
                h = ctx.conv2d_dev_bf16(h, kd, bd, cout, act="relu")
            acts.append(self._keep(name, h))
            if pooled:
                h = self._keep(name + "_pool", ctx.maxpool2_bf16(h))
        perc, g = ctx.mse_grad_bf16(h)
        self._keep("d_" + routes[-1][0], g)
        for i in range(len(routes) - 1, 0, -1):                 # g: the gradient of layer i's pre-activation -> of layer i - 1's, over the fake half
            name, _, _, cin, _, _, _, route = routes[i]
            prev, prev_pooled = routes[i - 1][0], routes[i - 1][6]
            a_prev = acts[i - 1][:B]
            if route == "small":
                g = ctx.conv3x3_small_bf16(g, None, None, cin, rot=True, mask=None if prev_pooled else a_prev, packed=self.handle(name, True))
            else:
                g = ctx.conv2d_dev_bf16(g, dev[name][0], None, cin, rot=True)
                if not prev_pooled:
                    self._keep("dx_" + name, g)
                    g = ctx.relu_bwd_bf16(g, a_prev)
            if prev_pooled:
                self._keep("d_" + prev + "_pool", g)
                g = ctx.maxpool2_bwd_bf16(a_prev, g)
            self._keep("d_" + prev, g)
        dv = self._keep("d_pre", ctx.conv2d_dev_bf16(g, dev["block1_conv1"][0], None, 3, rot=True))
        return perc, ctx.vgg_preprocess_bwd(dv)


def bce_mean(target, p, eps=1e-7):
    """mean(keras.backend.binary_crossentropy) on probabilities and its gradient w.r.t. p (clip passes the gradient inside [eps, 1-eps])."""
    pc = np.clip(p, eps, 1.0 - eps)
    loss = float(np.mean(-(target * np.log(pc + eps) + (1.0 - target) * np.log(1.0 - pc + eps))))
    inside = ((p >= eps) & (p <= 1.0 - eps)).astype(np.float64)
    dp = -(target / (pc + eps) - (1.0 - target) / (1.0 - pc + eps)) * inside / p.size
    return loss, dp


def staircase_lr(lr0, step, decay_steps=10000, decay_rate=0.5):
    """ExponentialDecay(staircase=True) (ESRGAN_model.py:176-195)."""
    return lr0 * decay_rate ** (step // decay_steps)


# ----------------------------------------------------------------------------------------------------------------- the discriminator
# One class per home of the discriminator's state; ESRGANTrainer.train_step sees the same surface of both:
#   weights, u, opt, params: host arrays {layer: (kernel, bias)} / {layer: [1,Cout]} to read and to write (a write keeps Adam's moments), the
#       optimiser, and the parameters' flat device bucket or None;
#   critic(x, target, wgrad, masks, devcache) -> loss: one training=True call -- renormalise every kernel, trunk, head, BCE against `target`,
#       backward (x.g is set when x.need); with wgrad the call's parameter gradients are added to the step's accumulator;
#   update(lr, allreduce, allreduce_flat): average the accumulated gradient over the ranks, apply Adam, keep the gradient for last_grads().
class HostDiscriminator:
    """discriminator="host": weights, u and Adam in NumPy.  The six convs run on the device -- every renormalised kernel is uploaded --, the
    [B,256] head, its BCE and their backward on the host in fp64; critic's loss is a Python float."""

    params = None

    def __init__(self, ctx, weights, u, lr):
        self.ctx, self.weights, self.u = ctx, weights, u
        self.opt = Adam(weights, lr, epsilon=1e-7)
        self._grads = self._applied = None

    def critic(self, x, target, wgrad=True, masks=None, devcache=None):
        ctx, w = self.ctx, self.weights
        for n in DISC_LAYERS:                               # in place: `weights` stays the dict its owner handed in
            k, self.u[n] = spectral_normalize(w[n][0], self.u[n])
            w[n] = (k, w[n][1])
        t = Tape(ctx, w, wgrad=wgrad, devcache=devcache)
        t.masks = masks
        h = disc_trunk(t, x)
        B, H, W, C = h.v.shape
        g = ctx.spatial_op(L.SP_GAP, h.v).cpu().numpy().astype(np.float64)          # [B,256]: the head runs on the host
        k1, b1 = (a.astype(np.float64) for a in w["disc_dense1"])
        k2, b2 = (a.astype(np.float64) for a in w["disc_output"])
        z1 = g @ k1 + b1
        a1 = np.where(z1 > 0, z1, 0.2 * z1)
        z2 = a1 @ k2 + b2
        p = 1.0 / (1.0 + np.exp(-z2))
        loss, dp = bce_mean(np.full_like(p, target), p)
        dz2 = dp * p * (1.0 - p)
        if wgrad:
            t.grads["disc_output"] = [a1.T @ dz2, dz2.sum(axis=0)]
        da1 = dz2 @ k2.T
        dz1 = np.where(z1 > 0, da1, 0.2 * da1)
        if wgrad:
            t.grads["disc_dense1"] = [g.T @ dz1, dz1.sum(axis=0)]
        dg = (dz1 @ k1.T) / float(H * W)                                             # GAP backward: spread over the H x W map
        h.g = ctx.to_device(dg.astype(np.float32))[:, None, None, :].expand(B, H, W, C).contiguous()
        t.backward()
        if wgrad:
            new, acc = self._host(t.grads), self._grads
            self._grads = new if acc is None else {n: (acc[n][0] + new[n][0], acc[n][1] + new[n][1]) for n in acc}
        return loss

    @staticmethod
    def _host(grads):
        """{layer: [dk, db]} (device tensors; host arrays for the dense head) -> host fp32 arrays; the device ones cross PCIe as ONE flat buffer."""
        out = {n: [None if isinstance(a, torch.Tensor) else np.asarray(a, np.float32) for a in pair] for n, pair in grads.items()}
        dev = [(n, s) for n in out for s in (0, 1) if out[n][s] is None]
        flat, o = torch.cat([grads[n][s].reshape(-1) for n, s in dev]).cpu().numpy(), 0
        for n, s in dev:
            t = grads[n][s]
            out[n][s] = flat[o:o + t.numel()].reshape(tuple(t.shape))
            o += t.numel()
        return {n: tuple(pair) for n, pair in out.items()}

    def update(self, lr, allreduce=None, allreduce_flat=None):
        """The host discriminator's gradients are a dict and take the dict route only: with `allreduce_flat` alone they stay unreduced."""
        grads, self._grads = self._grads, None
        if allreduce is not None:
            grads = allreduce(grads)
        self.opt.lr = lr
        self.weights = self.opt.apply(self.weights, grads)
        self._applied = grads

    def last_grads(self):
        return self._applied


class DeviceDiscriminator:
    """discriminator="device": the parameters as ONE flat device bucket in DISC_LAYERS order (the head's four arrays are its last 66 049
    values), u as one flat device tensor (the layers' [1,Cout] vectors one after the other: 961 floats), Adam's moments beside them.
    `weights`, `u` and last_grads() are host arrays refreshed from the device when somebody reads them; critic's loss is a one-element
    device tensor, a slot of `_losses`, good until the same kind of call comes again."""

    def __init__(self, ctx, weights, u, lr):
        self.ctx = ctx
        self.params = ParamBucket(ctx, {n: weights[n] for n in DISC_LAYERS})
        self._u_host = np.concatenate([u[n].ravel() for n in DISC_LAYERS]).astype(np.float32)
        self._u_views, o = {}, 0
        for n in DISC_LAYERS:
            self._u_views[n] = self._u_host[o:o + u[n].size].reshape(1, -1)
            o += u[n].size
        self.u_flat, self._u_stale = ctx.to_device(self._u_host), False
        self._sn_table, u_len = ctx.spectral_norm_table(self.params, DISC_LAYERS)
        assert u_len == self._u_host.size
        self.opt = DeviceAdam(ctx, self.params.flat, lr, epsilon=1e-7)
        self._head_off = self.params.flat.numel() - ctx.DISC_HEAD_PARAMS
        self._head_g = ctx.empty((ctx.DISC_HEAD_PARAMS,))                  # the head's slice of the gradient bucket: the first critic stores, the next add
        self._losses = ctx.empty((3,))                                     # BCE of the step's first wgrad critic, of its later ones, of the one without wgrad
        self._grads = self._applied = None

    @property
    def weights(self):
        return self.params.host()

    @weights.setter
    def weights(self, weights):                            # ESRGAN.set_loss_network_weights on a live trainer: Adam's moments and u stay
        self.params.load({n: weights[n] for n in DISC_LAYERS})

    @property
    def u(self):
        if self._u_stale:
            self._u_host[:] = self.u_flat.cpu().numpy()
            self._u_stale = False
        return self._u_views

    @u.setter
    def u(self, u):
        self._u_host[:] = np.concatenate([np.asarray(u[n], np.float32).ravel() for n in DISC_LAYERS])
        self.u_flat.copy_(self.ctx.to_device(self._u_host))
        self._u_stale = False

    def critic(self, x, target, wgrad=True, masks=None, devcache=None):
        """One launch renormalises the eight kernels where they lie, the six convs run on the bucket's views (`devcache` is not needed), the
        head op writes the BCE and d loss / d h, and the tape runs back."""
        ctx, P = self.ctx, self.params
        ctx.spectral_norm_bucket(P.flat, self.u_flat, self._sn_table)
        P.stale = self._u_stale = True
        t = Tape(ctx, P.arrays, wgrad=wgrad, devcache=dict(P.devcache))
        t.masks = masks
        h = disc_trunk(t, x)
        accumulate = wgrad and self._grads is not None
        slot = int(accumulate) if wgrad else 2
        loss = self._losses[slot:slot + 1]
        _, h.g = ctx.disc_head_step(h.v, P.flat[self._head_off:], target, loss, self._head_g if wgrad else None, accumulate)
        t.backward()
        if wgrad:                                          # the passes' gradients meet in one flat bucket (the head's through its accumulate flag)
            g = P.gather(t.grads)
            self._grads = ctx.eltwise(L.ELT_AXPBY, self._grads, g, 1.0, 1.0) if accumulate else g
        return loss

    def update(self, lr, allreduce=None, allreduce_flat=None):
        """The flat gradient bucket takes the generator's two routes: `allreduce_flat` where it lies, else `allreduce` as a host dict."""
        P = self.params
        d_flat, self._grads = self._grads, None
        d_flat[self._head_off:].copy_(self._head_g)
        if allreduce_flat is not None:
            d_flat = allreduce_flat(d_flat)
        elif allreduce is not None:                        # dict route (host): the 2-rank gloo tests
            d_flat = self.ctx.to_device(P.flatten(allreduce(P.split(d_flat.cpu().numpy()))))
        self.opt.lr = lr
        self.opt.apply(P.flat, d_flat)
        P.stale = True
        self._applied = d_flat

    def last_grads(self):
        if isinstance(self._applied, torch.Tensor):        # downloaded on first use
            self._applied = self.params.split(self._applied.cpu().numpy())
        return self._applied


# ----------------------------------------------------------------------------------------------------------------- the step
def _device_batch(ctx, images):
    """A step's image batch -> fp32 device tensor: a host array is uploaded, a tensor already on the device (a batch cut from
    sr355.patches.PatchPairs) is taken as it is."""
    if isinstance(images, torch.Tensor):
        return ctx.to_device(images, torch.float32)
    return ctx.to_device(np.asarray(images, np.float32))


def _floats(values):
    """Python floats and one-element device tensors -> Python floats; the tensors come over in ONE read."""
    dev = [v for v in values if isinstance(v, torch.Tensor)]
    read = iter(torch.cat(dev).cpu().numpy())
    return [float(next(read)) if isinstance(v, torch.Tensor) else v for v in values]


def _discriminator_attr(name):
    """ESRGANTrainer's `dw` / `u` / `d_opt` / `d_params`: the discriminator object's attribute; None on a generator-only trainer."""
    return property(lambda self: getattr(self.disc, name, None), lambda self, value: setattr(self.disc, name, value))


class ESRGANTrainer:
    """Holds generator / discriminator / VGG19 weights, the SN vectors u, the two Adam states and the step counter.  The discriminator's share
    lives in `disc`, a HostDiscriminator (discriminator="host", the default) or a DeviceDiscriminator ("device"); `dw`, `u`, `d_opt` and
    `d_params` are its `weights`, `u`, `opt` and `params`."""

    dw, u, d_opt, d_params = (_discriminator_attr(name) for name in ("weights", "u", "opt", "params"))

    def __init__(self, ctx, g_weights, d_weights, vgg_weights, scale, num_rrdb, attention=True, g_lr=1e-4, d_lr=1e-5, u_seed=0, allreduce=None,
                 allreduce_flat=None, discriminator="host", attention_impl="materialised", train_dtype="f32", dense_block_impl="layers", perceptual_dtype="f32"):
        if discriminator not in ("host", "device"):
            raise ValueError(f"discriminator must be 'host' or 'device', got {discriminator!r}")
        self.perceptual_dtype = check_perceptual_dtype(perceptual_dtype)      # the VGG19 perceptual term of train_step (PerceptualBf16); refused before any upload
        # what the taped training pass stores inside the RRDB trunk (Tape.trunk_bf16 / trunk_lds); refused before anything is uploaded or launched
        self.train_dtype = check_train_dtype(train_dtype)
        self.dense_block_impl = check_dense_block_impl(dense_block_impl, train_dtype)
        walk = trunk_layers_lds if self.dense_block_impl == "lds" else trunk_layers
        self._trunk = set(walk(g_weights, num_rrdb)) if train_dtype == "bf16" else set()
        self.attention_impl = check_attention_impl(attention_impl)      # the generator tape's SelfAttention core (Tape.attention)
        self.ctx, self.scale, self.nb, self.att = ctx, scale, num_rrdb, attention
        self.discriminator = discriminator
        # Generator (16.9 M parameters at the default depth): resident on the device as ONE flat fp32 bucket with its Adam moments beside it;
        # the per-layer tensors the tape multiplies with are views of it, the gradients are gathered into a bucket of the same order, and
        # the optimiser is one fused kernel (round 2: NumPy Adam on the host, 65 ms of a 258 ms step, plus 70 MB each way over PCIe).
        # `self.gw` stays available as host arrays: they are refreshed from the device when somebody reads them.
        self.g_params = ParamBucket(ctx, g_weights)
        self.vw = vgg_weights
        self._vgg = self._vgg_src = None                   # the frozen VGG19 on the device (a bucket of self.vw), uploaded by train_step
        self._perc16 = None                                # perceptual_dtype="bf16": the branch and its packed kernels, remade when the VGG19 weights are replaced
        self.g_lr0, self.d_lr0 = g_lr, d_lr
        self.g_opt = DeviceAdam(ctx, self.g_params.flat, g_lr, epsilon=1e-7)
        # d_weights / vgg_weights None: a generator-only trainer (pixel_step: sr355.recipes' L1 fit); it has no discriminator object and train_step refuses
        self.disc = None
        if d_weights is not None:
            dw = {n: (np.asarray(k, np.float32), np.asarray(b, np.float32)) for n, (k, b) in d_weights.items()}
            rng = np.random.default_rng(u_seed)           # tfa initialises u ~ TruncatedNormal(stddev 0.02), shape [1, Cout]
            u = {n: np.clip(rng.normal(0, 0.02, (1, dw[n][0].shape[-1])), -0.04, 0.04).astype(np.float32) for n in DISC_LAYERS}
            self.disc = (DeviceDiscriminator if discriminator == "device" else HostDiscriminator)(ctx, dw, u, d_lr)
        self.step = 0
        # data parallel: `allreduce` = callable(dict of host grads) -> averaged dict (the host discriminator's, whose spectral normalisation lives
        # there); `allreduce_flat` = callable(flat device tensor) -> averaged tensor for the generator's bucket (RCCL reduces it where it
        # lies).  With only `allreduce` given the generator's bucket takes the dict route too (the gloo CPU tests).  The device discriminator's
        # gradients are a flat device bucket as well and take the same two routes as the generator's.
        self.allreduce, self.allreduce_flat = allreduce, allreduce_flat
        self.collect_masks = False                         # tests: keep the activation branches of a step's forward passes in last_masks (oracle/train.py _masked_act)
        self.last_masks = self.last_dy = self.last_fake = None
        self._last = None
        self._packs = {}
        self._lds_packed = False

    @contextlib.contextmanager
    def _prepacked(self, with_vgg, hr_shape=None):
        """Pack every generator (and VGG19) conv's weights for its forward and its input-gradient use by ONE launch (sr_conv_prepack; ~700 of a step's ~800
        per-use packs, 3.5 ms of 53) for the duration of the block.  The discriminator's kernels are renormalised inside the step and keep packing per use.
        The list is dropped when the block ends: nobody else on this context may meet a pack older than the weights.
        perceptual_dtype="bf16" (hr_shape: the step's (B, H, W) of HR patches): the VGG19 layers stand in no fp32 list; the calls of the small-image kernel keep
        the handles PerceptualBf16 packed once, the others join the step's bf16 list."""
        vgg16 = with_vgg and self.perceptual_dtype == "bf16"
        if with_vgg not in self._packs:
            uses = []
            for params in [self.g_params] + ([self._vgg] if with_vgg and not vgg16 else []):
                for n, (kd, bd) in params.dev.items():
                    if params is self.g_params and n in self._trunk:      # train_dtype="bf16": the trunk's layers stand in the bf16 list only
                        continue
                    if kd.dim() == 4 and kd.shape[0] == kd.shape[1] and kd.shape[0] in (1, 3):
                        uses += [(kd, bd, False), (kd, None, True)]
            self._packs[with_vgg] = self.ctx.pack_list(uses)
        lds = self.dense_block_impl == "lds"
        trunk16 = bool(self._trunk) and not lds
        key16 = ("bf16", tuple((r[5], r[7]) for r in perceptual_routes(hr_shape[1], hr_shape[2], hr_shape[0]))) if vgg16 else "bf16"      # what changes the list: which calls stay on sr_conv2d_dev_bf16
        if (trunk16 or vgg16) and key16 not in self._packs:   # every trunk kernel rounded to bf16 once per step, for its forward and its input-gradient use
            dev = self.g_params.dev
            uses16 = [u for n in dev if n in self._trunk for u in ((dev[n][0], dev[n][1], False), (dev[n][0], None, True))] if trunk16 else []
            self._packs[key16] = self.ctx.pack_list(uses16 + (self._perc16.pack_uses(*hr_shape) if vgg16 else []))
        if lds and "lds" not in self._packs:                  # dense_block_impl="lds": the trunk's blocks as fragments of the LDS-resident kernels, in buffers of the trainer's
            self._packs["lds"] = lds_pack_plan(self.ctx, self.g_params.dev.__getitem__, self.nb)
        self.ctx.conv_prepack(self._packs[with_vgg])
        if lds:
            self.ctx.dense_block_pack_dev(*self._packs["lds"][:4])     # ... rounded to bf16 once per step, by one launch
            self._lds_packed = True
        if trunk16 or vgg16:
            self.ctx.conv_prepack_bf16(self._packs[key16])
        try:
            yield
        finally:
            self.ctx.conv_prepack(None)
            self._lds_packed = False                          # the weights move on in the step's last lines: a tape made outside the block packs for itself
            if trunk16 or vgg16:
                self.ctx.conv_prepack_bf16(None)

    @property
    def gw(self):
        """{layer: (kernel, bias)} host copies of the generator's parameters (refreshed from the device bucket when it has moved on)."""
        return self.g_params.host()

    @gw.setter
    def gw(self, weights):
        self.load_generator_weights(weights)

    def load_generator_weights(self, weights, reset_optimizer=True):
        """Replace the generator's parameters (ESRGAN.set_weights / load after the trainer exists): copies into the device bucket in
        parameter order; by default Adam's moments and step count start over, as a freshly compiled Keras model's would."""
        self.g_params.load(weights)
        if reset_optimizer:
            self.g_opt.m.zero_()
            self.g_opt.v.zero_()
            self.g_opt.t = 0

    def generator_tape(self, wgrad=True):
        """A tape over the generator's device-resident parameters (no upload, no host copy).  With train_dtype="bf16" the taped training pass (wgrad) runs the
        trunk in bf16 and collects every gradient in one flat bucket; the forward-only tape stays fp32."""
        bf16 = wgrad and self.train_dtype == "bf16"
        lds = bf16 and self.dense_block_impl == "lds"
        t = Tape(self.ctx, self.g_params.arrays, wgrad=wgrad, devcache=dict(self.g_params.devcache), attention_impl=self.attention_impl,
                 trunk_dtype="bf16" if bf16 else "f32", flat_grads=FlatGrads(self.g_params) if bf16 else None, dense_block_impl="lds" if lds else "layers")
        if lds and self._lds_packed:                           # inside _prepacked: this step's pack
            t.lds_packs = self._packs["lds"][1:]
        return t

    def _check_patch(self, lr_images):
        """dense_block_impl="lds": a batch whose patch the LDS-resident kernels cannot take is refused before the step touches anything."""
        if self.dense_block_impl == "lds":
            shape = lr_images.shape if hasattr(lr_images, "shape") else np.shape(lr_images)
            lds_patch_check(self.ctx, int(shape[1]), int(shape[2]))

    @property
    def last_grads(self):
        """{"g": {layer: (dk, db)}, "d": {...}} host arrays of the last step (the generator's, and a device discriminator's, are downloaded on first use)."""
        if self._last is None:
            return None
        if "g" not in self._last:
            full = self.g_params.split(self._last.pop("g_flat").cpu().numpy())
            self._last["g"] = {n: full[n] for n in full if n in self._last["g_names"]}     # only the variables the loss reaches, as Keras reports them
        self._last["d"] = self.disc.last_grads()
        return self._last

    def _update_generator(self, tape):
        """The generator's Adam step from its tape's gradients (averaged over the ranks first when data parallel) -> the flat gradient applied."""
        g_flat = self.g_params.gather(tape.flat if tape.flat is not None else tape.grads)
        if self.allreduce_flat is not None:
            g_flat = self.allreduce_flat(g_flat)
        elif self.allreduce is not None:                   # dict route (host): the 2-rank gloo tests
            g_flat = self.ctx.to_device(self.g_params.flatten(self.allreduce(self.g_params.split(g_flat.cpu().numpy()))))
        self.g_opt.lr = staircase_lr(self.g_lr0, self.step)
        self.g_opt.apply(self.g_params.flat, g_flat)
        self.g_params.stale = True
        self.step += 1
        return g_flat

    def pixel_step(self, lr_images, hr_images):
        """One generator update on the pixel loss alone (mean |hr - G(lr)|, ESRGAN_model.py:433-445; the generator half of _train_step,
        :506-531, without the adversarial / perceptual / spectral terms): sr355.recipes' fit.  -> the L1 value before the update."""
        ctx = self.ctx
        self._check_patch(lr_images)
        lr_t, hr_t = _device_batch(ctx, lr_images), _device_batch(ctx, hr_images)
        with self._prepacked(False):
            tg = self.generator_tape()
            y = generator_forward(tg, Var(lr_t, need=False), self.scale, self.nb, self.att)
            pix = float(ctx.l1(hr_t, y.v).item())
            y.g = ctx.eltwise(L.ELT_SIGN_DIFF, y.v, hr_t, 1.0 / y.v.numel(), 0.0)
            tg.backward()
        self._update_generator(tg)
        return pix

    def train_step(self, lr_images, hr_images):
        """-> {'g_loss', 'd_loss', parts...}; weights, u, optimiser states advance in place (ESRGAN_model.py:475-533).  With a device
        discriminator the step issues two uploads (the image batches) and one read (the six loss scalars)."""
        if self.disc is None or self.vw is None:
            raise RuntimeError("ESRGANTrainer was built without discriminator / VGG19 weights: only pixel_step is available")
        self._check_patch(lr_images)
        if self._vgg_src is not self.vw:                  # the first step, or ESRGAN.set_loss_network_weights has replaced the VGG19 weights
            self._vgg, self._vgg_src = ParamBucket(self.ctx, self.vw), self.vw
            for key in [k for k in self._packs if k is True or (isinstance(k, tuple) and k[0] == "bf16")]:
                del self._packs[key]
            self._perc16 = PerceptualBf16(self.ctx, self._vgg) if self.perceptual_dtype == "bf16" else None
        ctx, disc = self.ctx, self.disc
        hr_shape = hr_images.shape if hasattr(hr_images, "shape") else np.shape(hr_images)
        with self._prepacked(True, tuple(int(v) for v in hr_shape[:3])):                     # the generator's weights change only in the step's last lines, VGG19's never
            lr_t, hr_t = _device_batch(ctx, lr_images), _device_batch(ctx, hr_images)
            # The reference runs the generator twice per step, once under each tape (ESRGAN_model.py:490, :508); its weights do not change
            # in between (the discriminator is updated first), so both runs are the same tensor: one taped forward serves both.
            tg = self.generator_tape()
            masks = {"g": {}, "d_real": {}, "d_fake": {}} if self.collect_masks else {}
            self.last_masks = masks or None
            tg.masks = masks.get("g")
            y = generator_forward(tg, Var(lr_t, need=False), self.scale, self.nb, self.att)
            fake = y.v
            # ---- discriminator update (tg.dev: a host discriminator's tapes add this step's uploads of its arrays, one per array)
            l_real = disc.critic(Var(hr_t, need=False), 1.0, masks=masks.get("d_real"), devcache=tg.dev)      # renormalisation 1
            l_fake = disc.critic(Var(fake, need=False), 0.0, masks=masks.get("d_fake"), devcache=tg.dev)      # renormalisation 2
            disc.update(staircase_lr(self.d_lr0, self.step), self.allreduce, self.allreduce_flat)
            # ---- generator update
            yv = Var(fake)
            adv = disc.critic(yv, 1.0, wgrad=False, devcache=tg.dev)                                           # renormalisation 3
            perc, pix, spec, dy = self._content_terms(hr_t, fake, yv.g)
            # The one place where the step's loss scalars become floats, and the step's last read.  It waits for what has been launched so far, so it
            # stands before the generator's backward is queued (where the host mode always read perc / pix / spec), not after it: behind that backward,
            # most of the step's launches, the same read measured 0.5-0.7 ms a step slower in host mode, 0.3 ms in device mode (profiles/one_train_step_aba.txt).
            l_real, l_fake, adv, perc, pix, spec = _floats([l_real, l_fake, adv, perc, pix, spec])
            y.g = self.last_dy = dy
            tg.backward()
            self._last = {"g_flat": self._update_generator(tg), "g_names": set(tg.grads)}
            self.last_fake = fake
        return {"g_loss": adv + 1.0 * perc + 100.0 * pix + 1.0 * spec, "d_loss": l_real + l_fake, "adversarial": adv, "perceptual": perc,
                "pixel": pix, "spectral": spec}

    def _content_terms(self, hr_t, fake, d_adv):
        """The generator loss beside its adversarial term: VGG19 perceptual (x 1), pixel L1 (x 100) and spectral (x 1) of `fake` against hr_t
        -> (perc, pix, spec as one-element device tensors, d g_loss / d fake: their gradients and d_adv, the adversarial term's)."""
        ctx = self.ctx
        if self.perceptual_dtype == "bf16":
            perc, d_perc = self._perc16(hr_t, fake)
        else:
            tv = Tape(ctx, self._vgg.arrays, wgrad=False, devcache=self._vgg.devcache)
            fr = vgg19_features(tv, Var(hr_t, need=False))
            tv.ops = []
            yv = Var(fake)
            ff = vgg19_features(tv, yv)
            perc = ctx.mse(fr.v, ff.v)
            ff.g = ctx.eltwise(L.ELT_AXPBY, ff.v, fr.v, 2.0 / ff.v.numel(), -2.0 / ff.v.numel())
            tv.backward()
            d_perc = yv.g
        pix = ctx.l1(hr_t, fake)
        spec = ctx.spectral_l1(fake, hr_t)
        dy = ctx.eltwise(L.ELT_SIGN_DIFF, fake, hr_t, 100.0 / fake.numel(), 0.0)
        dy = ctx.eltwise(L.ELT_AXPBY, dy, ctx.spectral_l1_bwd(fake, hr_t, 1.0), 1.0, 1.0)
        dy = ctx.eltwise(L.ELT_AXPBY, dy, d_adv, 1.0, 1.0)
        dy = ctx.eltwise(L.ELT_AXPBY, dy, d_perc, 1.0, 1.0)
        return perc, pix, spec, dy
