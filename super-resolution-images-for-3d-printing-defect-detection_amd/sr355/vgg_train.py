"""Fine-tuning of the VGG16 base's last layers with the classifier head (FineTunedVGG16.setup_model(fine_tune_base=True)).

The reference (defect_detection_models/VGG16_model.py:75-82) freezes the whole nested VGG16 and then flips `trainable` on its last
`train_last_n_layers` sub-layers, which a frozen parent makes a no-op: it never trains a base layer, and neither does the default path of this
port.  This module is the training the flags ask for, with Keras' semantics for it: the convs among the last n of the base's 19 layers and the
two Dense layers are the variables of ONE Adam (lr `learning_rate`, epsilon 1e-7, no clipping), the loss is mean sparse categorical
cross-entropy + l2_reg * sum(dense kernel^2), Dropout sits in front of both Dense layers.

Per batch (VGGFineTuner.step):
  * the frozen prefix runs in the inference model, in its compute dtype (FineTunedVGG16._prefix_device: one tapped forward; the block5 / head
    part of that forward is computed and thrown away, as _gap_device throws away the head);
  * the trained tail runs in fp32 on a gan_train.Tape over the views of one flat train.ParamBucket (conv + ReLU, max-pool);
  * block5_pool + GAP are two launches forward; sr_dense_head_step_dx gives the head's gradients and the gradient at the GAP features,
    sr_pool_gap_bwd takes that through GAP, the pool and the last conv's ReLU in one launch, the tape takes it down through the convs
    (input gradients: the forward kernels on rotated weights; kernel gradients: sr_conv2d_wgrad, or sr_conv2d_wgrad_maps on maps of at most
    8 x 8, which packs three 8 x 8 images into one staged tile), and DeviceAdam applies the flat gradient;
  * nothing is read back: the step's loss / hits / sum k1^2 land in the fit's per-epoch stats tensor (train.fit_head_device).
"""
import torch

from . import _lib as L
from .gan_train import Tape, Var
from .train import DeviceAdam, ParamBucket

# keras.applications.VGG16(include_top=False).layers, in graph order
VGG16_BASE_LAYERS = ("input_1", "block1_conv1", "block1_conv2", "block1_pool", "block2_conv1", "block2_conv2", "block2_pool",
                     "block3_conv1", "block3_conv2", "block3_conv3", "block3_pool", "block4_conv1", "block4_conv2", "block4_conv3", "block4_pool",
                     "block5_conv1", "block5_conv2", "block5_conv3", "block5_pool")


def vgg16_tail_layers(n):
    """The last n of the base's 19 Keras layers, in graph order (n <= 0: none; n >= 19: all of them)."""
    n = max(0, min(int(n), len(VGG16_BASE_LAYERS)))
    return list(VGG16_BASE_LAYERS[len(VGG16_BASE_LAYERS) - n:])


def vgg16_tail_convs(n):
    """The layers of vgg16_tail_layers(n) that have parameters: the convs fine_tune_base trains (4: block5_conv1..3; 5 adds only block4_pool;
    6 adds block4_conv3; 1 is block5_pool alone: none)."""
    return [name for name in vgg16_tail_layers(n) if "_conv" in name]


def vgg16_prefix_tap(first_conv):
    """Where the trained tail's input comes from -> (op of the inference model to tap or None for the image itself, whether a 2x2 max-pool
    follows the tap)."""
    i = VGG16_BASE_LAYERS.index(first_conv)
    prev = VGG16_BASE_LAYERS[i - 1]
    if prev == "input_1":
        return None, False
    if prev.endswith("_pool"):
        return VGG16_BASE_LAYERS[i - 2], True
    return prev, False


class VGGFineTuner:
    """The trainable convs (graph order) and the head in one flat device bucket, its DeviceAdam and the training step.  `bucket`, `opt` and
    `head` (the head's slice of bucket.flat, sr_dense_head_step's parameter layout) are what train.fit_head_device drives."""

    def __init__(self, ctx, weights, convs, learning_rate=1e-3):
        if not convs:
            raise ValueError("VGGFineTuner: no trainable conv (head-only training is train.fit_head_device's default)")
        self.ctx, self.convs = ctx, list(convs)
        self.layers = [n for n in VGG16_BASE_LAYERS[VGG16_BASE_LAYERS.index(self.convs[0]):]]      # the tail in graph order, pools included
        self.bucket = ParamBucket(ctx, {n: weights[n] for n in self.convs + ["dense", "predictions"]})
        self.opt = DeviceAdam(ctx, self.bucket.flat, learning_rate, epsilon=1e-7)
        self.grads = torch.zeros_like(self.bucket.flat)
        self.gviews = self.bucket.split(self.grads)
        self.head_offset = sum(k.numel() + b.numel() for k, b in (self.bucket.dev[n] for n in self.convs))
        self.head, self.head_grads = self.bucket.flat[self.head_offset:], self.grads[self.head_offset:]
        self.collect_masks = False                         # tests: keep the step's ReLU output of every trained conv in last_acts
        self.last_acts = None

    def tail_features(self, x):
        """Prefix activations fp32 [n,h,w,C] -> GAP features fp32 [n,512] through the tail with the bucket's current weights (validation)."""
        ctx = self.ctx
        for name in self.layers:
            if name.endswith("_pool"):
                x = ctx.spatial_op(L.SP_MAXPOOL2, x)
            else:
                k, b = self.bucket.dev[name]
                x = ctx.conv2d_dev(x, k, b, k.shape[3], act="relu")
        return ctx.spatial_op(L.SP_GAP, x)

    def _wgrad(self, x, dz, k, out=None):
        """3x3 kernel and bias gradient: the packed-tile kernel on maps of at most 8 x 8 (block5 on 128-pixel patches), sr_conv2d_wgrad above."""
        if k == 3 and x.shape[1] <= 8 and x.shape[2] <= 8:
            return self.ctx.conv2d_wgrad_maps(x, dz, out=out)
        return self.ctx.conv2d_wgrad(x, dz, k, out=out)

    def step(self, x, labels, stats, work, keep0=None, keep1=None, keep_scale=1.0, l2_reg=0.0):
        """One update from prefix activations x fp32 [n,h,w,C] and labels int32 [n]; stats fp64 [3] as sr_dense_head_step fills it."""
        ctx, bucket = self.ctx, self.bucket
        t = Tape(ctx, bucket.arrays, devcache=dict(bucket.devcache))
        t.conv_wgrad = self._wgrad
        acts = {} if self.collect_masks else None
        v = Var(x, need=False)
        for name in self.layers[:-2]:                      # up to the last conv and block5_pool, which go by hand below
            v = t.maxpool(v) if name.endswith("_pool") else t.conv(v, name, act="relu")
            if acts is not None and not name.endswith("_pool"):
                acts[name] = v.v
        last = self.convs[-1]
        k, b = bucket.dev[last]
        a = ctx.conv2d_dev(v.v, k, b, k.shape[3], act="relu")
        if acts is not None:
            acts[last] = a
        self.last_acts = acts
        feats = ctx.spatial_op(L.SP_GAP, ctx.spatial_op(L.SP_MAXPOOL2, a))
        dfeats = torch.empty_like(feats)
        nc = bucket.shapes["predictions"][0][1]
        ctx.dense_head_step(feats, labels, self.head, nc, stats, work, self.head_grads, keep0, keep1, keep_scale, l2_reg, dfeats=dfeats)
        dz = ctx.pool_gap_bwd(a, dfeats)                   # GAP, block5_pool and the last conv's ReLU, backward
        self._wgrad(v.v, dz, 3, out=self.gviews[last])
        if v.need:
            v.g = ctx.conv2d_dev(dz, k, None, k.shape[2], rot=True)
        t.backward()
        for name, (dw, db) in t.grads.items():
            self.gviews[name][0].copy_(dw)
            self.gviews[name][1].copy_(db)
        self.opt.apply(bucket.flat, self.grads)
        bucket.stale = True
