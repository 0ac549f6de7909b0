"""Helpers shared by the tests that read a model's tensors op by op through sr_model_set_tap."""
import torch

from sr355 import Model


def host(t):
    return t.float().cpu().numpy()


def forward_tapped(m, x, idx):
    """forward with a tap on every op of `idx` -> (y, {op index: fp32 NHWC tensor}).  The tap buffers start out as NaN: a tap that is never
    written, or written in part, cannot pass for the values an earlier call left in the same memory."""
    ctx, ops = m.ctx, m.ops()
    B, H, W, _ = x.shape
    taps = {}
    try:
        for i in idx:
            h, w = Model._op_hw(ops[i], H, W)
            t = torch.full((B, h, w, ops[i][1]), float("nan"), dtype=torch.float32, device=ctx.torch_device)
            ctx.check(ctx.lib.sr_model_set_tap(m.h, i, t.data_ptr(), t.numel()))
            taps[i] = t
        y = m.forward(x)
        torch.cuda.synchronize()
    finally:
        for i in idx:
            ctx.lib.sr_model_set_tap(m.h, i, None, 0)
    return y, taps
