"""The benchmarked network (BASELINE configs[2]: ESRGAN x4, NB=23, G=32, both SelfAttention layers) at FULL depth against the CPU
oracle, stage by stage (reference graph: ESRGAN_model.py:212-345).

fp32 device path  vs  the oracle in fp64                      : rel-L2 <= 5e-5 at every stage and at the output.
bf16 device path  vs  the oracle in its bf16-storage mode     : the oracle rounds to bf16 exactly where the device stores bf16
    (oracle.models.esrgan_g_forward(bf16_storage=True)), so what is left is accumulation order.  Through 345 conv layers and a
    trunk gain of 1.2**23 that residue is not zero: two VALID evaluations of the same bf16-storage graph -- the oracle with fp32
    and with fp64 arithmetic inside a layer -- already differ by ~0.8 % rel-L2 at the end of the trunk (a value that lands on the
    other side of a bf16 rounding boundary is a 2**-8 perturbation that the following layers carry along).  That self-noise is
    measured here, per stage, and the device has to stay within a small multiple of it; absolute floors (PSNR >= 45 dB on the
    image, 2 % rel-L2 per stage) are asserted as well.  A wrong skip, a wrong channel offset in one of the three rotating
    row-blocked concat buffers or a dropped layer shows up as O(1) at the stage where it happens.

Weights: seeded glorot-uniform (sr355.weights.init_weights), attention logits conditioned (sr355.weights.condition_attention:
its docstring says why -- with raw glorot weights the logits span +-1700 and the oracle disagrees with ITSELF at 11 dB)."""
import numpy as np
import pytest
import torch

from oracle import models as M
from oracle import ops as O
from sr355 import Model
from sr355.synth import make_pairs
from sr355.weights import bf16_rounded, condition_attention, init_weights, round_to_bf16

pytestmark = pytest.mark.gpu

SCALE, NB, G = 4, 23, 32
# oracle stage name -> device op whose output it is (csrc/api.hip build_esrgan)
STAGES = ([("initial_conv", "initial_conv")] + [(f"rrdb_{b}", f"rrdb_{b}_dense3_conv5") for b in range(NB)] +
          [("trunk_add", "trunk_conv"), ("self_attention_trunk", "self_attention_trunk_v"), ("upsample_0", "upsample_0_conv"),
           ("self_attention_upsample_0", "self_attention_upsample_0_v"), ("upsample_1", "upsample_1_conv"),
           ("final_conv1", "final_conv1")])


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def psnr01(a, b):
    return float(O.psnr((np.asarray(a, np.float64) + 1) / 2, (np.asarray(b, np.float64) + 1) / 2, dtype=np.float64).min())


def lr_patches(n, seed):
    """n LR patches 48x48 cut from a synthetic 3D-print tile (the bench's input distribution), in [-1, 1]."""
    lr, _ = make_pairs(1, 48, 48 * n, SCALE, seed=seed)
    return np.stack([lr[0, :, 48 * i:48 * (i + 1)] for i in range(n)]) * 2.0 - 1.0


def device_trace(ctx, dtype, w, x, nb=NB, stages=STAGES):
    m = Model("esrgan_g", compute_dtype=dtype, scale_factor=SCALE, num_blocks=nb, growth_channels=G, use_attention=True, ctx=ctx)
    m.set_weights(w)
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    y, taps = m.forward_with_taps(ctx.to_device(x, td), [dev for _, dev in stages])
    y2 = m.forward(ctx.to_device(x, td))          # no taps, same buffers
    if dtype == "f32":
        assert torch.equal(y, y2)                 # the same kernels: the same image
    else:
        # a tap on final_conv1 makes final_conv1 / final_conv2 run as two kernels: the activation is stored as ONE bf16 value; the untapped
        # forward folds the RGB conv into final_conv1's epilogue, where the never-stored activation enters as a bf16 hi + lo pair (round 4),
        # so the two bf16 images differ by that one rounding of a 64-channel tensor: output roundings flipped by an ulp (2^-8 at most on [-1, 1]) ...
        d = (y.float() - y2.float()).abs()
        assert float(d.max()) <= 2.0 ** -6 and float(d.mean()) <= 2.0 ** -9, (float(d.max()), float(d.mean()), float((d > 0).float().mean()))
        ctx.set_fused(ctx.FUSED_ALL & ~ctx.FUSED_RGB_TAIL, 0)                 # ... and are the same image when that pair runs as two kernels in both
        try:
            assert torch.equal(y, m.forward(ctx.to_device(x, td)))
        finally:
            ctx.set_fused(ctx.FUSED_ALL, 0)
    return y.float().cpu().numpy(), {name: taps[dev].cpu().numpy() for name, dev in stages}


def test_full_depth_fp32_vs_fp64_oracle(ctx):
    w = condition_attention(init_weights(M.esrgan_g_layers(SCALE, G, NB), seed=3000))
    x = lr_patches(4, seed=44).astype(np.float32)
    got, taps = device_trace(ctx, "f32", w, x)
    parts = {}
    ref = M.esrgan_g_forward(x, w, SCALE, NB, dtype=np.float64, parts=parts)
    worst = 0.0
    for name, _ in STAGES:
        e = rel_l2(taps[name], parts[name])
        worst = max(worst, e)
        assert e <= 5e-5, (name, e)
    e = rel_l2(got, ref)
    print(f"\nfp32 full depth: output rel-L2 {e:.2e}, worst stage {worst:.2e}, PSNR(gpu, oracle) {psnr01(got, ref):.1f} dB")
    assert got.shape == ref.shape == (4, 192, 192, 3)
    assert e <= 5e-5, e


def test_full_depth_bf16_vs_bf16_storage_oracle(ctx):
    w = bf16_rounded(condition_attention(init_weights(M.esrgan_g_layers(SCALE, G, NB), seed=3000)))
    x = round_to_bf16(lr_patches(2, seed=45).astype(np.float32))
    got, taps = device_trace(ctx, "bf16", w, x)
    p64, p32 = {}, {}
    ref = M.esrgan_g_forward(x, w, SCALE, NB, dtype=np.float64, bf16_storage=True, parts=p64, fused_tail=False)
    alt = M.esrgan_g_forward(x, w, SCALE, NB, dtype=np.float32, bf16_storage=True, parts=p32, fused_tail=False)
    plain = M.esrgan_g_forward(x, w, SCALE, NB, dtype=np.float64)
    print("\nstage                       dev-vs-oracle   oracle self-noise (fp32 vs fp64 arithmetic)")
    for name, _ in STAGES:
        dev, noise = rel_l2(taps[name], p64[name]), rel_l2(p32[name], p64[name])
        print(f"{name:28s}{dev:10.2e}      {noise:10.2e}")
        assert dev <= 3.0 * noise + 1e-3, (name, dev, noise)
        assert dev <= 2e-2, (name, dev)
    dev, noise = rel_l2(got, ref), rel_l2(alt, ref)
    p_dev, p_noise, p_plain = psnr01(got, ref), psnr01(alt, ref), psnr01(got, plain)
    print(f"output                      {dev:10.2e}      {noise:10.2e}")
    print(f"PSNR(gpu bf16, bf16-storage oracle) {p_dev:.2f} dB; oracle self-noise {p_noise:.2f} dB; PSNR(gpu bf16, fp64 reference graph) {p_plain:.2f} dB")
    assert dev <= 3.0 * noise + 1e-3, (dev, noise)
    assert p_dev >= 45.0, p_dev
    assert p_plain >= 40.0, p_plain


def test_bf16_nb4_one_full_rotation_of_the_concat_buffers(ctx):
    """G=32 keeps the three dense-block buffers row-blocked and rotates them once per RRDB (X,Y,Z -> Y,Z,X): NB=4 is one full
    turn plus one.  Every RRDB output against the bf16-storage oracle; ragged 40x28 patches (tiles of 16x16 / 12x16 do not fit)."""
    nb = 4
    stages = [(f"rrdb_{b}", f"rrdb_{b}_dense3_conv5") for b in range(nb)] + [("trunk_add", "trunk_conv"), ("final_conv1", "final_conv1")]
    w = bf16_rounded(condition_attention(init_weights(M.esrgan_g_layers(SCALE, G, nb), seed=3300)))
    x = round_to_bf16(np.random.default_rng(9).uniform(-1, 1, (3, 40, 28, 3)).astype(np.float32))
    got, taps = device_trace(ctx, "bf16", w, x, nb=nb, stages=stages)
    p64 = {}
    ref = M.esrgan_g_forward(x, w, SCALE, nb, dtype=np.float64, bf16_storage=True, parts=p64, fused_tail=False)
    for name, _ in stages:
        e = rel_l2(taps[name], p64[name])
        assert e <= 5e-3, (name, e)
    assert got.shape == ref.shape == (3, 160, 112, 3)
    assert rel_l2(got, ref) <= 5e-3 and psnr01(got, ref) >= 50.0, (rel_l2(got, ref), psnr01(got, ref))
