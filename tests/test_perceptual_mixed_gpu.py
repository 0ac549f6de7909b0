"""ESRGAN's VGG19 perceptual term in bf16 mixed precision on the device (ESRGANTrainer(perceptual_dtype="bf16"), sr355.gan_train.PerceptualBf16)
against the contract restated in fp64 (tests/vgg_mixed_ref.py): every stored stage teacher-forced per element, the loss and its gradient end to end against
plain fp64 autograd, train_step beside the fp32 trainer.  Real VGG19 widths, seeded he-normal weights, a batch of 2 + 2."""
import numpy as np
import pytest
import torch

import vgg_mixed_ref as R
from sr355 import gan_train as GT
from sr355.train import ParamBucket

pytestmark = pytest.mark.gpu

SCALE, NB, G = 2, 2, 8                                        # the trainers' generator: x2, two RRDBs, the notebook's growth width


@pytest.fixture(scope="module")
def vgg():
    return R.vgg_weights()


@pytest.fixture(scope="module")
def branch(ctx, vgg):
    """One device pass per HR size, run once and shared: (hr, fake, perc, d perc / d fake fp64, tape as fp64)."""
    cache = {}

    def get(n):
        if n not in cache:
            hr, fake = R.images(2, n, 11)
            pb = GT.PerceptualBf16(ctx, ParamBucket(ctx, vgg))
            pb.tape = []
            perc, d = pb(ctx.to_device(hr), ctx.to_device(fake))
            assert perc.dtype == torch.float32 and d.dtype == torch.float32 and tuple(d.shape) == fake.shape
            assert all(t.dtype == torch.bfloat16 for _, t in pb.tape)
            tape = {k: R.t64(t) for k, t in pb.tape}
            assert len(tape) == len(pb.tape)
            cache[n] = (hr, fake, float(perc.item()), R.t64(d), tape)
        return cache[n]
    return get


def test_teacher_forced_stages_at_48(branch, vgg):
    """Every stored tensor of the branch recomputed in fp64 from the device's own stored input of that stage: conv outputs (both kernels, the fused masks
    included) within 2^-8 |v| + (9 Cin + 2) 2^-24 S and off the once-rounded reference in at most 1e-2 of their non-zero elements by one step; the pools, their
    gradients, the separate ReLU selects and the loss gradient bitwise."""
    hr, fake, _, d, tape = branch(48)
    convs, exact = R.teacher_forced(tape, vgg, 2, 48, 48)
    assert {c[0] for c in convs} | {e[0] for e in exact} | {"pre"} == set(tape)
    assert len(convs) == 16 + 16 and len(exact) == 4 + 1 + 4 + 5                     # 16 forward and 16 input-gradient convs; pools, the loss, pool gradients, five selects
    small = sum(r[5] == "small" for r in GT.perceptual_routes(48, 48, 2)), sum(r[7] == "small" for r in GT.perceptual_routes(48, 48, 2))
    assert small == (8, 8)                                                           # blocks 4 and 5 run on the small-image kernel, both ways
    v = R.preprocess64(torch.cat([R.t64(fake), R.t64(hr)]))
    assert float(((tape["pre"][..., :3] + tape["pre"][..., 3:] - v).abs() - 2.0 ** -16 * v.abs()).max()) <= 2.0 ** -15
    for label, got, v, bound in convs:
        R.check_conv(label, got, v, bound)
    for label, got, want in exact:
        assert torch.equal(got, want), label
    assert torch.equal(d, (torch.tensor(np.float32(127.5)) * tape["d_pre"].flip(-1).float()).double())
    off = np.mean([float((tape[f"block{b}_conv1"] <= 0).double().mean()) for b in (2, 3, 4, 5)])
    print(f"{off:.3f} of the ReLUs of block 2-5's first convs are off")
    assert 0.3 < off < 0.7


# |device - restated| / restated of perc, measured on an MI355X.  The first-order bound above is what reasoning gives and is loose (1e-1); this is
# the regression bar beside it, three times the measured figure, as for train_step below.
PERC_DEVICE_VS_RESTATED = {48: 7.402e-04, 24: 1.227e-02}


@pytest.mark.parametrize("n", [48, 24])
def test_end_to_end_against_fp64_autograd(branch, vgg, n):
    """The device and the restated reference are two realisations of one contract.  perc: |device - restated| / restated within the first-order effect of the
    restated reference's own feature error (vgg_mixed_ref.perc_bound), and within three times what was measured.  d perc / d fake: 1 - cos(device, fp64 autograd) <= 2 (1 - cos(restated, fp64 autograd)).
    Measured on an MI355X: 48 x 48 perc 7.402e-04 (bound 1.036e-01), 1 - cos 3.464e-02 against the restated
    reference's 3.424e-02; 24 x 24 (block 5 on 1 x 1 images) perc 1.227e-02 (bound 1.051e-01), 1 - cos 2.830e-02 against 2.849e-02."""
    hr, fake, perc, d, _ = branch(n)
    p_ref, d_ref, T = R.branch_ref(vgg, hr, fake)
    p64, d64, _, _ = R.branch_autograd(vgg, hr, fake)
    bound = R.perc_bound(vgg, hr, fake, T)
    rel = abs(perc - float(p_ref)) / float(p_ref)
    dev, ref = R.one_minus_cos(d.flatten(), d64.flatten()), R.one_minus_cos(d_ref.flatten(), d64.flatten())
    print(f"{n} x {n}: perc device {perc!r} restated {float(p_ref)!r} fp64 {float(p64)!r}: |device - restated| / restated {rel:.3e} (bound {bound:.3e}), "
          f"|restated - fp64| / fp64 {abs(float(p_ref) - float(p64)) / float(p64):.3e}; 1 - cos device {dev:.3e} restated {ref:.3e} (ratio {dev / ref:.2f})")
    assert rel <= bound
    assert rel <= 3.0 * PERC_DEVICE_VS_RESTATED[n]
    assert dev <= 2.0 * ref


# ---------------------------------------------------------------------------------------------------------------- train_step beside fp32
# |bf16 - fp32| / fp32 of the first train_step's `perceptual` and `g_loss`, measured on an MI355X over the data seeds 11 .. 15; the assertions
# are three times the largest of each.  g_loss is led by 100 x the pixel L1, which the option does not touch.
PERCEPTUAL_REL_DIFF = [1.874e-03, 1.036e-04, 2.022e-04, 2.849e-03, 1.493e-03]
G_LOSS_REL_DIFF = [1.155e-08, 5.790e-10, 1.319e-09, 1.895e-08, 1.002e-08]


@pytest.fixture(scope="module")
def gan_weights(vgg):
    from oracle import models as M
    from sr355.weights import init_weights
    gw = init_weights(M.esrgan_g_layers(SCALE, G, NB), scheme="he_normal", seed=4000)
    gw["final_conv2"] = ((gw["final_conv2"][0] * np.float32(0.05)).astype(np.float32), gw["final_conv2"][1])      # an unsaturated tanh (tests/esrgan_mixed_ref.py)
    for n in gw:
        if n.endswith("_f") or n.endswith("_g"):
            gw[n] = ((gw[n][0] * np.float32(0.25)).astype(np.float32), (gw[n][1] * np.float32(0.25)).astype(np.float32))
    return gw, init_weights(M.discriminator_layers(), seed=5000), vgg


def batch(seed):
    from sr355.synth import make_pairs
    lr, hr = make_pairs(2, 12, 12, SCALE, seed)
    return (lr * 2.0 - 1.0).astype(np.float32), (hr * 2.0 - 1.0).astype(np.float32)


def trainer(ctx, gan_weights, **kw):
    gw, dw, vw = gan_weights
    kw.setdefault("discriminator", "device")
    kw.setdefault("attention_impl", "streamed")
    return GT.ESRGANTrainer(ctx, gw, dw, vw, SCALE, NB, attention=True, u_seed=3, **kw)


def rel_diffs(ctx, gan_weights, seed):
    lr, hr = batch(seed)
    out = trainer(ctx, gan_weights, perceptual_dtype="bf16").train_step(lr, hr)
    ref = trainer(ctx, gan_weights).train_step(lr, hr)
    return out, ref, {k: abs(out[k] - ref[k]) / abs(ref[k]) for k in ("perceptual", "g_loss")}


def test_train_step_beside_the_fp32_trainer(ctx, gan_weights):
    """Two trainers from one start: nothing in front of d_loss, adversarial, pixel and spectral changed, so they are equal to the bit; perceptual and g_loss move
    by what bf16 costs the branch."""
    out, ref, rel = rel_diffs(ctx, gan_weights, 11)
    print(f"first step perceptual bf16 {out['perceptual']!r} fp32 {ref['perceptual']!r} ({rel['perceptual']:.3e}); g_loss bf16 {out['g_loss']!r} "
          f"fp32 {ref['g_loss']!r} ({rel['g_loss']:.3e})")
    assert all(np.isfinite(v) for v in out.values())
    for k in ("d_loss", "adversarial", "pixel", "spectral"):
        assert out[k] == ref[k], k
    assert out["perceptual"] != ref["perceptual"]
    assert rel["perceptual"] <= 3.0 * max(PERCEPTUAL_REL_DIFF) and rel["g_loss"] <= 3.0 * max(G_LOSS_REL_DIFF)


def test_the_default_is_unchanged(ctx, gan_weights):
    """perceptual_dtype="f32" is the argument omitted: two steps give the same losses and the same generator weights to the bit, and no kernel of the bf16 branch
    runs in them."""
    lr, hr = batch(11)
    runs = []
    for kw in ({}, {"perceptual_dtype": "f32"}):
        tr = trainer(ctx, gan_weights, **kw)
        ctx.conv_routes(True)
        losses = [tr.train_step(lr, hr) for _ in range(2)]
        routes = ctx.conv_routes(False)
        assert routes and not any("bf16" in r for r in routes), sorted(set(routes))
        assert tr._perc16 is None
        runs.append((losses, tr.g_params.flat.cpu().numpy().view(np.int32)))
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    tr = trainer(ctx, gan_weights, perceptual_dtype="bf16")
    ctx.conv_routes(True)
    tr.train_step(lr, hr)
    routes = ctx.conv_routes(False)
    assert sum("bf16" in r for r in routes) == 4 + 4, sorted(set(routes))            # HR 24: the convs of blocks 1 and 2 and their input gradients; the rest is the small-image kernel
    frozen = {k.data_ptr() for k, _ in tr._vgg.dev.values()}
    assert tr._packs[True][1] > 0 and not any(w.data_ptr() in frozen for w, _ in tr._packs[True][2])      # no VGG19 layer stands in the step's fp32 pack list


@pytest.mark.parametrize("kw", [{"discriminator": "host"}, {"discriminator": "device", "train_dtype": "bf16", "dense_block_impl": "lds"},
                                {"discriminator": "host", "train_dtype": "bf16", "dense_block_impl": "lds", "attention_impl": "materialised"}],
                         ids=["host", "device-lds", "host-lds-materialised"])
def test_the_option_composes(ctx, gan_weights, kw):
    """Beside the same trainer with the fp32 branch: the four terms in front of the branch are equal to the bit, perceptual within the measured bar."""
    lr, hr = batch(12)
    out = trainer(ctx, gan_weights, perceptual_dtype="bf16", **dict(kw)).train_step(lr, hr)
    ref = trainer(ctx, gan_weights, **dict(kw)).train_step(lr, hr)
    assert all(np.isfinite(v) for v in out.values())
    for k in ("d_loss", "adversarial", "pixel", "spectral"):
        assert out[k] == ref[k], k
    assert abs(out["perceptual"] - ref["perceptual"]) / ref["perceptual"] <= 3.0 * max(PERCEPTUAL_REL_DIFF)


def test_new_vgg19_weights_drop_the_packs(ctx, gan_weights):
    """ESRGAN.set_loss_network_weights on a live trainer: the step after it runs on the new weights -- its perceptual term is a fresh trainer's from the same
    generator, to the bit, and not what the packs made for the old weights give."""
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    gw, dw, vw = gan_weights
    vw2 = R.vgg_weights(seed=6001)
    m = ESRGAN(perceptual_dtype="bf16", discriminator_update="device", train_attention="streamed")
    m.setup_model(scale_factor=SCALE, growth_channels=G, num_rrdb_blocks=NB)
    m.set_weights(gw)
    m.set_loss_network_weights(discriminator=dw, vgg19=vw)
    tr = m._ensure_trainer()
    assert tr.perceptual_dtype == "bf16"
    lr, hr = batch(13)
    m._train_step(lr, hr)
    handles = tr._perc16
    assert handles is not None and len(handles._handles) == 2 * 12                    # HR 24: blocks 3-5 on the small-image kernel, forward and input gradient, packed once
    now = {n: (k.copy(), b.copy()) for n, (k, b) in tr.gw.items()}
    m.set_loss_network_weights(vgg19=vw2)
    second = m._train_step(lr, hr)
    assert tr._perc16 is not handles
    fresh = {w: trainer(ctx, (now, dw, v), perceptual_dtype="bf16").train_step(lr, hr)["perceptual"] for w, v in (("new", vw2), ("old", vw))}
    assert second["perceptual"] == fresh["new"] and second["perceptual"] != fresh["old"]
