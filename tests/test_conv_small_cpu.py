"""The host side of the bf16 perceptual branch, without a GPU: the option's validation, the exports, which VGG19 layer goes to which kernel, and
what bf16 itself costs -- the restated contract (tests/vgg_mixed_ref.py) beside plain fp64 autograd of VGG19."""
import numpy as np
import pytest
import torch

import vgg_mixed_ref as R
from sr355 import _lib as L
from sr355 import gan_train as GT

EXPORTS = ["sr_conv3x3_small_pack_bytes", "sr_conv3x3_small_pack_bf16", "sr_conv3x3_small_bf16", "sr_vgg_preprocess_bf16", "sr_vgg_preprocess_bwd", "sr_maxpool2_bf16",
           "sr_maxpool2_bwd_bf16", "sr_mse_grad_bf16"]


def test_the_option_is_validated_before_anything_is_uploaded():
    assert GT.check_perceptual_dtype("f32") == "f32" and GT.check_perceptual_dtype("bf16") == "bf16"
    for bad in ("fp16", "BF16", None, 16):
        with pytest.raises(ValueError, match=r"perceptual_dtype must be one of \('f32', 'bf16'\)"):
            GT.check_perceptual_dtype(bad)
    with pytest.raises(ValueError, match="perceptual_dtype must be one of"):
        GT.ESRGANTrainer(None, {}, None, None, 2, 1, perceptual_dtype="half")      # raised before the context or a weight is touched
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    with pytest.raises(ValueError, match="perceptual_dtype must be one of"):
        ESRGAN(perceptual_dtype="fp8")
    assert ESRGAN().perceptual_dtype == "f32" and ESRGAN(perceptual_dtype="bf16").perceptual_dtype == "bf16"


def test_the_binding_and_the_header_hold_the_new_exports():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sr355.h")).read()
    for name in EXPORTS:
        assert name in L.SIGNATURES and f" {name}(" in header, name
        assert "ESRGAN_model.py:" in header[:header.index(f" {name}(")].rsplit("/*", 1)[1], name      # the comment block in front cites the reference


@pytest.mark.parametrize("hr, B, fwd, bwd", [(48, 16, "5", "45"), (96, 16, "", "5"), (24, 16, "45", "345"), (48, 2, "45", "45"), (24, 2, "345", "345"),
                                             (48, None, "45", "45"), (96, None, "5", "5"), (48, 64, "5", "5"), (24, 64, "45", "45")])
def test_dispatch_rule(hr, B, fwd, bwd):
    """The small-image kernel takes a call where it measured fastest: images of at most 3 x 3 pixels, or of at most 6 x 6 with at most 1008 pixels in the call
    (2 B images forward, B backward), Cin a multiple of 32.  fwd / bwd: the blocks whose forward convs / input gradients it runs.  At the notebook's batch of 16 HR 48 patches that is
    block 5 forward and blocks 4-5 backward; at cfg3's 96 x 96, block 5 backward only."""
    routes = GT.perceptual_routes(hr, hr, B)
    assert [r[0] for r in routes] == [f"block{b}_conv{k}" for b, n, _ in GT.VGG19_CFG for k in range(1, n + 1)]
    for name, h, w, cin, cout, route, pooled, route_bwd in routes:
        blk = name[5]
        assert (h, w) == (hr >> (int(blk) - 1),) * 2
        assert route == ("small" if blk in fwd else "conv2d") and route_bwd == ("small" if blk in bwd else "conv2d"), name
        assert pooled == (name in ("block1_conv2", "block2_conv2", "block3_conv4", "block4_conv4"))
        for images, r, ci in ((1 if B is None else 2 * B, route, cin), (1 if B is None else B, route_bwd, cout)):
            assert (r == "small") == (ci % 32 == 0 and (h * w <= 9 or (h * w <= 36 and images * h * w <= 1008))), name
    assert routes[0][3] == 3 and routes[0][5] == routes[0][7] == "conv2d"
    assert GT.small_conv_wins(6, 6, 512, 512, 28) and not GT.small_conv_wins(6, 6, 512, 512, 29) and not GT.small_conv_wins(7, 6, 512, 512, 1)
    assert not GT.small_conv_wins(3, 3, 48, 64, 1) and GT.small_conv_wins(1, 1, 64, 32, 576) and GT.small_conv_wins(3, 3, 512, 512, 256)
    assert GT.small_conv_wins(4, 4, 512, 512, 63) and not GT.small_conv_wins(4, 4, 512, 512, 64)
    with pytest.raises(ValueError, match="leave no pixel"):
        GT.perceptual_routes(8, 8)


def test_pool_reference_ties_and_odd_sizes():
    x = torch.tensor([[1.0, 1.0, 5.0], [0.0, 1.0, 2.0], [7.0, 8.0, 9.0]]).double().reshape(1, 3, 3, 1)
    assert R.pool64(x).reshape(-1).tolist() == [1.0]
    dx = R.pool_bwd64(x, torch.full((1, 1, 1, 1), 3.0).double())
    assert dx.reshape(3, 3).tolist() == [[3.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]      # two equal maxima: the first wins; the dropped row and column get 0
    assert float(R.pool_bwd64(torch.zeros(1, 2, 2, 1).double(), torch.ones(1, 1, 1, 1).double()).abs().sum()) == 0.0      # an all-zero window: its winner is not positive


def test_what_bf16_itself_costs_at_24x24():
    """The restated contract against plain fp64 autograd on 2 + 2 images of 24 x 24 (block 5 runs on 1 x 1 images).  Recorded, and held to loose sanity bars only:
    the figures say what any bf16 realisation of this branch costs with he-normal weights, where half of every layer's ReLUs are off and a rounding may flip a
    select -- relative loss error 9.4e-4, 1 - cos of d perc / d fake 2.8e-2 (seed 11)."""
    w = R.vgg_weights()
    hr, fake = R.images(2, 24, 11)
    perc, d, T = R.branch_ref(w, hr, fake)
    p64, d64, _, _ = R.branch_autograd(w, hr, fake)
    rel, omc = abs(float(perc) - float(p64)) / float(p64), R.one_minus_cos(d.flatten(), d64.flatten())
    print(f"24 x 24: perc restated {float(perc)!r} fp64 {float(p64)!r} (rel {rel:.3e}); 1 - cos of d perc / d fake {omc:.3e}; first-order bound {R.perc_bound(w, hr, fake, T):.3e}")
    assert rel <= R.perc_bound(w, hr, fake, T)
    assert 0.0 < omc < 0.1 and abs(float(d.norm() / d64.norm()) - 1.0) < 0.05
    assert all(torch.equal(t, R.rb(t)) for t in T.values())                       # every stored tensor holds bf16 values
    assert T["pre"].shape == (4, 24, 24, 6) and T["block5_conv4"].shape == (4, 1, 1, 512) and T["d_pre"].shape == (2, 24, 24, 3)
    v = R.preprocess64(torch.cat([R.t64(fake), R.t64(hr)]))
    assert float(((T["pre"][..., :3] + T["pre"][..., 3:] - v).abs() - 2.0 ** -16 * v.abs()).max()) <= 0.0
