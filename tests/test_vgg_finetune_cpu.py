"""fine_tune_base without a device: the layer selection, and the reference of tests/test_vgg_finetune_gpu.py held against itself -- its
conv gradient against a direct tap sum, and its fp32 evaluation against its fp64 one at the GPU tests' seeds, which is what bounds how much
of the GPU tests' tolerances the reference itself may use."""
import numpy as np
import pytest
import torch

import vgg_finetune_ref as R


def test_tail_layers_follow_the_keras_layer_list():
    from sr355.vgg_train import VGG16_BASE_LAYERS, vgg16_prefix_tap, vgg16_tail_convs, vgg16_tail_layers
    assert VGG16_BASE_LAYERS == R.BASE and len(VGG16_BASE_LAYERS) == 19
    b5 = ["block5_conv1", "block5_conv2", "block5_conv3"]
    all13 = [n for n in R.BASE if "_conv" in n]
    assert len(all13) == 13
    assert vgg16_tail_layers(0) == [] and vgg16_tail_convs(0) == []
    assert vgg16_tail_layers(1) == ["block5_pool"] and vgg16_tail_convs(1) == []
    assert vgg16_tail_layers(4) == b5 + ["block5_pool"] and vgg16_tail_convs(4) == b5
    assert vgg16_tail_layers(5) == ["block4_pool"] + b5 + ["block5_pool"] and vgg16_tail_convs(5) == b5       # 5 adds only a pool
    assert vgg16_tail_convs(6) == ["block4_conv3"] + b5
    assert vgg16_tail_convs(18) == all13 and vgg16_tail_layers(18) == list(R.BASE[1:])
    assert vgg16_tail_convs(19) == all13 and vgg16_tail_layers(19) == list(R.BASE) and vgg16_tail_layers(25) == list(R.BASE)
    assert vgg16_prefix_tap("block5_conv1") == ("block4_conv3", True) and vgg16_prefix_tap("block4_conv3") == ("block4_conv2", False)
    assert vgg16_prefix_tap("block1_conv1") == (None, False)


def test_trainable_parameter_counts():
    from sr355.vgg_train import vgg16_tail_convs
    size = {n: int(np.prod(s)) + s[-1] for n, s in R.vgg16_layer_shapes(2)}
    head = size["dense"] + size["predictions"]
    assert head == 131842 and sum(size.values()) == 14846530
    assert sum(size[n] for n in vgg16_tail_convs(4)) + head == 7211266 == 3 * 2359808 + 131842
    assert sum(size[n] for n in vgg16_tail_convs(6)) + head == 9571074


def test_reference_conv_gradient_is_the_tap_sum():
    rng = np.random.default_rng(0)
    x, k, b, dz = rng.normal(size=(1, 3, 3, 4)), rng.normal(size=(3, 3, 4, 4)), rng.normal(size=4), rng.normal(size=(1, 3, 3, 4))
    kt = torch.tensor(k, requires_grad=True)
    z = R._conv(torch.tensor(x).permute(0, 3, 1, 2), kt, torch.tensor(b))
    (z * torch.tensor(dz).permute(0, 3, 1, 2)).sum().backward()
    assert R.rel_l2(kt.grad.numpy(), R.tail_conv_grad_numpy(x, dz)) <= 1e-14
    # and the forward: output pixel (1,1) sees the whole input under the whole kernel
    assert abs(float(z.detach()[0, 2, 1, 1]) - (np.sum(x[0] * k[:, :, :, 2]) + b[2])) <= 1e-12


@pytest.fixture(scope="module")
def weights():
    return R.seeded_weights()


@pytest.mark.parametrize("case", R.STEP_CASES)
def test_reference_fp32_takes_the_branches_of_fp64(weights, case):
    n_last, hw = case
    first = R.FIRST_CONV[n_last]
    X, y, k0, k1 = R.step_inputs(n_last, hw)
    x = R.forward_frozen(X, weights, R.BASE[:R.BASE.index(first)], torch.float32)
    kw = dict(keep0=k0, keep1=k1, keep_scale=1.25, l2_reg=1e-3)
    r64 = R.tail_head(x, R.tail_of(first), weights, y, dtype=torch.float64, **kw)
    r32 = R.tail_head(x, R.tail_of(first), weights, y, dtype=torch.float32, **kw)
    relu = sum(int(np.sum(r64["relu"][n] != r32["relu"][n])) for n in r64["relu"])
    sel = sum(int(np.sum((r64["sel"][n][0] != r32["sel"][n][0]) & r64["sel"][n][1])) for n in r64["sel"])
    worst = max(R.rel_l2(r32["grads"][n][s], r64["grads"][n][s]) for n in r64["grads"] for s in (0, 1))
    print(case, "relu branches", relu, "of", sum(m.size for m in r64["relu"].values()), "pool selections", sel, "gradient rel-L2", worst,
          "loss", abs(r32["loss"] - r64["loss"]) / r64["loss"])
    assert relu == 0 and sel == 0
    assert worst < 1e-6, worst


def test_reference_fit_fp32_against_fp64(weights):
    X, y, Xv, yv = R.fit_inputs()
    h64, _ = R.fit(X, y, Xv, yv, weights, dtype=torch.float64, **R.FIT)
    h32, _ = R.fit(X, y, Xv, yv, weights, dtype=torch.float32, **R.FIT)
    d32 = max(abs(a - b) / max(abs(b), 1e-30) for k in h64 for a, b in zip(h32[k], h64[k]))
    print("d32", d32, h64)
    assert d32 <= 2.5e-4, d32
