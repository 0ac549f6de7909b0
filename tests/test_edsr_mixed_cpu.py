"""EDSR's bf16 mixed-precision training option without a GPU: the constructor's rules, and the restated reference of the step (tests/edsr_mixed_ref.py)
against plain fp64 autograd -- its own gradient error is what the GPU tests' end-to-end bounds are multiples of."""
import numpy as np
import pytest
import torch

import edsr_mixed_ref as R


def test_constructor_rules():
    from SRModels.deep_learning_models.EDSR_model import EDSR
    assert EDSR().train_dtype == "f32" and EDSR(update="device").train_dtype == "f32"
    assert EDSR(update="device", train_dtype="bf16").train_dtype == "bf16"
    assert EDSR(compute_dtype="bf16", update="device", train_dtype="bf16").compute_dtype == "bf16"      # independent of the inference dtype
    for kw in (dict(train_dtype="bf16"), dict(train_dtype="bf16", update="host")):
        with pytest.raises(ValueError, match="train_dtype.*update"):
            EDSR(**kw)
    for bad in ("fp16", "bfloat16", None, "F32"):
        with pytest.raises(ValueError, match="train_dtype"):
            EDSR(update="device", train_dtype=bad)


def test_the_bf16_step_refuses_a_host_weight_dict():
    """The step keeps fp32 master weights in the fit's ParamBucket: a host weight dict (update="host") is refused before anything touches a device."""
    from sr355 import train as T
    with pytest.raises(ValueError, match="ParamBucket"):
        T.edsr_loss_and_grads_bf16(None, {"conv2d": (np.zeros((3, 3, 3, 4), np.float32), np.zeros(4, np.float32))}, None, None)


@pytest.mark.parametrize("which", ["he_normal", "inside"])
def test_restated_reference_against_fp64_autograd(which):
    """2 blocks, 64 filters, x2, batch 2 of 12 x 12.  The restated bf16 step's gradient against fp64 autograd: rel-L2 per layer (d_ref) and 1 - cos over
    the flat gradient, printed; the GPU tests bound the device by twice the latter.  bf16 keeps 8 significant bits (2^-9 = 0.2 % per rounding): a
    gradient further than 30 % per layer or 2e-2 in 1 - cos from fp64 is a wrong restatement, not rounding; with the clip idle ('inside') no mask
    of the last layer can flip and the figure must be well below that: 5 % and 1e-3."""
    scale, nb, rs = 2, 2, 0.1
    w = R.weight_sets(scale, nb)[which]
    x, t = R.batch(scale)
    T, loss, g = R.mixed_step_ref(w, x, t, scale, nb, rs)
    loss64, g64 = R.autograd_ref(w, x, t, scale, nb, rs)
    order = list(w)
    d_ref = {n: (R.rel_l2(g[n][0], g64[n][0]), R.rel_l2(g[n][1], g64[n][1])) for n in order}
    omc = R.one_minus_cos(R.flat(g, order), R.flat(g64, order))
    for n in order:
        print(f"{which}: {n}: d_ref kernel {d_ref[n][0]:.3e} bias {d_ref[n][1]:.3e}")
    print(f"{which}: 1 - cos = {omc:.3e}; loss {float(loss):.6f} vs fp64 {float(loss64):.6f}")
    lim_layer, lim_cos = (0.05, 1e-3) if which == "inside" else (0.30, 2e-2)
    assert max(max(v) for v in d_ref.values()) <= lim_layer and 0 <= omc <= lim_cos
    assert abs(float(loss) - float(loss64)) <= 2.0 ** -6 * float(loss64)
    # every taped tensor is a bf16 value, and the permutations / selects are exact functions of their inputs
    for name, v in T.items():
        assert torch.equal(R.rb(v), v), name
    assert torch.equal(T["dv_1"], R.s2d(T["d_out"], 2))
    if which == "inside":
        assert bool(((T["pre"] > 0) & (T["pre"] < 1)).all())


def test_teacher_forcing_the_reference_on_itself_is_exact():
    """teacher_forced fed the restated reference's own tape reproduces it: every conv output rounds to the taped value, the exact tensors match
    bitwise, the gradients are the same numbers -- the two walks of the graph agree on which tensor, weight, scale and skip goes where."""
    scale, nb, rs = 4, 2, 0.1
    w = R.weight_sets(scale, nb)["he_normal"]
    x, t = R.batch(scale)
    T, _, g = R.mixed_step_ref(w, x, t, scale, nb, rs)
    convs, exact, g2 = R.teacher_forced(T, w, t, scale, nb, rs)
    names = {n for n, _, _ in convs} | {n for n, _ in exact} | {"x"}
    assert names == set(T)
    for name, v, bound in convs:
        assert torch.equal(R.rb(v), T[name]), name
        assert bool((bound >= 0).all())
    for name, ref in exact:
        assert torch.equal(ref, T[name]), name
    for n in g:
        assert torch.equal(g[n][0], g2[n][0]) and torch.equal(g[n][1], g2[n][1]), n
