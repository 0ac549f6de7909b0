"""ESRGAN's bf16 mixed-precision trunk without a GPU: the argument check of the constructor, the ctypes mirror of sr_wgrad_job against the C compiler,
and the restated reference (tests/esrgan_mixed_ref.py) beside plain fp64 autograd."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import esrgan_mixed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_dtype_is_checked_in_the_constructor():
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    with pytest.raises(ValueError, match="train_dtype"):
        ESRGAN(train_dtype="fp16")
    assert ESRGAN(train_dtype="bf16").train_dtype == "bf16"
    assert ESRGAN().train_dtype == "f32"


def test_the_trainer_names_the_layer_it_refuses():
    """The growth-width check needs no device: it reads the weights' shapes before anything is uploaded."""
    from oracle import models as M
    from sr355 import gan_train as GT
    from sr355.weights import init_weights
    gw = init_weights(M.esrgan_g_layers(2, 8, 1), seed=3000)
    with pytest.raises(ValueError, match=r"rrdb_0_dense1_conv1 has 8 growth channels"):
        GT.ESRGANTrainer(None, gw, None, None, 2, 1, train_dtype="bf16")
    with pytest.raises(ValueError, match="train_dtype"):
        GT.ESRGANTrainer(None, gw, None, None, 2, 1, train_dtype="half")
    assert GT.trunk_layers(init_weights(M.esrgan_g_layers(2, 32, 2), seed=1), 2) == R.trunk_names(2)


def test_wgrad_job_layout_is_the_headers(tmp_path):
    """sr_wgrad_job crosses the ABI by pointer: the ctypes mirror must have the C compiler's size and field offsets."""
    from sr355 import _lib
    fields = ["x", "dy", "Cin", "Cout", "scale", "dw", "db"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sr355.h"\nint main(void) {\n  printf("%zu", sizeof(sr_wgrad_job));\n'
                   + "".join(f'  printf(" %zu", offsetof(sr_wgrad_job, {f}));\n' for f in fields)
                   + '  printf(" %d\\n", SR_WGRAD_GROUP_MAX);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    J = _lib.WgradJob
    assert out == [ctypes.sizeof(J)] + [getattr(J, f).offset for f in fields] + [8]
    assert [f for f, _ in J._fields_] == fields


def test_restated_reference_beside_fp64_autograd():
    """The restated contract against plain fp64 autograd of oracle.train.generator_forward_t on the test configuration (x2, two RRDBs, G = 32, batch 2 of
    12 x 12, pixel L1): a sanity bound on the reference itself, not a device measurement.  With the roundings taken out the two are one computation."""
    lr, hr = R.batch()
    names = R.trunk_names(R.NB)
    for which, w in R.weight_sets().items():
        loss64, g64 = R.pixel_grads(w, lr, hr, mode="plain")
        loss, g = R.pixel_grads(w, lr, hr, mode="mixed")
        assert set(g) == set(g64) == set(w)
        omc = R.one_minus_cos(R.flat(g, names), R.flat(g64, names))
        small = min(float(R.flat(g, names).abs()[R.flat(g, names) != 0].min()), 1.0)
        print(f"{which}: pixel loss restated {loss:.6f} fp64 {loss64:.6f}; 1 - cos over the flat trunk gradient {omc:.3e}; smallest non-zero |gradient| {small:.3e}")
        assert np.isfinite(omc) and omc < 1e-1


def test_restated_reference_without_roundings_is_autograd(monkeypatch):
    lr, hr = R.batch()
    w = R.weight_sets()["he_normal"]
    _, g64 = R.pixel_grads(w, lr, hr, mode="plain")
    monkeypatch.setattr(R, "rb", lambda t: t)
    _, g = R.pixel_grads(w, lr, hr, mode="mixed")
    assert R.rel_l2(R.flat(g, list(w)), R.flat(g64, list(w))) <= 1e-7      # (the gradient entering the trunk passes through fp32, as on the device)
