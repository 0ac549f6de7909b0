"""The streamed training attention without a GPU: the fp64 backward formulas of tests/attention_train_ref.py against torch autograd, the two
C-ABI exports, and the validation of the attention_impl / train_attention keywords."""
import os
import re

import numpy as np
import pytest
import torch

import attention_train_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fp64_backward_formulas_are_autograds():
    q, k, v, do = (torch.tensor(a.astype(np.float64)) for a in TR.gauss_case(33, 2, 33, 1.0))
    ref = TR.forward_backward_fp64(q.numpy(), k.numpy(), v.numpy(), do.numpy())
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    s = q @ k.transpose(1, 2)
    o = torch.softmax(s, dim=-1) @ v
    o.backward(do)
    assert np.abs(ref["o"] - o.detach().numpy()).max() <= 1e-13
    assert np.abs(ref["lse"] - torch.logsumexp(s, dim=-1).detach().numpy()).max() <= 1e-13
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        assert TR.rel_l2(ref[name], t.grad.numpy()) <= 1e-13, name
    # the statistic is what the backward recomputes the softmax from: rows of exp(s - lse) sum to one
    assert np.abs(np.exp(s.detach().numpy() - ref["lse"][..., None]).sum(-1) - 1).max() <= 1e-13


def test_rel_l2_of_a_zero_reference_accepts_only_zeros():
    z = np.zeros((2, 3))
    assert TR.rel_l2(z, z) == 0.0 and TR.rel_l2(z + 1e-30, z) == float("inf") and TR.rel_l2(np.full((2, 3), np.nan), z + 1) == float("inf")


def _declared_args(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sr355.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
    assert m, f"{name} is not declared in include/sr355.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_exports_are_declared_with_the_bindings_argument_counts():
    from sr355 import _lib
    for name, n in (("sr_attention_fwd_lse", 12), ("sr_attention_bwd", 16)):
        args = _declared_args(name)
        assert name in _lib.SIGNATURES and len(args) == len(_lib.SIGNATURES[name][1]) == n, (name, args)
        assert args[0] == "sr_ctx* ctx" and args[-1] == "void* stream"
        assert hasattr(_lib.load(), name)


def test_unknown_attention_implementations_are_refused_before_any_device_work():
    from sr355 import gan_train as GT
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    assert GT.ATTENTION_IMPLS == ("materialised", "streamed")
    for bad in ("flash", "Streamed", None):
        with pytest.raises(ValueError):
            GT.Tape(None, {}, attention_impl=bad)
        with pytest.raises(ValueError):
            GT.ESRGANTrainer(None, {}, None, None, 2, 1, attention_impl=bad)
        with pytest.raises(ValueError):
            ESRGAN(train_attention=bad)
    assert ESRGAN().train_attention == "materialised" and ESRGAN(train_attention="streamed").train_attention == "streamed"
