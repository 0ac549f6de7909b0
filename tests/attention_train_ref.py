"""fp64 reference of the training SelfAttention core (csrc/attention_train.hip): forward with the per-query softmax statistic, and the
backward pass, both MATERIALISED in NumPy (the [B,N,N] matrices the device path never forms).

    s = q k^T            lse_i = log sum_j exp(s_ij)          P = exp(s - lse)            o = P v
    dv = P^T dO          dP = dO v^T                          D_i = sum_j P_ij dP_ij = <dO_i, o_i>
    dS = P (dP - D)      dq = dS k                            dk = dS^T q

(ESRGAN_model.py:57-65 with q = g, k = f, v = h; no 1/sqrt(d) scale.)  tests/test_attention_train_cpu.py checks these formulas against
torch autograd in fp64.

Bounds of tests/test_attention_train_gpu.py
-------------------------------------------
o: per element, attention_ref.bound(..., "f32", ...) -- the forward kernel is the inference kernel's arithmetic.
lse: |lse - ref| <= 1e-5 max(1, |ref|);  dq, dk, dv: rel-L2 <= 2e-5 -- the project's figure for the materialised fp32 attention gradient
(test_attention_forward_backward_materialised).  rel_l2 is ||got - ref|| / ||ref||; a reference that is exactly zero (N = 1: P = 1, dS = 0)
is met only by exact zeros.
"""
import numpy as np

LSE_TOL = 1e-5
GRAD_TOL = 2e-5


def forward_backward_fp64(q, k, v, do):
    """q, k [B,N,8], v, do [B,N,32] -> dict of fp64 o, lse, dq, dk, dv."""
    q, k, v, do = (np.asarray(a, np.float64) for a in (q, k, v, do))
    s = np.matmul(q, k.transpose(0, 2, 1))
    m = s.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(axis=-1, keepdims=True))
    p = np.exp(s - lse)
    o = np.matmul(p, v)
    dv = np.matmul(p.transpose(0, 2, 1), do)
    dp = np.matmul(do, v.transpose(0, 2, 1))
    d = (p * dp).sum(axis=-1, keepdims=True)
    ds = p * (dp - d)
    return dict(o=o, lse=lse[..., 0], dq=np.matmul(ds, k), dk=np.matmul(ds.transpose(0, 2, 1), q), dv=dv)


def rel_l2(got, ref):
    """||got - ref|| / ||ref||; 0 / 0 = 0, x / 0 = inf."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, nrm = float(np.linalg.norm(got - ref)), float(np.linalg.norm(ref))
    if not np.isfinite(err):
        return float("inf")
    if nrm == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / nrm


def lse_ratio(got, ref):
    """max |lse - ref| / (LSE_TOL max(1, |ref|)): accepted when <= 1."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    r = np.abs(got - ref) / (LSE_TOL * np.maximum(1.0, np.abs(ref)))
    return float(np.where(np.isfinite(r), r, np.inf).max())


def gauss_case(seed, B, N, sd):
    """Gaussian q, k of standard deviation sd (scores q . k have standard deviation sd^2 sqrt(8): sd = 1 spans about +-8, sd = sqrt(10)
    about +-80, where nearly every P_ij underflows and one key carries each row), Gaussian v and a dense Gaussian dO; fp32."""
    rng = np.random.default_rng(seed)
    f = lambda c, s: (s * rng.standard_normal((B, N, c))).astype(np.float32)
    return f(8, sd), f(8, sd), f(32, 1.0), f(32, 1.0)
