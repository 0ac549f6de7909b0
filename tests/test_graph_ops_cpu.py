"""tests/graph_ref.py is the reference graph, and its designed weights keep the per-op GPU tests (tests/test_graph_ops_gpu.py) from hiding a failure.
No GPU.

  * The free-running chain -- every row fed with the previous rows' own fp64 outputs -- equals oracle.models.*_forward(dtype=float64) to 1e-12
    relative (largest difference over the largest reference magnitude), for every model kind, configuration, shape and data type's table of
    graph_ref.cases(), and at every stage esrgan_g_forward's parts= exposes.
  * On that chain alone: every op with a skip has median |alpha conv| >= median |sum beta_i skip_i| (a wrong tap of the conv then moves the sum by
    more than the bf16 contract allows), every ReLU / LeakyReLU op has at least 25 % of its outputs positive, and every clipped / tanh output has at
    least 50 % of its elements strictly inside (0, 1) / with |y| < 0.9 (a saturated output hides everything in front of it)."""
import numpy as np
import pytest

import graph_ref as G

CASES = [(kind, cfg, dt, shape) for kind, cfg, dts, shapes in G.cases() for dt in dts for shape in shapes]


def case_id(k, cfg, dt, s):
    return f"{k}{'-' + 'x'.join(str(int(c)) for c in cfg) if cfg else ''}-{dt}-{'x'.join(map(str, s))}"


IDS = [case_id(*c) for c in CASES]


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and float(np.abs(a - b).max()) <= 1e-12 * max(float(np.abs(b).max()), 1e-300)


@pytest.mark.parametrize("kind,cfg,dtype,shape", CASES, ids=IDS)
def test_free_running_chain_is_the_reference_graph(kind, cfg, dtype, shape):
    t, outs = G.chain_of(kind, cfg, shape, dtype)
    x, w = G.model_input(kind, shape), G.weights(kind, cfg)
    parts = {} if kind == "esrgan_g" else None
    ref = G.oracle_forward(kind, cfg, x, w, parts)
    assert t[-1]["out"] and close(outs[-1], ref), (outs[-1].shape, ref.shape)
    hw = G.out_hw(t, shape[1], shape[2])
    for r, o, (h, wd) in zip(t, outs, hw):
        if o.ndim == 4:
            assert o.shape == (shape[0], h, wd, r["C"]), (r["name"], o.shape)
    if parts is None:
        return
    ks = G.KSCALE if dtype == "bf16" else 1.0
    seen = set()
    for r, o in zip(t, outs):
        st = r.get("stage")
        if st is None:
            continue
        seen.add(st)
        if st.endswith("/fgh"):
            p = parts[st[:-4] + "/parts"]
            B, H, W, _ = o.shape
            assert close(o[..., 0:8].reshape(B, H * W, 8) / ks, p["f"]) and close(o[..., 8:16].reshape(B, H * W, 8), p["g"]), st
            assert close(o[..., 16:48].reshape(B, H * W, 32), p["h"]), st
        elif st.endswith("/o"):
            assert close(o, parts[st[:-2] + "/parts"]["o"]), st
        else:
            assert close(o, parts[st]), st
    want = {k for k in parts if not k.endswith("/parts")} | {k[:-6] + s for k in parts if k.endswith("/parts") for s in ("/fgh", "/o")}
    assert seen == want, (seen ^ want)


COND = [(kind, cfg, ("bf16" if "bf16" in dts else "f32"), shape) for kind, cfg, dts, shapes in G.cases() for shape in shapes]
COND_IDS = [case_id(*c) for c in COND]


@pytest.mark.parametrize("kind,cfg,dtype,shape", COND, ids=COND_IDS)
def test_conditions_that_keep_the_gpu_tests_from_hiding_a_failure(kind, cfg, dtype, shape):
    t, outs = G.chain_of(kind, cfg, shape, dtype)
    x, w = G.model_input(kind, shape), G.weights(kind, cfg)
    ks = G.KSCALE if dtype == "bf16" else 1.0
    get = lambda i: x if i < 0 else outs[i]
    for r, o in zip(t, outs):
        if r["kind"] != "conv":
            continue
        if r["skips"] and dtype == "bf16":
            c, s = G.conv_terms(r, [get(i) for i in r["src"]], [get(i) for i, _ in r["skips"]], w, ks)
            assert np.median(c) >= np.median(s), (r["name"], float(np.median(c)), float(np.median(s)))
        if r["act"] in ("relu", "lrelu"):
            assert float(np.mean(o > 0)) >= 0.25, (r["name"], float(np.mean(o > 0)))
        if r["clip"]:
            assert float(np.mean((o > 0) & (o < 1))) >= 0.5, (r["name"], float(np.mean((o > 0) & (o < 1))))
        if r["act"] == "tanh":
            assert float(np.mean(np.abs(o) < 0.9)) >= 0.5, (r["name"], float(np.mean(np.abs(o) < 0.9)))


def test_recorded_gains_are_the_tables():
    """The gains in the rows are the ones the weights carry, and every bf16 configuration with a skip has one."""
    for kind, cfg, dts, _ in G.cases():
        t = G.table(kind, cfg, dts[-1])
        got = {r["name"]: r["gain"] for r in t if r["kind"] == "conv" and r["gain"]}
        assert got == G.GAINS.get((kind, cfg), {}), (kind, cfg)
        base, w = G.base_weights(kind, cfg), G.weights(kind, cfg)
        for r in t:
            if r["kind"] == "conv":
                for n, _ in r["parts"]:
                    assert np.array_equal(w[n][0], base[n][0] * np.float32(2.0 ** (r["gain"] if n == r["name"] else 0))), n


@pytest.mark.parametrize("n", [5, 8, 21, 22, 35, 36])
def test_pick_phase_is_keras_same_padding(n):
    """A stride-2 SAME 3x3 conv of an impulse train equals the picked stride-1 conv (oracle.ops.conv2d pads as TensorFlow does)."""
    from oracle import ops as O
    rng = np.random.default_rng(n)
    x = rng.standard_normal((1, n, n + 1, 2))
    k = rng.standard_normal((3, 3, 2, 3))
    full = O.conv2d(x, k, None, dtype=np.float64)
    assert np.array_equal(O.conv2d(x, k, None, stride=2, dtype=np.float64).shape, full[:, G.pick_phase(n)::2, G.pick_phase(n + 1)::2].shape)
    assert np.allclose(O.conv2d(x, k, None, stride=2, dtype=np.float64), full[:, G.pick_phase(n)::2, G.pick_phase(n + 1)::2], rtol=0, atol=1e-12)
