"""ESRGANTrainer(discriminator="device"): the discriminator's spectral normalisation, dense head, gradient bucket and Adam on the device
(csrc/disc_train.hip, sr355/gan_train.py) against the fp64 oracle (oracle/ops.py, oracle/train.py) -- the two ops alone, one step, a second
step on carried state, host mode against device mode, the all-reduce hooks, determinism and the ESRGAN wrapper.

Bounds are those of tests/test_train_gpu.py::test_esrgan_train_step for the same quantities: losses 2e-4 max(1, |v|), gradients rel-L2 2e-4,
kernels and u after renormalisation rel-L2 1e-5.  p of the head alone is an fp64 value rounded once to fp32 (2^-24 = 6e-8 relative): 1e-6."""

import numpy as np
import pytest
import torch

from oracle import models as M
from oracle import ops as O
from oracle import train as OT
from sr355 import _lib as L
from sr355 import gan_train as GT
from sr355 import train as T
from sr355.weights import init_weights

pytestmark = pytest.mark.gpu

HEAD = 256 * 256 + 256 + 256 + 1


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _gan_setup(scale, nb, G):
    """The recipe of tests/test_train_gpu.py."""
    gw = init_weights(M.esrgan_g_layers(scale, G, nb), seed=3000)
    gw = {n: ((k * 0.25, b * 0.25) if (n.endswith("_f") or n.endswith("_g")) else (k, b)) for n, (k, b) in gw.items()}     # moderate attention logits
    dw = init_weights(M.discriminator_layers(), seed=5000)
    vw = init_weights(M.vgg19_extractor_layers(), scheme="he_normal", seed=6000)
    vw = {n: (k * 0.05 if n == "block1_conv1" else k, b) for n, (k, b) in vw.items()}          # inputs are +-128 after caffe preprocessing: keep the features O(1)
    return gw, dw, vw


def _batch(scale, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (2, 12, 12, 3)).astype(np.float32), rng.uniform(-1, 1, (2, 12 * scale, 12 * scale, 3)).astype(np.float32)


def _copy(w):
    return {n: tuple(np.array(a, copy=True) for a in pair) for n, pair in w.items()}


# ------------------------------------------------------------------------------------------------ 1. spectral normalisation alone
SN_SHAPES = [("l0", (3, 3, 3, 64)), ("l1", (3, 3, 5, 7)), ("l2", (3, 3, 64, 128)), ("l3", (256, 256)), ("l4", (256, 1))]
SN_NAMES = [n for n, _ in SN_SHAPES]


def _sn_state(ctx):
    w = init_weights(SN_SHAPES[:2] + [("free", (3, 3, 4, 4))] + SN_SHAPES[2:], seed=77)          # "free": a layer no descriptor names
    rng = np.random.default_rng(3)                        # u as the trainer draws it: TruncatedNormal(stddev 0.02), [1, Cout]
    u = {n: np.clip(rng.normal(0, 0.02, (1, w[n][0].shape[-1])), -0.04, 0.04).astype(np.float32) for n in SN_NAMES}
    bucket = T.ParamBucket(ctx, w)
    table, u_len = ctx.spectral_norm_table(bucket, SN_NAMES)
    uflat = ctx.to_device(np.concatenate([u[n].ravel() for n in SN_NAMES]))
    assert u_len == uflat.numel() == 64 + 7 + 128 + 256 + 1
    return w, u, bucket, table, uflat


def test_spectral_norm_bucket_against_the_oracle(ctx):
    w, u, bucket, table, uflat = _sn_state(ctx)
    k64 = {n: w[n][0].astype(np.float64) for n in SN_NAMES}
    u_ref = dict(u)
    worst_k = worst_u = 0.0
    for it in range(3):
        ctx.spectral_norm_bucket(bucket.flat, uflat, table)
        got = bucket.split(bucket.flat.cpu().numpy())
        gu, o = uflat.cpu().numpy(), 0
        for n in SN_NAMES:
            k64[n], u_ref[n] = O.spectral_normalize(k64[n], u_ref[n])
            ek, eu = rel_l2(got[n][0], k64[n]), rel_l2(gu[o:o + u_ref[n].size], u_ref[n].ravel())
            worst_k, worst_u = max(worst_k, ek), max(worst_u, eu)
            assert ek <= 1e-5 and eu <= 1e-5, (it, n, ek, eu)
            assert np.array_equal(got[n][1], w[n][1]), (it, n, "bias")
            o += u_ref[n].size
        assert np.array_equal(got["free"][0], w["free"][0]) and np.array_equal(got["free"][1], w["free"][1]), it
    print(f"\nspectral_norm_bucket vs oracle, worst rel-L2 over 3 applications: kernel {worst_k:.1e}, u {worst_u:.1e}")
    # two fresh runs: the same bits
    _, _, bucket2, table2, uflat2 = _sn_state(ctx)
    for _ in range(3):
        ctx.spectral_norm_bucket(bucket2.flat, uflat2, table2)
    assert torch.equal(bucket2.flat, bucket.flat) and torch.equal(uflat2, uflat)


def test_spectral_norm_bucket_refuses_bad_descriptors(ctx):
    _, _, bucket, table, uflat = _sn_state(ctx)
    before, ubefore = bucket.flat.clone(), uflat.clone()
    n = bucket.flat.numel()
    bad = (L.SnDesc * 2)()
    bad[0].koff, bad[0].K, bad[0].Cout, bad[0].uoff = table[0].koff, table[0].K, table[0].Cout, table[0].uoff
    bad[1].koff, bad[1].K, bad[1].Cout, bad[1].uoff = n - 10, 4, 3, 0                  # 12 floats from 10 before the end
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, bad)
    bad[1].koff, bad[1].K, bad[1].Cout, bad[1].uoff = 0, 4, 3, uflat.numel() - 2        # u reaches past its tensor
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, bad)
    bad[1].koff, bad[1].K, bad[1].Cout, bad[1].uoff = 0, 0, 3, 0                        # K < 1
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, bad)
    bad[1].koff, bad[1].K, bad[1].Cout, bad[1].uoff = table[0].koff + 5, 4, 3, table[0].Cout                 # two kernels share floats: their workgroups would race
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, bad)
    bad[1].koff, bad[1].K, bad[1].Cout, bad[1].uoff = table[1].koff, 4, 3, table[0].Cout - 1                 # two u ranges share a float
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, bad)
    with pytest.raises(ValueError):
        ctx.spectral_norm_bucket(bucket.flat, uflat, (L.SnDesc * 0)())
    lib = ctx.lib
    assert lib.sr_spectral_norm_bucket(ctx.h, bucket.flat.data_ptr(), n, uflat.data_ptr(), uflat.numel(), table, 0, ctx.stream()) == L.SR_ERR_INVALID
    assert lib.sr_spectral_norm_bucket(ctx.h, None, n, uflat.data_ptr(), uflat.numel(), table, len(table), ctx.stream()) == L.SR_ERR_INVALID
    assert lib.sr_spectral_norm_bucket(ctx.h, bucket.flat.data_ptr(), n, uflat.data_ptr(), uflat.numel(), None, len(table), ctx.stream()) == L.SR_ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(bucket.flat, before) and torch.equal(uflat, ubefore)              # refused: nothing was launched


# ------------------------------------------------------------------------------------------------ 2. the head alone
def _head_params(seed=11):
    w = init_weights([("disc_dense1", (256, 256)), ("disc_output", (256, 1))], seed=seed)
    return np.concatenate([w["disc_dense1"][0].ravel(), w["disc_dense1"][1], w["disc_output"][0].ravel(), w["disc_output"][1]]).astype(np.float32)


def _head_ref(h, prm, target):
    """The tail of oracle.train.discriminator_forward_t (GAP, Dense 256 LeakyReLU 0.2, Dense 1 sigmoid) with oracle.train._bce, torch autograd fp64
    on an NHWC map.  -> (loss, p [B], z2 [B], dh, flat parameter gradient)."""
    F = torch.nn.functional
    p64 = prm.astype(np.float64)
    k1 = torch.tensor(p64[:65536].reshape(256, 256), requires_grad=True)
    b1 = torch.tensor(p64[65536:65792], requires_grad=True)
    k2 = torch.tensor(p64[65792:66048].reshape(256, 1), requires_grad=True)
    b2 = torch.tensor(p64[66048:], requires_grad=True)
    ht = torch.tensor(h.astype(np.float64), requires_grad=True)
    g = ht.mean(dim=(1, 2))
    a1 = F.leaky_relu(g @ k1 + b1, 0.2)
    z2 = a1 @ k2 + b2
    p = torch.sigmoid(z2)
    loss = OT._bce(torch.full_like(p, float(target)), p)
    loss.backward()
    grad = np.concatenate([k1.grad.numpy().ravel(), b1.grad.numpy(), k2.grad.numpy().ravel(), b2.grad.numpy()])
    return float(loss.item()), p.detach().numpy().ravel(), z2.detach().numpy().ravel(), ht.grad.numpy(), grad


def _head_run(ctx, h, prm, target, grads=None, accumulate=False):
    loss = ctx.empty((3,))
    loss.fill_(-7.0)
    p, dh = ctx.disc_head_step(ctx.to_device(h), prm, target, loss[1:2], grads, accumulate)
    l = loss.cpu().numpy()
    assert l[0] == -7.0 and l[2] == -7.0                  # the op writes its slot only
    return float(l[1]), p.cpu().numpy(), dh.cpu().numpy()


@pytest.mark.parametrize("case", [(2, 2, 2, 1.0), (3, 3, 1, 0.0)])
def test_disc_head_step_against_the_oracle(ctx, case):
    B, H, W, target = case
    rng = np.random.default_rng(100 + B)
    h = rng.standard_normal((B, H, W, 256)).astype(np.float32)
    prm = _head_params()
    pd = ctx.to_device(prm)
    grads = ctx.empty((HEAD,))
    grads.fill_(3.0)
    loss, p, dh = _head_run(ctx, h, pd, target, grads)
    rl, rp, _, rdh, rg = _head_ref(h, prm, target)
    g = grads.cpu().numpy()
    figs = {"loss": abs(loss - rl), "p": rel_l2(p, rp), "dh": rel_l2(dh, rdh), "dk1": rel_l2(g[:65536], rg[:65536]), "db1": rel_l2(g[65536:65792], rg[65536:65792]),
            "dk2": rel_l2(g[65792:66048], rg[65792:66048]), "db2": rel_l2(g[66048:], rg[66048:])}
    print("\ndisc_head_step vs oracle:", {k: f"{v:.1e}" for k, v in figs.items()})
    assert figs["loss"] <= 2e-4 * max(1.0, abs(rl)) and figs["p"] <= 1e-6
    assert all(figs[k] <= 2e-4 for k in ("dh", "dk1", "db1", "dk2", "db2")), figs
    # the accumulate flag: a second call (other map, other target) added onto the first equals the sum of the two single calls
    h2 = rng.standard_normal((B, H, W, 256)).astype(np.float32)
    g2 = ctx.empty((HEAD,))
    _head_run(ctx, h2, pd, 1.0 - target, g2)
    _, _, dh2 = _head_run(ctx, h2, pd, 1.0 - target, grads, accumulate=True)
    assert np.array_equal(grads.cpu().numpy(), g + g2.cpu().numpy())
    # wgrad off: the gradient bucket is not touched, dh is the same
    held = grads.clone()
    _, p3, dh3 = _head_run(ctx, h2, pd, 1.0 - target)
    assert torch.equal(grads, held) and np.array_equal(dh3, dh2)
    assert torch.equal(pd, ctx.to_device(prm))            # parameters are read only


def _saturated_case():
    """B = 4 on a 2 x 2 map: rows 0 and 1 are ten times larger than rows 2 and 3, the biases are zero, and disc_output's kernel is scaled so that the
    smaller of |z2[0]|, |z2[1]| is 22: rows 0, 1 lie outside the clip range (|z2| >= 20: p beyond 1e-7 of 0 or 1), rows 2, 3 inside (|z2| <= 8)."""
    rng = np.random.default_rng(5)
    h = rng.standard_normal((4, 2, 2, 256)).astype(np.float32)
    h[2:] *= 0.1
    prm = _head_params(seed=21)
    prm[65536:65792] = 0.0
    prm[66048:] = 0.0
    _, _, z2, _, _ = _head_ref(h, prm, 1.0)
    prm[65792:66048] *= np.float32(22.0 / min(abs(z2[0]), abs(z2[1])))
    return h, prm


def test_disc_head_step_outside_the_clip_range(ctx):
    h, prm = _saturated_case()
    pd = ctx.to_device(prm)
    for target in (1.0, 0.0):
        rl, rp, z2, rdh, rg = _head_ref(h, prm, target)
        assert np.all(np.abs(z2[:2]) >= 20.0) and np.all(np.abs(z2[2:]) <= 8.0), z2
        grads = ctx.empty((HEAD,))
        loss, p, dh = _head_run(ctx, h, pd, target, grads)
        g = grads.cpu().numpy()
        assert abs(loss - rl) <= 2e-4 * max(1.0, abs(rl)), (loss, rl)
        assert not dh[:2].any() and dh[2:].any()                                     # nothing flows back through a clipped probability
        assert rel_l2(dh, rdh) <= 2e-4 and rel_l2(g[:65536], rg[:65536]) <= 2e-4 and rel_l2(g[65792:66048], rg[65792:66048]) <= 2e-4
        assert rel_l2(g[65536:65792], rg[65536:65792]) <= 2e-4 and rel_l2(g[66048:], rg[66048:]) <= 2e-4          # db1, db2
        # ... and to every parameter gradient the saturated rows add exactly zero: alone they give exactly zero,
        g_sat = ctx.empty((HEAD,))
        g_sat.fill_(1.0)
        _, _, dh_sat = _head_run(ctx, h[:2], pd, target, g_sat)
        assert not g_sat.cpu().numpy().any() and not dh_sat.any()
        # and the batch's gradient is the other rows' own (their mean is over 2 rows instead of 4: a factor of exactly 2)
        g_in = ctx.empty((HEAD,))
        _head_run(ctx, h[2:], pd, target, g_in)
        assert rel_l2(2.0 * g.astype(np.float64), g_in.cpu().numpy()) <= 1e-6


def test_disc_head_step_refuses_other_widths(ctx):
    prm = ctx.to_device(_head_params())
    loss = ctx.empty((1,))
    with pytest.raises(ValueError):
        ctx.disc_head_step(ctx.empty((2, 2, 2, 128)), prm, 1.0, loss)
    with pytest.raises(ValueError):
        ctx.disc_head_step(ctx.empty((2, 2, 2, 256)), prm[:-1].contiguous(), 1.0, loss)
    with pytest.raises(ValueError):
        ctx.disc_head_step(ctx.empty((2, 2, 2, 256)), prm, 0.5, loss)
    h, p, dh = ctx.empty((2, 2, 2, 256)), ctx.empty((2,)), ctx.empty((2, 2, 2, 256))
    call = lambda i, hd, o: ctx.lib.sr_disc_head_step(ctx.h, h.data_ptr(), 2, 2, 2, i, hd, o, prm.data_ptr(), 1.0, loss.data_ptr(), p.data_ptr(), dh.data_ptr(),
                                                      None, 0, ctx.stream())
    for widths in ((128, 256, 1), (256, 128, 1), (256, 256, 2), (512, 256, 1)):
        assert call(*widths) == L.SR_ERR_INVALID, widths
    assert call(256, 256, 1) == L.SR_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 3. / 4. steps against the oracle
_RUNS = {}


def _device_run(ctx, cfg, second=False):
    """One device-mode step (and, with `second`, another on a second batch) of the existing test's configuration, every checked quantity
    copied to the host after each step, with the oracle's results: computed once per configuration and shared."""
    key = (cfg, second)
    if key in _RUNS:
        return _RUNS[key]
    scale, nb, G, att = cfg
    gw, dw, vw = _gan_setup(scale, nb, G)
    lr, hr = _batch(scale)
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=att, g_lr=1e-4, d_lr=1e-5, u_seed=3, discriminator="device")
    u0 = {n: v.copy() for n, v in tr.u.items()}
    snap = lambda out: dict(out=dict(out), d=_copy(tr.last_grads["d"]), dw=_copy(tr.dw), u={n: v.copy() for n, v in tr.u.items()}, t=tr.d_opt.t,
                            flat=tr.d_params.flat.cpu().numpy(), opt=type(tr.d_opt))
    out = tr.train_step(lr, hr)
    run = {"dw0": dw, "s1": snap(out), "ref1": OT.esrgan_train_step_ref(gw, dw, u0, vw, lr, hr, scale, nb, attention=att)}
    if second:
        gw1 = _copy(tr.gw)
        lr2, hr2 = _batch(scale, seed=8)
        out2 = tr.train_step(lr2, hr2)
        run["s2"] = snap(out2)
        r1 = run["ref1"]
        run["ref2"] = OT.esrgan_train_step_ref(gw1, r1["dw"], r1["u"], vw, lr2, hr2, scale, nb, attention=att, d_opt=r1["d_opt"],
                                               fake_override=tr.last_fake.cpu().numpy())
    _RUNS[key] = run
    return run


def _check_discriminator(s, ref, label):
    figs = {k: abs(s["out"][k] - ref["losses"][k]) for k in ("d_loss", "adversarial")}
    for k, v in figs.items():
        assert v <= 2e-4 * max(1.0, abs(ref["losses"][k])), (label, k, s["out"][k], ref["losses"][k])
    assert set(s["d"]) == set(ref["d_grads"]) == set(GT.DISC_LAYERS)
    ge = {n: (rel_l2(s["d"][n][0], ref["d_grads"][n][0]), rel_l2(s["d"][n][1], ref["d_grads"][n][1])) for n in ref["d_grads"]}
    ke = {n: (rel_l2(s["dw"][n][0], ref["dw"][n][0]), rel_l2(s["u"][n], ref["u"][n])) for n in ref["dw"]}
    print(f"\n{label}: |d_loss err| {figs['d_loss']:.1e}, |adversarial err| {figs['adversarial']:.1e}, worst gradient rel-L2 kernel "
          f"{max(v[0] for v in ge.values()):.1e} bias {max(v[1] for v in ge.values()):.1e}, worst kernel {max(v[0] for v in ke.values()):.1e} u {max(v[1] for v in ke.values()):.1e}")
    for n, (a, b) in ge.items():
        assert a <= 2e-4 and b <= 2e-4, (label, "gradient", n, a, b)
    for n, (a, b) in ke.items():
        assert a <= 1e-5 and b <= 1e-5, (label, "kernel / u", n, a, b)


@pytest.mark.parametrize("cfg", [(2, 1, 8, True), (2, 2, 8, False)])
def test_device_step_against_the_oracle(ctx, cfg):
    run = _device_run(ctx, cfg, second=cfg == (2, 1, 8, True))
    s = run["s1"]
    for k, v in run["ref1"]["losses"].items():           # the other four scalars travel in the same copy
        assert abs(s["out"][k] - v) <= 2e-4 * max(1.0, abs(v)), (k, s["out"][k], v)
    _check_discriminator(s, run["ref1"], f"step 1 {cfg}")
    assert s["opt"] is T.DeviceAdam and s["t"] == 1
    flat = np.concatenate([a.ravel() for n in GT.DISC_LAYERS for a in s["dw"][n]])
    assert np.array_equal(flat, s["flat"])               # tr.dw is the bucket, downloaded


def test_second_device_step_carries_its_state(ctx):
    run = _device_run(ctx, (2, 1, 8, True), second=True)
    _check_discriminator(run["s2"], run["ref2"], "step 2")
    assert run["s2"]["t"] == 2


def test_device_steps_do_not_download_the_bucket(ctx):
    """Nothing in train_step reads the discriminator's host copy: after two steps the bucket's host buffer and u's still hold the initial
    values (no refresh has run) and are marked stale; the first read of tr.dw / tr.u then downloads them."""
    scale, nb, G, att = 2, 1, 8, False
    gw, dw, vw = _gan_setup(scale, nb, G)
    lr, hr = _batch(scale)
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=att, u_seed=3, discriminator="device")
    h0, u0 = tr.d_params._hflat.copy(), tr.disc._u_host.copy()
    calls = []
    host = tr.d_params.host
    tr.d_params.host = lambda: (calls.append(1), host())[1]
    tr.train_step(lr, hr)
    tr.train_step(lr, hr)
    assert not calls and tr.d_params.stale and tr.disc._u_stale
    assert np.array_equal(tr.d_params._hflat, h0) and np.array_equal(tr.disc._u_host, u0)
    moved = tr.dw["disc_conv1"][0]
    assert calls == [1] and not tr.d_params.stale and not np.array_equal(tr.d_params._hflat, h0) and np.array_equal(moved.ravel(), tr.d_params.flat[:moved.size].cpu().numpy())
    assert not np.array_equal(np.concatenate([tr.u[n].ravel() for n in GT.DISC_LAYERS]), u0) and not tr.disc._u_stale


# ------------------------------------------------------------------------------------------------ 5. host mode and device mode
def test_host_and_device_modes_agree(ctx):
    cfg = (2, 1, 8, True)
    scale, nb, G, att = cfg
    dev = _device_run(ctx, cfg, second=True)["s1"]
    gw, dw, vw = _gan_setup(scale, nb, G)
    lr, hr = _batch(scale)
    res = []
    for kw in ({"discriminator": "host"}, {}):
        tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=att, g_lr=1e-4, d_lr=1e-5, u_seed=3, **kw)
        assert tr.d_params is None and isinstance(tr.d_opt, T.Adam)
        out = tr.train_step(lr, hr)
        res.append((out, _copy(tr.last_grads["d"]), _copy(tr.dw), {n: v.copy() for n, v in tr.u.items()}, tr.g_params.flat.cpu().numpy()))
    (o1, d1, w1, u1, g1), (o2, d2, w2, u2, g2) = res
    assert o1 == o2 and np.array_equal(g1, g2)            # the keyword's default is the code without it, bit for bit
    for n in d1:
        assert all(np.array_equal(a, b) for a, b in zip(d1[n], d2[n])) and all(np.array_equal(a, b) for a, b in zip(w1[n], w2[n])) and np.array_equal(u1[n], u2[n])
    lerr = {k: abs(dev["out"][k] - v) for k, v in o1.items()}
    gerr = {n: max(rel_l2(dev["d"][n][0], d1[n][0]), rel_l2(dev["d"][n][1], d1[n][1])) for n in d1}
    print("\nhost vs device mode: loss differences", {k: f"{v:.1e}" for k, v in lerr.items()}, "worst discriminator gradient rel-L2", f"{max(gerr.values()):.1e}")
    for k, v in o1.items():
        assert lerr[k] <= 2e-4 * max(1.0, abs(v)), (k, dev["out"][k], v)
    assert max(gerr.values()) <= 2e-4, gerr


# ------------------------------------------------------------------------------------------------ 6. the all-reduce hooks
def _after_three_renormalisations(dw, u):
    k = {n: dw[n][0].astype(np.float64) for n in GT.DISC_LAYERS}
    u = dict(u)
    for _ in range(3):
        for n in GT.DISC_LAYERS:
            k[n], u[n] = O.spectral_normalize(k[n], u[n])
    return k


@pytest.mark.parametrize("route", ["flat", "dict"])
def test_allreduce_hooks_see_the_discriminator_bucket(ctx, route):
    scale, nb, G, att = 2, 1, 8, True
    gw, dw, vw = _gan_setup(scale, nb, G)
    lr, hr = _batch(scale)
    count = lambda w: sum(int(np.prod(k.shape)) + int(np.prod(b.shape)) for k, b in w.values())
    seen = []

    def zero_flat(flat):
        seen.append(flat.numel())
        return torch.zeros_like(flat)

    def zero_dict(grads):
        seen.append(set(grads))
        return {n: tuple(np.zeros_like(a) for a in pair) for n, pair in grads.items()}
    hooks = {"allreduce_flat": zero_flat} if route == "flat" else {"allreduce": zero_dict}
    tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=att, u_seed=3, discriminator="device", **hooks)
    u0 = {n: v.copy() for n, v in tr.u.items()}
    g0 = tr.g_params.flat.cpu().numpy()
    tr.train_step(lr, hr)
    assert seen == ([count(dw), count(gw)] if route == "flat" else [set(dw), set(gw)])
    assert tr.d_opt.t == 1 and tr.g_opt.t == 1
    want = _after_three_renormalisations(dw, u0)          # a zero gradient makes Adam's step exactly zero
    for n in GT.DISC_LAYERS:
        assert rel_l2(tr.dw[n][0], want[n]) <= 1e-5, n
        assert np.array_equal(tr.dw[n][1], dw[n][1]), n
    assert np.array_equal(tr.g_params.flat.cpu().numpy(), g0)


# ------------------------------------------------------------------------------------------------ 7. determinism
def test_device_step_is_deterministic(ctx):
    scale, nb, G, att = 4, 1, 32, True
    gw, dw, vw = _gan_setup(scale, nb, G)
    lr, hr = _batch(scale)
    runs = []
    for _ in range(2):
        tr = GT.ESRGANTrainer(ctx, gw, dw, vw, scale, nb, attention=att, u_seed=3, discriminator="device")
        out = tr.train_step(lr, hr)
        assert all(np.isfinite(v) for v in out.values()), out
        runs.append((out, tr.dw["disc_conv1"][0].copy(), tr.dw["disc_output"][0].copy(), np.concatenate([tr.u[n].ravel() for n in GT.DISC_LAYERS])))
    assert runs[0][0] == runs[1][0]
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1:], runs[1][1:]))


# ------------------------------------------------------------------------------------------------ 8. the wrapper
def test_esrgan_wrapper_in_device_mode(ctx, tmp_path):
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    from sr355.wrappers import load_pretrained
    m = ESRGAN(compute_dtype="f32", discriminator_update="device")
    m.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1, use_attention=True)
    _, dw, vw = _gan_setup(2, 1, 8)
    m.set_loss_network_weights(discriminator=dw, vgg19=vw)
    rng = np.random.default_rng(12)
    X, Y = rng.uniform(0, 1, (8, 12, 12, 3)).astype(np.float32), rng.uniform(0, 1, (8, 24, 24, 3)).astype(np.float32)
    losses, _, _ = m.fit(X, Y, epochs=1, batch_size=4, shuffle_seed=42)
    assert len(losses["g_loss"]) == 2 == len(losses["d_loss"]) and np.isfinite(losses["g_loss"]).all() and np.isfinite(losses["d_loss"]).all()
    tr = m._trainer
    assert tr.discriminator == "device" and m.d_optimizer is tr.d_opt and isinstance(tr.d_opt, T.DeviceAdam) and tr.d_opt.t == 2 and tr.step == 2
    moved = max(float(np.abs(tr.dw[n][0] - dw[n][0]).max()) for n in dw)
    assert moved > 0
    gpath = m.save(str(tmp_path), "t1")
    saved = load_pretrained(gpath.replace("ESRGAN_generator", "ESRGAN_discriminator"))
    assert set(saved) == set(dw) and all(np.array_equal(saved[n][s], tr.dw[n][s]) for n in dw for s in (0, 1))
    assert np.array_equal(np.concatenate([a.ravel() for n in GT.DISC_LAYERS for a in tr.dw[n]]), tr.d_params.flat.cpu().numpy())
    new = {n: (k * np.float32(0.5), b + np.float32(0.25)) for n, (k, b) in dw.items()}
    m.set_loss_network_weights(discriminator=new)         # a live trainer follows: the values land in the device bucket
    assert np.array_equal(tr.d_params.flat.cpu().numpy(), np.concatenate([a.ravel() for n in GT.DISC_LAYERS for a in new[n]]))
    assert tr.d_opt.t == 2
    bad = ESRGAN(compute_dtype="f32", discriminator_update="gpu")
    bad.setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1, use_attention=True)
    with pytest.raises(ValueError):
        bad._ensure_trainer()
