"""The device LPIPS (csrc/lpips.hip; contract in include/sr355.h) against the fp64 restatement of tests/lpips_ref.py, with seeded weights.

Bars: the project's standing fp32 bar of 1e-5.  torch fp32 on the CPU, compared with the same restatement on these inputs at
31 x 31, 35 x 47, 67 x 90, 239 x 239 and 478 x 478, showed at most: taps rel-L2 1.4e-6, taps max-abs error / max-abs value 2.2e-6, score
relative 8e-7, a term relative to the score 1.3e-6.  Each test prints its figures before it asserts.

The shapes are the smallest at which each piece can go wrong: 31 x 31 (every late map is 1 x 1), 35 x 47 (non-square, floors in the conv
stride and both pools, a 1 x 2 map), 67 x 90 (several tiles of the conv kernels), 478 x 478 (the EDA's image)."""
import numpy as np
import pytest
import torch

import lpips_ref as R
from sr355 import lpips as LP

pytestmark = pytest.mark.gpu

BAR = 1e-5
CASES = {"31x31": (2, 31, 31), "35x47": (2, 35, 47), "67x90": (2, 67, 90), "478x478": (1, 478, 478)}
_cache = {}


@pytest.fixture(scope="module")
def weights():
    return LP.seeded_weights(7)


@pytest.fixture
def loaded(ctx, weights):
    """The context with the seeded weights set; unloaded again after every test, so that no other test file sees them."""
    ctx.lpips_set_weights(weights)
    try:
        yield ctx
    finally:
        ctx.lpips_set_weights(None)


def case(loaded, weights, name):
    """Inputs, device results (raw) and the fp64 restatement of one case, computed once."""
    if name not in _cache:
        B, H, W = CASES[name]
        lr, hr = R.make_pair(B, H, W, seed=1000 + H)
        score, terms, taps = loaded.lpips(loaded.to_device(lr), loaded.to_device(hr), raw=True)
        torch.cuda.synchronize()
        _cache[name] = {"lr": lr, "hr": hr, "ref": R.lpips_u8(lr, hr, weights), "score": score.cpu().numpy(), "terms": terms.cpu().numpy(),
                        "taps": [t.cpu().numpy() for t in taps]}
    return _cache[name]


def tap_errors(got, ref):
    d = got.astype(np.float64) - ref
    return float(np.sqrt((d * d).sum() / (ref * ref).sum())), float(np.abs(d).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", list(CASES))
def test_conv2_tap_per_element(loaded, weights, name):
    """Tap 2 first: the 5x5 wide fp32 route with many couts, which nothing ran before LPIPS."""
    c = case(loaded, weights, name)
    assert c["taps"][1].shape == c["ref"]["taps"][1].shape
    l2, mx = tap_errors(c["taps"][1], c["ref"]["taps"][1])
    print(f"{name} tap2: rel-L2 {l2:.3e}  max-abs/max {mx:.3e}")
    assert l2 <= BAR and mx <= BAR


@pytest.mark.parametrize("name", list(CASES))
def test_taps_per_element(loaded, weights, name):
    c = case(loaded, weights, name)
    figs = []
    for l in range(5):
        assert c["taps"][l].shape == c["ref"]["taps"][l].shape
        assert np.isfinite(c["taps"][l]).all() and (c["taps"][l] >= 0).all()
        figs.append(tap_errors(c["taps"][l], c["ref"]["taps"][l]))
        print(f"{name} tap{l + 1} {c['taps'][l].shape}: rel-L2 {figs[-1][0]:.3e}  max-abs/max {figs[-1][1]:.3e}")
    assert all(l2 <= BAR and mx <= BAR for l2, mx in figs), figs


@pytest.mark.parametrize("name", list(CASES))
def test_terms_and_score(loaded, weights, name):
    c = case(loaded, weights, name)
    s64, t64 = c["ref"]["score"], c["ref"]["terms"]
    et = np.abs(c["terms"] - t64) / s64[:, None]
    es = np.abs(c["score"] - s64) / s64
    print(f"{name}: score {c['score']}  fp64 {s64}  |term err| / score {et.max():.3e}  |score err| / score {es.max():.3e}")
    assert (s64 > 0).all() and et.max() <= BAR and es.max() <= BAR
    s = c["terms"][:, 0]
    for l in range(1, 5):
        s = (s + c["terms"][:, l]).astype(np.float32)
    assert s.tobytes() == c["score"].tobytes()          # the score is the fp32 sum of the five terms, in tap order


def test_both_entry_forms_agree(loaded, weights):
    c = case(loaded, weights, "35x47")
    f = lambda bgr: loaded.to_device((2.0 * (bgr[..., ::-1].astype(np.float64) / 255.0) - 1.0).astype(np.float32))
    got = loaded.lpips(f(c["lr"]), f(c["hr"])).cpu().numpy()
    rel = np.abs(got.astype(np.float64) - c["score"]) / c["score"]
    print(f"uint8 {c['score']}  float32 {got}  rel {rel.max():.3e}")
    assert rel.max() <= 1e-6
    ref = R.lpips_f32(f(c["lr"]).cpu().numpy(), f(c["hr"]).cpu().numpy(), weights)["score"]
    assert (np.abs(got - ref) / ref).max() <= BAR


def test_batch_and_position_invariance(loaded):
    """Pair 3 of B = 5, alone, and in a batch that crosses an internal chunk boundary: the same bits.  At 31 x 31 a chunk is
    SR_LPIPS_CHUNK_PAIRS = 64 pairs (its maps are far below SR_LPIPS_WORK_BYTES), so B = 65 is the smallest batch with a second chunk;
    the pair sits last, alone in that chunk."""
    def run(lr, hr):
        s, t, _ = loaded.lpips(loaded.to_device(lr), loaded.to_device(hr), raw=True)
        return s.cpu().numpy(), t.cpu().numpy()

    lr, hr = R.make_pair(5, 35, 47, seed=5)
    s5, t5 = run(lr, hr)
    s1, t1 = run(lr[3:4], hr[3:4])
    assert s5[3].tobytes() == s1[0].tobytes() and t5[3].tobytes() == t1[0].tobytes()
    s5b, t5b = run(lr, hr)
    assert s5.tobytes() == s5b.tobytes() and t5.tobytes() == t5b.tobytes()

    lr, hr = R.make_pair(65, 31, 31, seed=6)
    s65, t65 = run(lr, hr)
    for i in (0, 63, 64):
        s1, t1 = run(lr[i:i + 1], hr[i:i + 1])
        assert s65[i].tobytes() == s1[0].tobytes() and t65[i].tobytes() == t1[0].tobytes(), i
    # the same pair at position 3 of the first chunk and alone in the second
    lr[3], hr[3] = lr[64], hr[64]
    s, t = run(lr, hr)
    assert s[3].tobytes() == s[64].tobytes() and t[3].tobytes() == t[64].tobytes()


def test_exact_cases(ctx, loaded, weights):
    lr, hr = R.make_pair(2, 31, 31, seed=9)
    x = loaded.to_device(hr)
    s, t, _ = loaded.lpips(x, x, raw=True)
    assert (s.cpu().numpy() == 0.0).all() and (t.cpu().numpy() == 0.0).all()
    const = loaded.to_device(np.full_like(hr, 93))
    s = loaded.lpips(const, x).cpu().numpy()
    assert np.isfinite(s).all() and (s > 0).all()
    zero = loaded.to_device(np.zeros_like(hr))
    assert np.isfinite(loaded.lpips(zero, x).cpu().numpy()).all()
    # tap 5 all zero: its pixels normalise to zeros, never to NaN
    w = {k: [a.copy() for a in v] for k, v in weights.items()}
    w["conv_b"][4] -= 100.0
    try:
        ctx.lpips_set_weights(w)
        s, t, taps = ctx.lpips(loaded.to_device(lr), x, raw=True)
        s, t = s.cpu().numpy(), t.cpu().numpy()
        assert (taps[4].cpu().numpy() == 0.0).all()
        assert (t[:, 4] == 0.0).all() and np.isfinite(s).all() and (s > 0).all()
        four = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
        assert s.tobytes() == four.astype(np.float32).tobytes()
    finally:
        ctx.lpips_set_weights(None)


def test_eda_integration(ctx, weights, tmp_path):
    import data.eda_methods as E
    A, M = E.ImageDatasetAnalyzer, E.MetricsAggregator
    alex, lins = LP.to_state_dicts(weights)
    pa, pl = str(tmp_path / "alexnet.pth"), str(tmp_path / "alex.pth")
    torch.save({k: torch.from_numpy(v) for k, v in alex.items()}, pa)
    torch.save({k: torch.from_numpy(v) for k, v in lins.items()}, pl)
    lr, hr = R.make_pair(5, 64, 64, seed=11)
    rows0, g0 = M.collect_arrays(lr, hr)
    assert all(np.isnan(r.lpips) for r in rows0)
    try:
        A.load_lpips(pa, pl)
        rows, g = M.collect_arrays(lr, hr)
        want = ctx.lpips(ctx.to_device(lr), ctx.to_device(hr)).cpu().numpy()
        for i, (r, r0) in enumerate(zip(rows, rows0)):
            assert isinstance(r.lpips, float) and np.float32(r.lpips).tobytes() == want[i].tobytes()
            d, d0 = r.as_dict(), r0.as_dict()
            assert list(d) == list(d0)
            for k in d:
                if k not in ("lpips", "filename"):
                    assert np.float64(d[k]).tobytes() == np.float64(d0[k]).tobytes(), k
        for k in ("lr_fft_sum", "hr_fft_sum", "grad_hr_sum", "glcm_sum"):
            assert np.array_equal(g[k], g0[k])
        assert A.lpips_score(lr[0], hr[0]) == rows[0].lpips
        to_tensor = lambda img: torch.from_numpy(np.transpose(2 * (img[..., ::-1] / 255.0) - 1, (2, 0, 1)).copy()).unsqueeze(0).float()
        assert A.loss_fn()(to_tensor(lr[0]), to_tensor(hr[0])).item() == rows[0].lpips
        best, worst = E.StatsReporter.lpips_scenarios(E.StatsReporter.dataframe(rows), top_k=2)
        order = np.argsort(want, kind="stable")
        assert best == [str(i) for i in order[:2]] and worst == [str(i) for i in order[-2:]]
    finally:
        A.unload_lpips()
    with pytest.raises(NotImplementedError, match="LPIPS"):
        A.lpips_score(lr[0], hr[0])
    with pytest.raises(NotImplementedError, match="LPIPS"):
        A.loss_fn()
    assert all(np.isnan(r.lpips) for r in M.collect_arrays(lr, hr)[0])


def test_refusals(ctx, weights):
    ctx.lpips_set_weights(None)
    lr, hr = R.make_pair(1, 31, 31, seed=2)
    with pytest.raises(RuntimeError, match="weights are not set"):
        ctx.lpips(ctx.to_device(lr), ctx.to_device(hr))
    try:
        ctx.lpips_set_weights(weights)
        z = lambda *s: torch.zeros(s, dtype=torch.uint8, device=ctx.torch_device)
        with pytest.raises(ValueError):
            ctx.lpips(z(1, 30, 40, 3), z(1, 30, 40, 3))
        with pytest.raises(ValueError):
            ctx.lpips(z(1, 31, 40, 3), z(1, 31, 41, 3))
        with pytest.raises(ValueError):
            ctx.lpips(z(2, 40, 40), z(2, 40, 40))
        with pytest.raises(ValueError):
            ctx.lpips(z(1, 40, 40, 3), z(1, 40, 40, 3).float())
        with pytest.raises(ValueError):
            ctx.lpips(z(1, 40, 40, 3).cpu(), z(1, 40, 40, 3))
        with pytest.raises(ValueError):
            ctx.lpips_set_weights({"conv_w": weights["conv_w"][:4], "conv_b": weights["conv_b"], "lin_w": weights["lin_w"]})
        bad = {k: list(v) for k, v in weights.items()}
        bad["conv_w"][0] = bad["conv_w"][0][:, :10]
        with pytest.raises(ValueError):
            ctx.lpips_set_weights(bad)
        # the refused calls left the loaded weights in place
        assert float(ctx.lpips(ctx.to_device(lr), ctx.to_device(hr))[0]) > 0
    finally:
        ctx.lpips_set_weights(None)
