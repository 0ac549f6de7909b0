"""tests/dense_ref.py on the CPU: the restatement against the oracle's dense block, the designed weight sets' properties, and the
checker against simulated faults of the kind the fused dense-block kernels could have.  The stand-in for the device is the same
graph in fp32 arithmetic with bf16 storage (a real, non-zero distance to the fp64 reference); c4 is kept with an explicit zero
frame, [B, H + 2, W + 2, 32], so that a fault can put something where the kernel's separator rows and seam columns are."""
import functools

import numpy as np
import pytest

import dense_ref as D
from oracle import models as M
from oracle import ops as O

SHAPES = [("initial_conv", (3, 3, 3, 64))] + [s for d in (1, 2, 3) for s in D.dense_block_shapes(f"rrdb_0_dense{d}")]
SEED = 4100
# B, H, W: the GPU module's small shapes plus one 24-wide shape for the seam fault
DOMINANCE_SHAPES = [(5, 9, 48), (4, 1, 48), (2, 17, 48), (9, 8, 48), (3, 48, 48), (7, 24, 24), (5, 9, 24), (3, 1, 24)]


def conv32(x, kb, act=None, padding="same"):
    return O.conv2d(np.asarray(x, np.float32), kb[0], kb[1], act=act, dtype=np.float32, padding=padding).astype(np.float64)


def frame(c4):
    return np.pad(c4, ((0, 0), (1, 1), (1, 1), (0, 0)))


def tail_from_frame(x, c1, c2, c3, c4f, w, name, so, conv=conv32):
    """The tail's stored output with c4 given in its frame (the frame's border is what conv5 reads beyond the image)."""
    k5, b5 = w[f"{name}_conv5"]
    n = 64 + 3 * D.G
    c5 = conv(np.concatenate([x, c1, c2, c3], axis=-1), (k5[:, :, :n], b5)) + conv(c4f, (k5[:, :, n:], None), padding="valid")
    alpha, bx, bo = D.TAIL_ALPHA[3 if so is not None else 1]
    return D.rbf(alpha * c5 + bx * x + (bo * so if so is not None else 0.0))


@functools.lru_cache(maxsize=None)
def standin(weight_set, shape):
    """The stand-in device's tensors of one RRDB: (w, {block: dict(x, c1, c2, c3, c4, out, so)})."""
    B, H, W = shape
    w = D.WEIGHT_SETS[weight_set](SHAPES, SEED)
    x = D.rbf(np.random.default_rng(B * 100 + H).uniform(-1, 1, (B, H, W, 3)))
    x0 = D.rbf(conv32(x, w["initial_conv"]))
    t, xin = {}, x0
    for d in (1, 2, 3):
        name = f"rrdb_0_dense{d}"
        f = [xin]
        for k in range(1, 5):
            f.append(D.rbf(conv32(np.concatenate(f, axis=-1), w[f"{name}_conv{k}"], act="relu")))
        so = x0 if d == 3 else None
        out = tail_from_frame(*f[:4], frame(f[4]), w, name, so)
        t[name] = dict(x=f[0], c1=f[1], c2=f[2], c3=f[3], c4=f[4], out=out, so=so)
        xin = out
    return w, t


def tail_check(weight_set, t, w, name, got):
    r = D.tail_reference(weight_set, t["x"], t["c1"], t["c2"], t["c3"], w, name, t["so"])
    return D.check(got, r["ref"], r["scale"], r["extra"])


def test_chained_restatement_is_the_oracles_dense_block():
    w = D.random_weights(SHAPES, SEED)
    x = D.rbf(np.random.default_rng(0).uniform(-1, 1, (2, 7, 11, 64)))
    for d in (1, 2, 3):
        name = f"rrdb_0_dense{d}"
        got, feats = D.dense_block_chain(x, w, name)
        assert np.array_equal(got, M._dense_block(x, w, name, np.float64, O.round_bf16))
        # dense3 with the RRDB's skip: the expression of esrgan_g_forward
        assert np.array_equal(D.tail_ref(*feats, w, name, so=x), x + got * np.float64(0.2))
        x = D.rbf(got)


def test_stream_position_follows_the_launch_arithmetic():
    # (5, 9, cap 2): T = 50, two ranges of 25 rows; row 5 of image 2 is stream row 25 = the first row of workgroup 1, local row 1
    assert D.stream_position(2, 5, 5, 9, 2, 256) == (25, 1, 1, 0, 1)
    # (3, 48, cap 0) on 256 CUs: 147 rows -> ceil(147 / 24) = 7 workgroups of 21 rows
    assert D.stream_position(1, 0, 3, 48, 0, 256)[:3] == (49, 2, 8)
    # packed pairs: image 5 rides in pair 2
    assert D.stream_position(5, 3, 7, 24, 2, 256, packed=True)[:2] == (53, 1)
    # conv1's streaming kernel cuts at >= 16 rows
    assert D.stream_position(1, 0, 3, 48, 0, 256, min_rows=16)[:2] == (49, 3)


def test_probe_conv5_set_one_hot_conv4_is_bit_exact_and_covers_taps_and_chunks():
    w, t = standin("probe_conv5", (2, 17, 48))
    for name, b in t.items():
        k4, b4 = w[f"{name}_conv4"]
        assert not b4.any() and (np.count_nonzero(k4.reshape(-1, D.G), axis=0) == 1).all()
        ky, kx, ci, co = np.nonzero(k4)
        assert set(zip(ky.tolist(), kx.tolist())) == {(i, j) for i in range(3) for j in range(3)}
        assert set((ci // 32).tolist()) == {0, 1, 2, 3, 4}
        m = np.abs(k4[ky, kx, ci, co])
        assert np.array_equal(np.log2(m), np.round(np.log2(m)))
        # fp64 restatement == the fp32 stand-in's ring, bit for bit: no allowance for conv4 in this set
        c4 = D.growth_ref([b["x"], b["c1"], b["c2"], b["c3"]], w, name, 4)
        assert np.array_equal(c4, b["c4"]) and np.array_equal(c4, D.rbf(c4)) and (c4 > 0).mean() > 0.2


def test_probe_conv4_set_conv5_copies_c4_through_every_off_centre_tap():
    w, _ = standin("probe_conv4", (2, 17, 48))
    for d in (1, 2, 3):
        k5, b5 = w[f"rrdb_0_dense{d}_conv5"]
        assert not b5.any() and not k5[:, :, :64 + 3 * D.G].any()
        ky, kx, ci, co = np.nonzero(k5)
        assert sorted(co.tolist()) == list(range(64)) and (k5[ky, kx, ci, co] == 2.0 ** D.K5_PROBE_CONV4[d]).all()
        assert ((ky == 1) & (kx == 1))[np.argsort(co)][:32].all() and np.array_equal(ci[np.argsort(co)] - 160, np.arange(64) % 32)
        assert len({(a, b) for a, b, c in zip(ky.tolist(), kx.tolist(), co.tolist()) if c >= 32}) == 8


@pytest.mark.parametrize("weight_set", ["probe_conv5", "probe_conv4"])
@pytest.mark.parametrize("shape", DOMINANCE_SHAPES)
def test_conv_term_exceeds_the_skips_in_the_median(weight_set, shape):
    """The chosen powers of two (dense_ref.K5_*), on the reference.  Median |alpha conv5| / median |skips| at (3, 48, 48), dense1 / 2 / 3:
    probe_conv5 7.1 / 7.5 / 14.6, probe_conv4 7.2 / 3.2 / 16.6; the smallest are the one-row images' (only the middle row of taps sees data):
    probe_conv5 3.5 / 2.7 / 5.7, probe_conv4 9.1 / 4.0 / 5.7."""
    w, t = standin(weight_set, shape)
    for name, b in t.items():
        r = D.tail_reference(weight_set, b["x"], b["c1"], b["c2"], b["c3"], w, name, b["so"])
        assert r["conv_median"] > r["skip_median"] > 0, (name, r["conv_median"], r["skip_median"])
        assert tail_check(weight_set, b, w, name, b["out"])["ok"]                       # and the clean stand-in passes


def test_clean_standin_passes_growth_convs():
    w, t = standin("random", (2, 17, 48))
    for name, b in t.items():
        feats = [b["x"], b["c1"], b["c2"], b["c3"]]
        for k in (1, 2, 3):
            r = D.check(feats[k], D.growth_ref(feats[:k], w, name, k))
            assert r["ok"] and r["worst"] < 1, (name, k, r)


# ------------------------------------------------------------------------------------------------ simulated faults
def _one_flagged(r, rows):
    """The checker fails, and only in the rows the fault can reach."""
    assert not r["ok"] and r["count"] >= 1, r
    assert all(ix[:2] in rows for ix in r["first"]), (r["first"], rows)


@pytest.mark.parametrize("name", ["rrdb_0_dense1", "rrdb_0_dense3"])
def test_fault_c4_nonzero_on_a_separator_row(name):
    """conv4 writing relu(bias + ...) into the separator row under image 1: conv5's dy = +1 taps of the image's last row read it."""
    w, t = standin("probe_conv4", (3, 9, 48))
    b = t[name]
    c4f = frame(b["c4"])
    inp = np.concatenate([b["x"], b["c1"], b["c2"], b["c3"]], axis=-1)
    strip = np.stack([inp[1, -1], np.zeros_like(inp[1, -1]), inp[2, 0]])[None]      # the stream around the separator: last row, zeros, next image's first row
    c4f[1, -1, 1:-1] = D.rbf(conv32(strip, w[f"{name}_conv4"], act="relu")[0, 1])
    assert c4f[1, -1].any()
    _one_flagged(tail_check("probe_conv4", b, w, name, tail_from_frame(b["x"], b["c1"], b["c2"], b["c3"], c4f, w, name, b["so"])), {(1, 8)})


def test_fault_seam_column_reads_the_neighbour_image():
    """Two-up rows: image 3's column 0 is packed column 24, whose left neighbour (packed column 23) is image 2's column 23 and must read as zero."""
    w, t = standin("probe_conv4", (5, 9, 24))
    name = "rrdb_0_dense2"
    b = t[name]
    c4f = frame(b["c4"])
    c4f[3, 1 + 4, 0] = b["c4"][2, 4, 23]
    r = tail_check("probe_conv4", b, w, name, tail_from_frame(b["x"], b["c1"], b["c2"], b["c3"], c4f, w, name, b["so"]))
    _one_flagged(r, {(3, 3), (3, 4), (3, 5)})
    assert all(ix[2] == 0 for ix in r["first"])


def test_fault_conv3_drops_one_chunk_in_one_row():
    w, t = standin("random", (2, 17, 48))
    name = "rrdb_0_dense2"
    b = t[name]
    ref = D.growth_ref([b["x"], b["c1"], b["c2"]], w, name, 3)
    assert D.check(b["c3"], ref)["ok"]
    for chunk in range(4):
        k3, b3 = w[f"{name}_conv3"]
        kz = k3.copy()
        kz[:, :, 32 * chunk:32 * chunk + 32] = 0
        bad = b["c3"].copy()
        bad[1, 8] = D.rbf(conv32(np.concatenate([b["x"], b["c1"], b["c2"]], axis=-1), (kz, b3), act="relu"))[1, 8]
        _one_flagged(D.check(bad, ref), {(1, 8)})


@pytest.mark.parametrize("name", ["rrdb_0_dense1", "rrdb_0_dense3"])
def test_fault_stale_ring_row_at_a_step_boundary(name):
    """Row 8 of an image (the first row of the second step when the range starts at the image) holding what the ring row held a step earlier."""
    w, t = standin("probe_conv4", (2, 17, 48))
    b = t[name]
    c4f = frame(b["c4"])
    c4f[0, 1 + 8] = c4f[0, 1 + 0]
    _one_flagged(tail_check("probe_conv4", b, w, name, tail_from_frame(b["x"], b["c1"], b["c2"], b["c3"], c4f, w, name, b["so"])), {(0, 7), (0, 8), (0, 9)})


@pytest.mark.parametrize("name", ["rrdb_0_dense1", "rrdb_0_dense2", "rrdb_0_dense3"])
@pytest.mark.parametrize("tap", [(0, 0), (1, 1), (2, 1)])
def test_fault_conv5_drops_one_tap_at_one_pixel(name, tap):
    w, t = standin("probe_conv5", (2, 17, 48))
    b = t[name]
    k5, _ = w[f"{name}_conv5"]
    alpha = D.TAIL_ALPHA[int(name[-1])][0]
    full = np.concatenate([b["x"], b["c1"], b["c2"], b["c3"], b["c4"]], axis=-1)
    y, x = 9, 20
    r0 = D.tail_reference("probe_conv5", b["x"], b["c1"], b["c2"], b["c3"], w, name, b["so"])
    bad = b["out"].copy()
    lost = alpha * full[1, y + tap[0] - 1, x + tap[1] - 1] @ np.asarray(k5[tap[0], tap[1]], np.float64)
    bad[1, y, x] = D.rbf(r0["ref"][1, y, x] - lost)
    r = D.check(bad, r0["ref"], r0["scale"], r0["extra"])
    _one_flagged(r, {(1, y)})
    assert all(ix[2] == x for ix in r["first"])


def test_exact_integer_case_stays_exact_in_bf16_storage():
    """What test_fused_seam_exact_integers relies on: everything conv2 and conv3 of the first block READ is an integer below 2^8."""
    x, feats = D.exact_integer_case()
    for f in feats:
        assert np.array_equal(f, np.round(f))
    assert max(float(np.abs(f).max()) for f in feats[:3]) < 256
    assert np.abs(feats[2]).max() > 128                     # ... and the density is not far below what exactness allows
