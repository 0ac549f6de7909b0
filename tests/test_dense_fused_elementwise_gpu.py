"""Every launch of the fused dense-block kernels (csrc/dense_fused.hip: dense_conv1_stream<bf16,64->32>, dense_pair_fused<bf16>,
dense_tail_fused<bf16,conv4+conv5>, plain and SEAM) per element against an fp64 restatement fed with the device's own inputs
(tests/dense_ref.py): one forward with taps on initial_conv and on conv1, conv2, conv3 and conv5 of every dense block -- never conv4,
whose tap would switch the tail pair back to layer by layer -- gives the bf16 tensors each launch read and wrote, so nothing compounds
through the network and a single wrong element fails the bf16 contract (dense_ref.assert_bf16_close).

Three weight sets (dense_ref.WEIGHT_SETS):
  random       conv1, conv2 and conv3 of every block per element, two RRDBs (conv3 from the device's own c2: ring and memory hold the same
               bf16 value, see dense_ref's docstring).  The tail is left to test_dense_fused_gpu.py's aggregates: its skip (rms 0.17) hides
               0.2 * conv5 (rms 0.034) and conv4's rounding flips would need an allowance many times the bound.
  probe_conv5  conv4 one-hot (exact in bf16, so the fp64 c4 IS the ring's), conv5 random times 2^k: the tail's output per element, no allowance.
  probe_conv4  conv4 random, conv5 copying 2^k c4 through the centre tap (couts 0..31) and every off-centre tap (couts 32..63): conv4's sums, its
               zero separator rows, the ring across step and range boundaries and the seam columns 23 | 24, with the one derived allowance
               alpha 2^k spacing_bf16(c4) for the ring's own rounding.
Both designed sets run one RRDB: dense1 / dense2 (alpha 0.2, xscale 5) and dense3 (alpha 0.04, xscale 5, oscale 25: the second skip)."""
import numpy as np
import pytest
import torch

import dense_ref as D
from sr355 import Context, Model

pytestmark = pytest.mark.gpu

CONV1, PAIR, TAIL = "dense_conv1_stream<bf16,64->32>", "dense_pair_fused<bf16>", "dense_tail_fused<bf16,conv4+conv5>"
TILE_GROWTH = "conv_rows<bf16,k3,kg1,nt2>"            # a dense-block growth conv on the tile kernel

# mask name -> (mask, fused kernels that must have run; the others must not have)
MASKS = {
    "mid": (Context.FUSED_DENSE_MID, {PAIR}),
    "tail": (Context.FUSED_DENSE_TAIL, {TAIL}),
    "conv1": (Context.FUSED_CONV1_STREAM, {CONV1}),
    "three": (Context.FUSED_TWO_UP, {CONV1, PAIR, TAIL}),         # on 48-pixel rows: all three fused kernels, no seam
    "all": (Context.FUSED_ALL, {CONV1, PAIR, TAIL}),              # on 24-pixel rows: two-up, the SEAM instances
}
# (B, H, W, grid cap): the smallest shapes that cut the row stream everywhere it can be cut (>= 24 rows per workgroup, 8-row steps, one separator per image)
CASES_48 = [
    (5, 9, 48, 2),       # height not a multiple of the step; two ranges of 25 rows, the cut inside the third image
    (4, 1, 48, 3),       # one-row images: every second stream row a separator, one range
    (2, 17, 48, 0),      # two ranges of 18 rows that meet exactly at the image boundary; a third step of one row
    (9, 8, 48, 4),       # height == step; four ranges of 21 rows, cutting images 2, 4 and 7
]
BENCH_CASE = (3, 48, 48, 0)  # the bench shape: 147 rows -> 7 ranges of 21 rows, every cut inside an image
CASES_24 = [
    (7, 24, 24, 2),      # an odd batch: the last pair's right half is padding; two ranges of 50 rows
    (5, 9, 24, 3),       # two ranges of 15 rows: a cut in the middle of the second pair
    (3, 1, 24, 0),       # one-row pairs
]
PARAMS = ([(c, mk, "random") for c in CASES_48 for mk in ("mid", "tail", "conv1", "three")]
          + [(c, mk, ws) for c in CASES_48 for ws in ("probe_conv5", "probe_conv4") for mk in ("tail", "three")]
          + [(BENCH_CASE, "three", ws) for ws in D.WEIGHT_SETS]
          + [(c, "all", ws) for c in CASES_24 for ws in D.WEIGHT_SETS])
SEEDS = {"random": 4000, "probe_conv5": 4100, "probe_conv4": 4100}
NUM_BLOCKS = {"random": 2, "probe_conv5": 1, "probe_conv4": 1}

_MODELS = {}


def model_of(ctx, weight_set):
    if weight_set not in _MODELS:
        m = Model("esrgan_g", compute_dtype="bf16", scale_factor=2, num_blocks=NUM_BLOCKS[weight_set], growth_channels=32, use_attention=False, ctx=ctx)
        w = D.WEIGHT_SETS[weight_set](m.layer_shapes(), SEEDS[weight_set])
        m.set_weights(w)
        _MODELS[weight_set] = (m, w)
    return _MODELS[weight_set]


@pytest.fixture()
def fused_ctx(ctx):
    yield ctx
    ctx.set_fused(ctx.FUSED_ALL, 0)


@pytest.mark.parametrize("case,mask_name,weight_set", PARAMS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_every_launch_per_element(fused_ctx, case, mask_name, weight_set):
    ctx = fused_ctx
    B, H, W, cap = case
    mask, fused = MASKS[mask_name]
    m, w = model_of(ctx, weight_set)
    nb = NUM_BLOCKS[weight_set]
    x = D.rbf(np.random.default_rng(B * 1000 + H * 10 + W).uniform(-1, 1, (B, H, W, 3)))
    xd = ctx.to_device(x.astype(np.float32), torch.bfloat16)
    blocks = [f"rrdb_{b}_dense{d}" for b in range(nb) for d in (1, 2, 3)]
    names = ["initial_conv"] + [f"{n}_conv{k}" for n in blocks for k in (1, 2, 3, 5)]
    ctx.set_fused(mask, cap)
    ctx.profile_begin()
    _, taps = m.forward_with_taps(xd, names)
    ran = {r["kernel"] for r in ctx.profile_end()}
    # the kernels under test ran, the others did not, and in the all-fused configurations no growth conv ran on the tile kernel
    assert fused <= ran and not (({CONV1, PAIR, TAIL} - fused) & ran), (mask_name, ran)
    if len(fused) == 3:
        assert not any(k.startswith(TILE_GROWTH) for k in ran), ran
    t = {n: v.cpu().numpy().astype(np.float64) for n, v in taps.items()}
    assert all(v.shape[:3] == (B, H, W) for v in t.values())
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    packed = W == 24

    def locate(min_rows):
        def f(img, y):
            g, wg, l, step, ring = D.stream_position(img, y, B, H, cap, ncu, packed, min_rows)
            return f"stream row {g}, workgroup {wg}, local row {l}, step {step}, ring row {ring}"
        return f

    tag = f"{weight_set} {case} {mask_name}"
    for bi, name in enumerate(blocks):
        d = int(name[-1])
        xin = t["initial_conv"] if bi == 0 else t[blocks[bi - 1] + "_conv5"]
        c1, c2, c3, out = (t[f"{name}_conv{k}"] for k in (1, 2, 3, 5))
        so = None
        if d == 3:                                                            # the RRDB's input: initial_conv or the previous RRDB's output
            so = t["initial_conv"] if bi < 3 else t[blocks[bi - 3] + "_conv5"]
        if weight_set == "random":
            for k, feats, got, kern in ((1, [xin], c1, CONV1), (2, [xin, c1], c2, PAIR), (3, [xin, c1, c2], c3, PAIR)):
                ref = D.memo((weight_set, name, k), lambda *f: D.growth_ref(list(f), w, name, k), *feats)
                worst = D.assert_bf16_close(got, ref, what=f"{tag} {name}_conv{k}", locate=locate(16 if k == 1 else 24))
                print(f"RATIO {kern if kern in fused else 'tile'} conv{k} {tag} {name} {worst:.4f}")
        else:
            r = D.memo((weight_set, name, 5), lambda *f: D.tail_reference(weight_set, *f[:4], w, name, f[4] if d == 3 else None),
                       xin, c1, c2, c3, *([so] if d == 3 else []))
            # the designed set does what it was designed for on THIS case: the conv term stands above the skips in the median
            assert r["conv_median"] > r["skip_median"] > 0, (tag, name, r["conv_median"], r["skip_median"])
            worst = D.assert_bf16_close(out, r["ref"], scale=r["scale"], extra=r["extra"], what=f"{tag} {name}_conv5", locate=locate(24))
            print(f"RATIO {TAIL if TAIL in fused else 'tile'} {weight_set} {tag} {name} {worst:.4f} median-ratio {r['conv_median'] / r['skip_median']:.2f}")
