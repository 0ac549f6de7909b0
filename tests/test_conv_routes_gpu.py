"""One case per kernel variant conv_launch can pick (csrc/conv.hip conv_route), each asserting the variant it reached.

Every case runs sr_conv2d twice against the fp64 oracle:
- on seeded normal data with the kernel-level contracts of test_kernels_gpu.py: fp32 rel-L2 <= 1e-5, bf16 every element within
  one bf16 ulp of the bf16-rounded fp64 result;
- on small integers (inputs, weights, biases, skips; alpha and betas powers of two): every partial sum is an integer far below 2^24,
  so fp32 accumulation in any order is exact and the result must equal the oracle bit for bit (bf16: its round-to-nearest-even).
  A wrong tap, halo, channel or cout index is then a mismatch, not a tolerance miss.
The output goes into the middle of a NaN-filled buffer: the bytes around it must come back untouched (padded couts, ragged tiles and
the scalar epilogue must not store outside [y, y + B*H*W*Cout)).

The grid-size variants of the fp32 wide kernel (split K, 8 x 16 and 24 x 16 tiles) are chosen by the number of workgroups against the
device's CU count, so their shapes are derived from that count here.  The largest (24 x 16 tiles) cases keep Cin small, so that their
full fp64 oracle stays around a second of CPU time; no crops are needed.
"""
import numpy as np
import pytest
import torch

from oracle import models as M
from oracle import ops as O
from sr355 import Model
from sr355 import _lib as L
from sr355.runtime import _fptr
from sr355.weights import init_weights, round_to_bf16

pytestmark = pytest.mark.gpu

ACT = {"linear": L.ACT_LINEAR, "relu": L.ACT_RELU, "lrelu": L.ACT_LRELU, "tanh": L.ACT_TANH}
GUARD = 4096                      # bytes of NaN on either side of the output
NAN_BITS = {"f32": 0x7FC0DEAD, "bf16": 0x7FDE}


@pytest.fixture
def route_ctx(ctx):
    ctx.set_fused(ctx.FUSED_ALL, 0)
    ctx.conv_routes(False)
    yield ctx
    ctx.conv_routes(False)
    ctx.set_fused(ctx.FUSED_ALL, 0)


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def rel_l2(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def assert_bf16_close(got, ref, scale=1.0, rel=1e-3):
    """test_kernels_gpu.py's bf16 contract: got the device's bf16 result, ref the fp64 oracle before the storage rounding."""
    refq = O.round_bf16(np.asarray(ref, np.float64))
    d = np.abs(np.asarray(got, np.float64) - refq)
    bound = 2.0 ** -7 * np.abs(refq) + 3e-5 * scale
    bad = d > bound
    assert not bad.any(), (int(bad.sum()), float(d.max()), float((d / bound).max()))
    assert rel_l2(got, refq) <= rel


# ------------------------------------------------------------------------------------------------ shapes of the grid-size variants
def _wide_grid(B, H, W, nct):
    """(workgroups of the 8 x 16 tiling, of the 24 x 16 tiling) of an fp32 wide conv, as conv_route counts them."""
    tx = (W + 15) // 16
    return tx * -(-H // 8) * B * nct, tx * -(-H // 24) * B * nct


def _nct(Cout, K, Cin):
    """cout tiles per pixel tile of an fp32 wide conv (conv_plan's NT choice)."""
    nb = -(-Cout // 32)
    nt = 2 if nb % 2 == 0 else (3 if nb % 3 == 0 else 1)
    if K == 5:
        nt = 1
    return nb // nt


def _h_for(sub, B, W, K, Cin, Cout):
    """An image height that puts an fp32 wide conv of [B, ., W] on variant `sub`, with a ragged last tile."""
    cu, nct = cu_count(), _nct(Cout, K, Cin)
    tx = (W + 15) // 16
    if sub == "mt3":                                   # at least two 24 x 16 tiles per CU
        n = -(-2 * cu // (tx * B * nct))
        H = 24 * (n - 1) + 19
    elif sub == "mt1" and K == 3:                      # split K would have at least one 8 x 16 tile per CU: not taken
        n = -(-cu // (tx * B * nct))
        H = 8 * (n - 1) + 5
    else:                                              # mt1 of 1x1 / 5x5, and split K: small images
        H = 13
    wgs1, wgs3 = _wide_grid(B, H, W, nct)
    assert {"sk": wgs1 < cu, "mt1": wgs3 < 2 * cu and (K != 3 or wgs1 >= cu), "mt3": wgs3 >= 2 * cu}[sub], (sub, H, wgs1, wgs3, cu)
    return H


# ------------------------------------------------------------------------------------------------ the route table
# (id, dtype, B, H, W, Cin, Cout, K, epilogue, expected route); H None: derived from the CU count (_h_for, variant = the route's suffix)
# epilogues: "relu" / "linear" / "tanh": act alone; "full": alpha, two skips, lrelu, clip01; "d2s": depth_to_space 2;
# "skip1x" / "skip2x": the input itself is skip 1 (alone) / skip 2 (another tensor is skip 1), linear -- a dense-block tail
def _fp32_wide():
    out = []
    # 3x3 from 40 channels (2.5 chunks of 16); NT 1 / 2 / 3; cout 20 / 62 / 90 (62: not a multiple of 4 -> scalar epilogue)
    for nt, cout in ((1, 20), (2, 62), (3, 90)):
        out.append((f"f32-k3-nt{nt}-sk", "f32", 2, 13, 21, 40, cout, 3, "relu", f"wide<f32,k3,kg2,nt{nt}>/sk"))
        out.append((f"f32-k3-nt{nt}-mt1", "f32", 2, None, 37, 12, cout, 3, "relu", f"wide<f32,k3,kg2,nt{nt}>/mt1"))
    # 24 x 16 tiles: more cout tiles per pixel tile keep the image (and the CPU oracle) small: nb 5 -> NT 1 x 5, nb 6 -> NT 2 x 3, nb 9 -> NT 3 x 3
    for nt, cout in ((1, 150), (2, 190), (3, 282)):
        out.append((f"f32-k3-nt{nt}-mt3", "f32", 2, None, 37, 12, cout, 3, "relu", f"wide<f32,k3,kg2,nt{nt}>/mt3"))
    # 1x1: KGPT 2 (Cin rounds to 16 / 48 channels) and 4 (to 32 / 64); one image too small for 24 x 16 tiles, one large enough
    for kg, cin, cin3 in ((2, 40, 12), (4, 60, 28)):
        for nt, cout in ((1, 20), (2, 62), (3, 90)):
            out.append((f"f32-k1-kg{kg}-nt{nt}-mt1", "f32", 2, 13, 21, cin, cout, 1, "relu", f"wide<f32,k1,kg{kg},nt{nt}>/mt1"))
        for nt, cout in ((1, 150), (2, 190), (3, 282)):
            out.append((f"f32-k1-kg{kg}-nt{nt}-mt3", "f32", 2, None, 37, cin3, cout, 1, "relu", f"wide<f32,k1,kg{kg},nt{nt}>/mt3"))
    out.append(("f32-k5-mt1", "f32", 2, 13, 21, 12, 40, 5, "relu", "wide<f32,k5,kg2,nt1>/mt1"))
    out.append(("f32-k5-mt3", "f32", 1, None, 37, 6, 140, 5, "relu", "wide<f32,k5,kg2,nt1>/mt3"))
    # epilogues on the three tilings
    out.append(("f32-k3-sk-full", "f32", 2, 11, 13, 24, 64, 3, "full", "wide<f32,k3,kg2,nt2>/sk"))
    out.append(("f32-k3-sk-d2s", "f32", 1, 7, 9, 24, 12, 3, "d2s", "wide<f32,k3,kg2,nt1>/sk"))
    out.append(("f32-k1-mt1-full", "f32", 2, 9, 21, 40, 64, 1, "full", "wide<f32,k1,kg2,nt2>/mt1"))
    out.append(("f32-k1-mt1-d2s", "f32", 2, 9, 5, 64, 36, 1, "d2s", "wide<f32,k1,kg4,nt2>/mt1"))
    out.append(("f32-k3-mt1-tanh", "f32", 2, None, 37, 12, 20, 3, "tanh", "wide<f32,k3,kg2,nt1>/mt1"))
    return out


def _with_h(cases):
    out = []
    for c in cases:
        if c[3] is None:
            sub = c[9].rsplit("/", 1)[1]
            c = c[:3] + (("auto", sub),) + c[4:]
        out.append(c)
    return out


ROUTES = _with_h(_fp32_wide()) + [
    # few: fp32, <= 4 couts; 3x3 / 5x5 x whole channel depth in LDS (<= 80 KiB) / 4 channels at a time
    ("few-k3-lds", "f32", 2, 19, 21, 50, 3, 3, "relu", "few<f32,k3>/lds"),
    ("few-k3-direct", "f32", 2, 19, 13, 60, 3, 3, "relu", "few<f32,k3>/direct"),
    ("few-k5-lds", "f32", 2, 17, 35, 30, 3, 5, "relu", "few<f32,k5>/lds"),
    ("few-k5-direct", "f32", 1, 33, 21, 64, 3, 5, "relu", "few<f32,k5>/direct"),
    ("few-k3-h1", "f32", 3, 1, 37, 8, 2, 3, "linear", "few<f32,k3>/lds"),
    ("few-k3-full", "f32", 2, 11, 18, 16, 4, 3, "full", "few<f32,k3>/lds"),
    ("few-k5-d2s", "f32", 1, 9, 7, 40, 4, 5, "d2s", "few<f32,k5>/direct"),
    # thin: one 16-byte slice per pixel holds every input channel (4 fp32 / 8 bf16)
    ("thin-f32-k3", "f32", 2, 20, 37, 3, 64, 3, "relu", "thin<f32,k3,nt1,nv4>"),
    ("thin-f32-k5", "f32", 2, 17, 13, 4, 40, 5, "relu", "thin<f32,k5,nt1,nv4>"),
    ("thin-f32-k9", "f32", 1, 26, 19, 3, 32, 9, "relu", "thin<f32,k9,nt1,nv4>"),
    ("thin-f32-k9-head", "f32", 2, 27, 21, 3, 96, 9, "relu", "thin<f32,k9,nt1,nv3>"),
    ("thin-f32-k3-h1", "f32", 2, 1, 9, 2, 36, 3, "linear", "thin<f32,k3,nt1,nv4>"),
    ("thin-bf16-k3", "bf16", 2, 20, 37, 3, 64, 3, "relu", "thin<bf16,k3,nt1,nv4>"),
    ("thin-bf16-k5", "bf16", 1, 17, 13, 8, 40, 5, "relu", "thin<bf16,k5,nt1,nv4>"),
    ("thin-bf16-k9", "bf16", 2, 26, 19, 5, 96, 9, "relu", "thin<bf16,k9,nt1,nv4>"),
    ("thin-f32-full", "f32", 2, 25, 19, 3, 64, 3, "full", "thin<f32,k3,nt1,nv4>"),
    ("thin-bf16-full", "bf16", 2, 25, 19, 3, 64, 3, "full", "thin<bf16,k3,nt1,nv4>"),
    ("thin-f32-d2s", "f32", 1, 11, 14, 3, 12, 3, "d2s", "thin<f32,k3,nt1,nv4>"),
    # 1x1 from a thin input: the wide / 1x1 kernels on zero-padded channels
    ("k1-rgb-f32", "f32", 2, 11, 21, 3, 64, 1, "relu", "wide<f32,k1,kg2,nt2>/mt1"),
    ("k1-rgb-bf16", "bf16", 2, 11, 21, 3, 32, 1, "relu", "pw<bf16,nb2,nch1>"),
    ("k1-rgb-bf16-wide", "bf16", 1, 9, 13, 8, 96, 1, "relu", "wide<bf16,k1,kg2,nt3>/mt3"),
    # bf16 wide: 1x1 too wide for the register-resident kernel, KGPT 2 / 4; 5x5
    ("bf16-k1-kg2", "bf16", 2, 9, 21, 160, 64, 1, "relu", "wide<bf16,k1,kg2,nt2>/mt3"),
    ("bf16-k1-kg4", "bf16", 2, 9, 21, 256, 64, 1, "relu", "wide<bf16,k1,kg4,nt2>/mt3"),
    ("bf16-k1-kg4-nt3", "bf16", 1, 25, 13, 240, 90, 1, "relu", "wide<bf16,k1,kg4,nt3>/mt3"),
    ("bf16-k5", "bf16", 2, 17, 21, 20, 40, 5, "relu", "wide<bf16,k5,kg2,nt1>/mt3"),
    ("bf16-k5-full", "bf16", 1, 13, 19, 24, 32, 5, "full", "wide<bf16,k5,kg2,nt1>/mt3"),
    ("bf16-k5-d2s", "bf16", 1, 9, 11, 24, 12, 5, "d2s", "wide<bf16,k5,kg2,nt1>/mt3"),
] + [
    # pw: bf16 1x1 with the whole weight matrix in registers, every (16-cout blocks, 32-channel chunks) instantiation
    (f"pw-{nb}x{nch}", "bf16", 2, 7 + nb, 13 + 8 * nch, 32 * nch - 8 * (nb % 2), 16 * nb - (3 if nb == 3 else 4 * (nb % 2)), 1, "relu",
     f"pw<bf16,nb{nb},nch{nch}>")
    for nb, nch in ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 3), (4, 1))
] + [
    ("pw-h1", "bf16", 3, 1, 5, 64, 32, 1, "relu", "pw<bf16,nb2,nch2>"),
    ("pw-full", "bf16", 2, 9, 21, 64, 48, 1, "full", "pw<bf16,nb3,nch2>"),
    # rows: bf16 3x3, 16-cout blocks per workgroup NB16 = 1 / 2 / 4; the skip read from the staged input
    ("rows-nb1", "bf16", 2, 19, 21, 40, 48, 3, "relu", "rows<bf16,nb1>"),
    ("rows-nb2", "bf16", 2, 19, 21, 72, 32, 3, "relu", "rows<bf16,nb2>"),
    ("rows-nb4", "bf16", 2, 13, 21, 96, 64, 3, "relu", "rows<bf16,nb4>"),
    ("rows-nb1-ragged", "bf16", 1, 9, 7, 32, 12, 3, "relu", "rows<bf16,nb1>"),
    ("rows-nb4-h1", "bf16", 3, 1, 23, 64, 64, 3, "relu", "rows<bf16,nb4>"),
    ("rows-skip1-lds", "bf16", 2, 13, 21, 64, 64, 3, "skip1x", "rows<bf16,nb4>/skip_lds"),
    ("rows-skip2-lds", "bf16", 2, 26, 18, 64, 64, 3, "skip2x", "rows<bf16,nb4>/skip_lds"),
    ("rows-skip1-lds-wide", "bf16", 2, 7, 5, 128, 128, 3, "skip1x", "rows<bf16,nb4>/skip_lds"),
    ("rows-full", "bf16", 2, 26, 18, 64, 64, 3, "full", "rows<bf16,nb4>"),
    ("rows-d2s", "bf16", 1, 9, 13, 32, 64, 3, "d2s", "rows<bf16,nb4>"),
    # stream: bf16 3x3 from 64 channels, 64-cout tiles, whole 24 x 16 tiles
    ("stream", "bf16", 2, 48, 32, 64, 64, 3, "relu", "stream<bf16,nb4>"),
    ("stream-d2s", "bf16", 1, 24, 16, 64, 128, 3, "d2s", "stream<bf16,nb4>"),
]

# every variant conv_route names that sr_conv2d reaches (the fused epilogues and the fused 9x9 + 1x1 head are model-forward only: below)
EXPECTED_ROUTES = (
    {f"few<f32,k{k}>/{s}" for k in (3, 5) for s in ("lds", "direct")}
    | {f"thin<{d},k{k},nt1,nv4>" for d in ("f32", "bf16") for k in (3, 5, 9)} | {"thin<f32,k9,nt1,nv3>"}
    | {f"wide<f32,k3,kg2,nt{n}>/{s}" for n in (1, 2, 3) for s in ("sk", "mt1", "mt3")}
    | {f"wide<f32,k1,kg{g},nt{n}>/{s}" for g in (2, 4) for n in (1, 2, 3) for s in ("mt1", "mt3")}
    | {f"wide<f32,k5,kg2,nt1>/{s}" for s in ("mt1", "mt3")}
    | {"wide<bf16,k1,kg2,nt2>/mt3", "wide<bf16,k1,kg4,nt2>/mt3", "wide<bf16,k5,kg2,nt1>/mt3"}
    | {f"pw<bf16,nb{nb},nch{nch}>" for nb, nch in ((1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 3), (4, 1))}
    | {f"rows<bf16,nb{n}>" for n in (1, 2, 4)} | {"rows<bf16,nb4>/skip_lds", "stream<bf16,nb4>"}
)


def test_route_table_covers_every_variant():
    assert EXPECTED_ROUTES <= {c[9] for c in ROUTES}, sorted(EXPECTED_ROUTES - {c[9] for c in ROUTES})


# ------------------------------------------------------------------------------------------------ one call
def _data(rng, shape, exact, bf16, lo=-3, hi=3, scale=1.0):
    if exact:
        a = rng.integers(lo, hi + 1, shape).astype(np.float32)
    else:
        a = (rng.standard_normal(shape) * scale).astype(np.float32)
    return round_to_bf16(a) if bf16 else a


def _epilogue(ep, exact):
    """(act, alpha, skips, beta1, beta2, clip01, d2s)"""
    if ep == "full":
        return ("relu", 2.0, 2, 1.0, 0.5, False, 1) if exact else ("lrelu", 0.3, 2, 1.0, 0.2, True, 1)
    if ep in ("skip1x", "skip2x"):
        return ("linear", 2.0 if exact else 0.2, ep, 1.0, 0.5 if exact else 0.2, False, 1)
    if ep == "d2s":
        return ("relu", 1.0, 0, 0.0, 0.0, False, 2)
    if ep == "tanh" and exact:
        return ("relu", 1.0, 0, 0.0, 0.0, False, 1)
    return (ep, 1.0, 0, 0.0, 0.0, False, 1)


def run_conv(ctx, x, w, b, dtype, act="linear", alpha=1.0, skip1=None, beta1=0.0, skip2=None, beta2=0.0, clip01=False, d2s=1):
    """sr_conv2d with y placed GUARD bytes into a NaN-filled buffer; skip1 / skip2 may be the string "x" (the input tensor itself).
    Returns (y as fp32 NumPy, the conv variants logged, whether the guard bytes came back untouched)."""
    td, esz = (torch.float32, 4) if dtype == "f32" else (torch.bfloat16, 2)
    itd = torch.int32 if dtype == "f32" else torch.int16
    B, H, W, Cin = x.shape
    K, Cout = w.shape[0], w.shape[3]
    r = d2s
    xd = ctx.to_device(x, td)
    skd = [None if s is None else (xd if isinstance(s, str) else ctx.to_device(s, td)) for s in (skip1, skip2)]
    n = B * H * r * W * r * (Cout // (r * r))
    g = GUARD // esz
    buf = torch.empty(n + 2 * g, dtype=td, device=xd.device)
    bits = NAN_BITS[dtype]
    buf.view(itd).fill_(bits)
    y = buf[g:g + n]
    ctx.conv_routes(True)
    ctx.check(ctx.lib.sr_conv2d(ctx.h, xd.data_ptr(), L.DTYPE_F32 if dtype == "f32" else L.DTYPE_BF16, B, H, W, Cin, _fptr(w), _fptr(b), K, K, Cout,
                                ACT[act], float(alpha), None if skd[0] is None else skd[0].data_ptr(), float(beta1),
                                None if skd[1] is None else skd[1].data_ptr(), float(beta2), int(bool(clip01)), r, y.data_ptr(), ctx.stream()))
    torch.cuda.synchronize()
    routes = ctx.conv_routes(False)
    guard = torch.cat([buf[:g], buf[g + n:]]).view(itd)
    untouched = bool((guard == bits).all().item())
    return y.float().cpu().numpy().reshape(B, H * r, W * r, Cout // (r * r)), routes, untouched


def _case(case, exact):
    cid, dtype, B, H, W, Cin, Cout, K, ep, route = case
    if isinstance(H, tuple):
        H = _h_for(H[1], B, W, K, Cin, Cout)
    bf = dtype == "bf16"
    rng = np.random.default_rng(abs(hash((cid, exact))) % (2 ** 31))
    x = _data(rng, (B, H, W, Cin), exact, bf)
    w = _data(rng, (K, K, Cin, Cout), exact, bf, -2, 2, 1.0 / np.sqrt(K * K * Cin))
    b = rng.integers(-4, 5, Cout).astype(np.float32) if exact else rng.uniform(-0.1, 0.1, Cout).astype(np.float32)
    act, alpha, skips, beta1, beta2, clip01, r = _epilogue(ep, exact)
    s1 = s2 = None
    if skips == 2:
        s1 = _data(rng, (B, H, W, Cout), exact, bf, scale=0.5)
        s2 = _data(rng, (B, H, W, Cout), exact, bf, scale=0.5)
    elif skips == "skip1x":
        s1 = "x"
    elif skips == "skip2x":
        s1 = _data(rng, (B, H, W, Cout), exact, bf, scale=0.5)
        s2 = "x"
    ref = alpha * O.conv2d(x, w, b, act=act, dtype=np.float64)
    for s, beta in ((s1, beta1), (s2, beta2)):
        if s is not None:
            ref = ref + beta * (x if isinstance(s, str) else s).astype(np.float64)
    if clip01:
        ref = np.clip(ref, 0.0, 1.0)
    if r > 1:
        ref = O.depth_to_space(ref, r)
    return dict(x=x, w=w, b=b, dtype=dtype, act=act, alpha=alpha, skip1=s1, beta1=beta1, skip2=s2, beta2=beta2, clip01=clip01, d2s=r), ref, route


@pytest.mark.parametrize("exact", [False, True], ids=["seeded", "exact"])
@pytest.mark.parametrize("case", ROUTES, ids=[c[0] for c in ROUTES])
def test_conv_route(route_ctx, case, exact):
    kw, ref, route = _case(case, exact)
    got, routes, untouched = run_conv(route_ctx, **kw)
    assert routes == [route], (routes, route)
    assert untouched, "the conv stored outside its output tensor"
    assert got.shape == ref.shape
    if exact:
        want = O.round_bf16(ref) if kw["dtype"] == "bf16" else ref
        bad = got != want
        assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), float(np.abs(got - want).max()))
    elif kw["dtype"] == "f32":
        assert rel_l2(got, ref) <= 1e-5
    else:
        assert_bf16_close(got, ref)


# ------------------------------------------------------------------------------------------------ the fused 9x9 + 1x1 head
@pytest.mark.parametrize("exact", [False, True], ids=["seeded", "exact"])
@pytest.mark.parametrize("fused", [True, False], ids=["pw2", "alone"])
def test_srcnn_head_routes(route_ctx, fused, exact):
    """SRCNN's 9x9 RGB head with its 1x1 successor in the epilogue (only sr_forward builds it) and alone, fp32."""
    ctx = route_ctx
    m = Model("srcnn", compute_dtype="f32", ctx=ctx)
    rng = np.random.default_rng(23 + exact)
    if exact:
        w = {k: (rng.integers(-1, 2, np.shape(kb[0])).astype(np.float32), rng.integers(-2, 3, np.shape(kb[1])).astype(np.float32))
             for k, kb in init_weights(m.layer_shapes(), seed=3).items()}
        x = rng.integers(0, 3, (2, 29, 35, 3)).astype(np.float32)
    else:
        w = init_weights(m.layer_shapes(), seed=3)
        x = rng.uniform(0, 1, (2, 29, 35, 3)).astype(np.float32)
    ctx.set_fused(ctx.FUSED_ALL if fused else ctx.FUSED_ALL & ~ctx.FUSED_SRCNN_1X1, 0)
    m.set_weights(w)
    xd = ctx.to_device(x, torch.float32)
    ctx.conv_routes(True)
    got = m.forward(xd).float().cpu().numpy()
    routes = ctx.conv_routes(False)
    head = ["thin<f32,k9,nt3,nv3>/pw2"] if fused else ["thin<f32,k9,nt1,nv3>", "wide<f32,k1,kg4,nt1>/mt1"]
    assert routes == head + ["few<f32,k5>/lds"], routes
    ref = M.srcnn_forward(x, w, dtype=np.float64)
    if exact:
        assert np.array_equal(got, ref), float(np.abs(got - ref).max())
    else:
        assert rel_l2(got, ref) <= 1e-5
