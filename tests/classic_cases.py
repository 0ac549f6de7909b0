"""Case tables and designed images for the classical kernels' arguments off the notebook's defaults (tests/test_classic_args_gpu.py runs
them on the device; tests/test_classic_args_cpu.py proves on the fp64 restatements that each table does what it claims).

NL-means.  nlm_kernel keeps the weight exp(-dist) of a (pixel, shift) pair where dist = D / 65025 / (h^2 patch^2) <= 5.  The notebook's
h = 1.15 sigma has sigma on the 0..255 scale and D / 65025 on the 0..1 scale, so at the default h_scale no weight is ever cut and every weight
is ~1: a box mean.  The cases here supply sigma themselves (sr_nl_means reads it from a device tensor), one value per image of a batch, and run
each (patch, distance) at the default h_scale and at two selective ones, on images whose structure decides which pairs are cut: two gray
levels in irregular blocks, a slow sinusoid and Gaussian noise of 6.

A shift of zero has D = 0 and is never cut; with distance 0 it is the only shift, so those cases have no selective regime by construction:
their output is x / 255 rounded to float32 at every h_scale, which is what they assert."""
import functools

import numpy as np

import classic_ref as CR

NLM_TILE = 32                       # csrc/classic.hip
H_DEFAULT = 1.15
H_SCALES = (H_DEFAULT, 0.02, 0.008)
SIGMAS = (4.0, 5.0)                 # one per image of a batch of two, 0..255 units (estimate_sigma gives about 6 on these images)
PATCH_DISTANCE = ((5, 6), (1, 0), (1, 12), (9, 12), (9, 0), (3, 1), (7, 2))

# fp32 steps: |got - ref| <= STEP * max(|ref|, FLOOR).  The device's cutoff decisions and summation order are the restatement's (an exact
# int32 SSD, the same two fp64 divisions, the same shift order); exp and a possible fma differ by ~1e-13 relative, far below the one
# rounding to float32 that ends the kernel, which is at most half a step.
STEP = 2.0 ** -23
FLOOR = 2.0 ** -24


def structured(h, w, seed, levels=(70, 190), amp=18.0, noise=6.0):
    """uint8 [h, w]: two gray levels in blocks of irregular widths (3..9 pixels), a slow diagonal sinusoid, Gaussian noise."""
    rng = np.random.default_rng(seed)

    def cells(n):
        edges = np.cumsum(rng.integers(3, 10, n + 1))
        return np.searchsorted(edges, np.arange(n), side="right")

    cy, cx = cells(h), cells(w)
    pick = rng.integers(0, 2, (cy.max() + 1, cx.max() + 1))
    pick[::2, ::2] = 0                                            # both levels present whatever the draw
    pick[1::2, ::2] = 1
    lev = np.asarray(levels, np.float64)[pick[cy[:, None], cx[None, :]]]
    y, x = np.mgrid[0:h, 0:w]
    wave = amp * np.sin(2 * np.pi * (y / 37.0 + x / 53.0) + rng.uniform(0, 2 * np.pi))
    return np.clip(lev + wave + rng.normal(0, noise, (h, w)), 0, 255).astype(np.uint8)


def structured_small(h, w, seed):
    """The same for images of a few pixels: blocks of 3 x 2 from a seeded origin, so that a 5 x 7, 1 x 9 or 40 x 1 image still has both levels."""
    rng = np.random.default_rng(seed)
    oy, ox = int(rng.integers(0, 3)), int(rng.integers(0, 2))
    y, x = np.mgrid[0:h, 0:w]
    lev = np.where(((y + oy) // 3 + (x + ox) // 2) % 2 == 0, 70.0, 190.0)
    return np.clip(lev + rng.normal(0, 6.0, (h, w)), 0, 255).astype(np.uint8)


# (h, w) -> what the shape is for
GEOMETRY = {
    (33, 65): "remainders both ways, 2 x 3 tiles",
    (32, 32): "one exact tile",
    (5, 7): "with distance 12 the halo is several image sizes: the reflect index bounces more than once",
    (1, 9): "n == 1 along y",
    (40, 1): "n == 1 along x, two tiles",
    (40, 3): "narrower than any halo, two tiles",
}


# The selective h_scales: 0.02 and 0.008 unless listed.  On these two-level images the share of pairs cut falls from ~1 to 0 as h = h_scale * sigma
# goes from 0.09 to 0.25 (a patch that straddles a level edge has a mean squared difference of the straddling share of its pixels times
# (120 / 255)^2 = 0.22, against 5 h^2).  A 9 x 9 patch straddles an edge at nearly every shift, and so does any patch on an image of a few pixels,
# so those run inside that band, at values picked on the restatement alone until it cuts between 5 % and 95 % of the pairs for both sigmas
# (test_classic_args_cpu.py asserts that for every selective case of the table).
SELECTIVE = {(9, 12): (0.03, 0.025)}
SMALL_SELECTIVE = {(5, 7): 0.03, (1, 9): 0.03, (40, 1): 0.025, (40, 3): 0.03}


def _nlm_cases():
    cases = []
    for p, d in PATCH_DISTANCE:                                   # every argument pair in every regime at the shape with remainders
        for hs in (H_DEFAULT,) + SELECTIVE.get((p, d), H_SCALES[1:]):
            cases.append((33, 65, p, d, hs))
    for hs in H_SCALES:
        cases.append((32, 32, 5, 6, hs))
    for hw, sel in SMALL_SELECTIVE.items():
        for p, d in ((1, 12), (9, 12), (5, 6), (3, 1)):
            for hs in (H_DEFAULT, sel):
                cases.append(hw + (p, d, hs))
    return cases


NLM_CASES = _nlm_cases()


def nlm_id(case):
    h, w, p, d, hs = case
    return f"{h}x{w}-p{p}-d{d}-h{hs:g}"


def nlm_selective(case):
    """Whether the case is one whose h_scale must cut between 5 % and 95 % of the (pixel, shift) pairs of each image."""
    return case[4] != H_DEFAULT and case[3] > 0


@functools.lru_cache(maxsize=None)
def nlm_images(h, w):
    """The batch of two uint8 images of one shape (shared by every case of that shape; never written to)."""
    make = structured if min(h, w) >= 32 else structured_small
    x = np.stack([make(h, w, seed=1000 * h + w + i) for i in range(len(SIGMAS))])
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def nlm_reference(case):
    """-> (fp64 reference [B, h, w], cut share per image) of one case, computed once."""
    h, w, p, d, hs = case
    refs, cuts = [], []
    for img, sigma in zip(nlm_images(h, w), SIGMAS):
        dist, vals = CR.nl_means_dist(img, hs * sigma, p, d)
        keep = dist <= 5.0
        refs.append(CR.nl_means_of_dist(dist, vals, keep))
        cuts.append(1.0 - float(np.mean(keep)))
    ref = np.stack(refs)
    ref.setflags(write=False)
    return ref, tuple(cuts)


def steps(got, ref):
    """|got - ref| in units of the tolerance's fp32 step, per element."""
    return np.abs(got.astype(np.float64) - ref) / (STEP * np.maximum(np.abs(ref), FLOOR))


# ------------------------------------------------------------------------------------------------ the cutoff itself
# patch 1, h_scale 1, sigma^2 == 0.2 in fp64: a pixel pair that differs by 255 has D = 65025 and dist = 1 / 0.2 == 5.0 exactly, the last value
# `<=` keeps.  The second and third image of the batch get the neighbouring sigmas: one ulp-scale step down cuts those pairs (dist > 5), one up keeps
# them with room (dist < 5).
CUTOFF_SIGMA = float.fromhex("0x1.c9f25c5bfedd9p-2")
CUTOFF_SIGMAS = (CUTOFF_SIGMA, CUTOFF_SIGMA * (1 - 1e-12), CUTOFF_SIGMA * (1 + 1e-12))
CUTOFF_PATCH, CUTOFF_DISTANCE, CUTOFF_H_SCALE = 1, 2, 1.0


@functools.lru_cache(maxsize=None)
def cutoff_image(h=33, w=40):
    """0 / 255 checkerboard with a few isolated flipped pixels (which break the board's symmetry between a shift and its mirror)."""
    y, x = np.mgrid[0:h, 0:w]
    img = np.where((y + x) % 2 == 0, 0, 255).astype(np.uint8)
    rng = np.random.default_rng(5)
    for _ in range(12):
        r, c = rng.integers(0, h), rng.integers(0, w)
        img[r, c] = 255 - img[r, c]
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------ refusals of sr_nl_means
# (name, patch, distance, B, sigma given); everything else valid.  Nothing may be launched and the output buffer stays untouched.
NLM_REFUSALS = (
    ("patch0", 0, 6, 2, True), ("patch4", 4, 6, 2, True), ("patch11", 11, 6, 2, True), ("patch-1", -1, 6, 2, True),
    ("distance-1", 5, -1, 2, True), ("distance13", 5, 13, 2, True), ("B0", 5, 6, 0, True), ("null_sigma", 5, 6, 2, False),
)

# ------------------------------------------------------------------------------------------------ hf_radius_frac
HF_FRACS = (-0.5, 0.0, 0.25, 0.6, 0.999, 1.0, 1.5)
HF_SHAPES = ((20, 23), (48, 48))
HF_MASK_SIZES_20x23 = (460, 459, 415, 219, 2, 0, 0)          # the last two equal by design: f >= 1 empties the mask


@functools.lru_cache(maxsize=None)
def hf_pair(H, W, C):
    """uint8 (hr, sr) of [H, W] or [H, W, 3]: structured HR, SR its 3 x 3 box blur plus noise (so the two spectra differ most at high radius)."""
    rng = np.random.default_rng(H * 31 + W * 7 + C)
    hr = np.stack([structured(H, W, seed=H + W + 10 * c, noise=5.0).astype(np.float64) for c in range(3)], axis=-1)
    pad = np.pad(hr, ((1, 1), (1, 1), (0, 0)), mode="edge")
    blur = sum(pad[i:i + H, j:j + W] for i in range(3) for j in range(3)) / 9.0
    sr = np.clip(blur + rng.normal(0, 8, hr.shape), 0, 255).astype(np.uint8)
    hr = hr.astype(np.uint8)
    out = (hr, sr) if C == 3 else (np.ascontiguousarray(hr[..., 1]), np.ascontiguousarray(sr[..., 1]))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ up-scalers at scale 1
# (H, W, h, w): equality on x, on y, on both; one row added to 8 x 7; the 1 x 1 image (whose noise estimate is NaN)
UNIT_SCALE_SHAPES = ((24, 30, 24, 15), (24, 30, 12, 30), (24, 30, 24, 30), (9, 7, 8, 7), (2, 2, 1, 1))


@functools.lru_cache(maxsize=None)
def unit_scale_pair(H, W, h, w):
    """uint8 (hr [H, W], lr [h, w]), independent draws of the same kind of image."""
    hr, lr = structured_small(H, W, seed=H * W + h), structured_small(h, w, seed=h * w + W + 1)
    if min(H, W) >= 9:
        hr = structured(H, W, seed=H * W + h)
    if min(h, w) >= 9:
        lr = structured(h, w, seed=h * w + W + 1)
    hr.setflags(write=False)
    lr.setflags(write=False)
    return hr, lr
