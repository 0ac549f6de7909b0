"""The square crop on the device (sr_object_boxes / sr_square_crop, Context.object_boxes / square_crop, data.common_methods.square_crop_batch /
synthesize_pairs) against the NumPy restatement of tests/crop_ref.py, stage by stage through the raw outputs.  Everything compared is an
integer or a byte: exact equality throughout.  The frames are 97 x 150, 150 x 97 and 101 x 101: three or four 32-pixel labelling tiles and
a remainder each way, B = 3 (a design, its mirror image and its upside-down image, so that no result can lean on a symmetry)."""
import numpy as np
import pytest
import torch

import crop_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(97, 150), (150, 97), (101, 101)]


def random_mask(density, seed):
    return lambda H, W: np.random.default_rng(seed).random((H, W)) < density


def isolated_pixels(H, W):
    m = np.zeros((H, W), bool)
    m[5, 7] = m[H // 2, W - 1] = m[H - 1, 3] = m[H - 3, W // 2] = m[33, 31] = True
    return m


def two_equal_squares(H, W):
    m = np.zeros((H, W), bool)
    m[4:40, 6:42] = True                              # both straddle a tile seam
    m[H - 45:H - 9, W - 50:W - 14] = True
    return m


DESIGNS = {
    "random 0.3": random_mask(0.3, 1), "random 0.5": random_mask(0.5, 2), "random 0.7": random_mask(0.7, 3),
    "checkerboard": R.checkerboard, "spiral": R.spiral, "serpentine": R.serpentine,
    "nested rings": lambda H, W: R.nested_rings(H, W, n=6, width=3, gap=4),
    "all foreground": lambda H, W: np.ones((H, W), bool),
    "isolated pixels": isolated_pixels, "two equal squares": two_equal_squares,
    "black frame": lambda H, W: np.zeros((H, W), bool),
}

_cache = {}


def design_frames(name, shape):
    m = DESIGNS[name](*shape)
    return R.frames_from_mask(np.stack([m, m[:, ::-1], m[::-1]]))


def reference(key, frames_fn):
    """The restatement's outputs for a batch, computed once per module run and shared."""
    if key not in _cache:
        frames = frames_fn()
        _cache[key] = (frames, R.object_boxes(frames))
    return _cache[key]


def run(ctx, frames):
    boxes, raw = ctx.object_boxes(ctx.to_device(frames), raw=True)
    return boxes.cpu().numpy(), {k: v.cpu().numpy() for k, v in raw.items()}


def assert_stages_equal(got_boxes, got_raw, ref, what):
    assert np.array_equal(got_raw["gray"], ref["gray"]), what
    assert np.array_equal(got_boxes[:, 7], ref["boxes"][:, 7]), (what, got_boxes[:, 7], ref["boxes"][:, 7])
    assert np.array_equal(got_raw["mask"], ref["mask"]), what
    assert np.array_equal(got_raw["labels"], ref["labels"]), what
    assert np.array_equal(got_boxes, ref["boxes"]), (what, got_boxes, ref["boxes"])


# ---------------------------------------------------------------------------------------------- gray, Otsu, mask on natural-looking inputs
def photo_like(shape, seed):
    H, W = shape
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    blob = ((yy - 0.6 * H) ** 2 / (0.25 * H) ** 2 + (xx - 0.3 * W) ** 2 / (0.2 * W) ** 2) < 1
    bimodal = np.clip(np.where(blob, 170, 60)[..., None] + rng.normal(0, 25, (H, W, 3)), 0, 255).astype(np.uint8)
    return np.stack([noise, bimodal, np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 200, np.uint8)])


@pytest.mark.parametrize("shape", SHAPES)
def test_gray_otsu_mask_labels_on_noise_bimodal_and_constant_frames(ctx, shape):
    frames, ref = reference(("photo", shape), lambda: photo_like(shape, 5))
    boxes, raw = run(ctx, frames)
    assert_stages_equal(boxes, raw, ref, shape)
    H, W = shape
    assert ref["boxes"][2].tolist()[:5] == [0, 0, 0, 0, 0] and ref["boxes"][2, 7] == 0          # black: no contour, the centre crop
    assert ref["boxes"][3].tolist()[:5] == [1, 0, 0, W, H] and ref["boxes"][3, 7] == 0          # constant 200: threshold 0, all foreground
    assert 60 < ref["boxes"][1, 7] < 170 and ref["boxes"][1, 0] == 1                            # bimodal: between the two modes


# ---------------------------------------------------------------------------------------------- labels and boxes on driven masks
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", sorted(DESIGNS))
def test_labels_boxes_and_crop_on_designed_masks(ctx, name, shape):
    frames, ref = reference((name, shape), lambda: design_frames(name, shape))
    boxes, raw = run(ctx, frames)
    assert_stages_equal(boxes, raw, ref, (name, shape))
    crops = ctx.square_crop(ctx.to_device(frames)).cpu().numpy()
    assert np.array_equal(crops, R.square_crop(frames, ref["boxes"])), (name, shape)
    if shape[0] == shape[1]:
        assert np.array_equal(crops, frames)


def test_tie_cases_are_what_the_contract_says():
    shape = SHAPES[0]
    _, ref = reference(("isolated pixels", shape), lambda: design_frames("isolated pixels", shape))
    H, W = shape
    assert ref["boxes"][0].tolist()[:5] == [1, 3, H - 1, 1, 1]                   # the last isolated pixel in raster order
    _, ref = reference(("two equal squares", shape), lambda: design_frames("two equal squares", shape))
    assert ref["boxes"][0].tolist()[:5] == [1, W - 50, H - 45, 36, 36]           # equal areas: the later square
    _, ref = reference(("black frame", shape), lambda: design_frames("black frame", shape))
    assert ref["boxes"][0].tolist() == [0, 0, 0, 0, 0, (W - H) // 2, 0, 0]


# ---------------------------------------------------------------------------------------------- the gather alone
def test_square_crop_with_a_table_of_the_callers_at_every_copy_width(ctx):
    rng = np.random.default_rng(9)
    frames = rng.integers(0, 256, (3, 64, 128, 3), dtype=np.uint8)
    for lefts in ((16, 48, 64), (4, 20, 8), (3, 63, 1)):                          # 16-, 4- and 1-byte copies (row pitches 384 and 192 bytes)
        boxes = np.zeros((3, 8), np.int32)
        boxes[:, 5] = lefts
        got = ctx.square_crop(ctx.to_device(frames), boxes).cpu().numpy()
        assert np.array_equal(got, R.square_crop(frames, boxes)), lefts
    tall = np.ascontiguousarray(frames.transpose(0, 2, 1, 3))
    boxes = np.zeros((3, 8), np.int32)
    boxes[:, 6] = (0, 64, 37)
    assert np.array_equal(ctx.square_crop(ctx.to_device(tall), boxes).cpu().numpy(), R.square_crop(tall, boxes))
    boxes[1, 6] = 65                                                              # one row below the last square that fits
    with pytest.raises(ValueError, match="row 1"):
        ctx.square_crop(ctx.to_device(tall), boxes)
    clamped = ctx.square_crop(ctx.to_device(tall), boxes, check=False).cpu().numpy()
    boxes[1, 6] = 64
    assert np.array_equal(clamped, R.square_crop(tall, boxes))


def test_odd_sized_frames_take_the_unaligned_paths(ctx):
    """33 x 35 x 3 bytes per frame is odd: frames 1 and 2 of the batch start off every alignment the vector paths want."""
    rng = np.random.default_rng(10)
    frames = rng.integers(0, 256, (3, 33, 35, 3), dtype=np.uint8)
    frames[1] = R.frames_from_mask(R.nested_rings(33, 35))[..., :]
    ref = R.object_boxes(frames)
    boxes, raw = run(ctx, frames)
    assert_stages_equal(boxes, raw, ref, "33 x 35")
    assert np.array_equal(ctx.square_crop(ctx.to_device(frames)).cpu().numpy(), R.square_crop(frames, ref["boxes"]))
    tiny = rng.integers(0, 256, (2, 2, 3, 3), dtype=np.uint8)                     # the smallest frame the entry takes
    b2, r2 = run(ctx, tiny)
    assert_stages_equal(b2, r2, R.object_boxes(tiny), "2 x 3")
    with pytest.raises(ValueError):
        ctx.object_boxes(ctx.to_device(np.zeros((1, 1, 5, 3), np.uint8)))


# ---------------------------------------------------------------------------------------------- batch independence
def test_a_mixed_batch_equals_its_frames_run_one_at_a_time(ctx):
    shape = SHAPES[0]
    names = ["random 0.5", "spiral", "black frame", "nested rings", "all foreground", "isolated pixels", "two equal squares", "checkerboard"]
    frames = np.concatenate([design_frames(n, shape)[:1] for n in names] + [photo_like(shape, 6)])
    x = ctx.to_device(frames)
    boxes, raw = ctx.object_boxes(x, raw=True)
    crops = ctx.square_crop(x, boxes)
    for k in range(frames.shape[0]):
        b1, r1 = ctx.object_boxes(x[k:k + 1].contiguous(), raw=True)
        assert torch.equal(b1[0], boxes[k]), k
        for key in ("gray", "mask", "labels"):
            assert torch.equal(r1[key][0], raw[key][k]), (k, key)
        assert torch.equal(ctx.square_crop(x[k:k + 1].contiguous())[0], crops[k]), k
    again = ctx.object_boxes(x)                                                   # and the same bits on a second run
    assert torch.equal(again, boxes)


# ---------------------------------------------------------------------------------------------- the data module
def test_square_crop_batch_and_synthesize_pairs(ctx):
    from data import common_methods as M
    shape = (97, 150)
    frames = np.concatenate([photo_like(shape, 7)[:2], design_frames("two equal squares", shape)[:1]])
    ref = R.object_boxes(frames)
    crops, boxes = M.square_crop_batch(frames)
    assert isinstance(boxes, np.ndarray) and boxes.shape == (3, 8) and np.array_equal(boxes, ref["boxes"])
    assert crops.device == ctx.torch_device and crops.dtype == torch.uint8 and tuple(crops.shape) == (3, 97, 97, 3)
    assert np.array_equal(crops.cpu().numpy(), R.square_crop(frames, ref["boxes"]))
    x = ctx.to_device(frames)                                                     # device tensor in, device tensor out, the same bytes
    crops_t, boxes_t = M.square_crop_batch(x)
    assert crops_t.device == x.device and torch.equal(crops_t, crops) and np.array_equal(boxes_t, boxes)
    for seed in (0, 3):
        hr, lr, names = M.synthesize_pairs(x, 0.5, seed)
        want_lr, want_names = M.degrade_batch(crops, 0.5, seed)
        assert hr.device == x.device and lr.device == x.device
        assert torch.equal(hr, crops) and torch.equal(lr, want_lr) and names == want_names
        assert tuple(lr.shape) == (3, 48, 48, 3)
    hr_n, lr_n, _ = M.synthesize_pairs(frames, 0.5, 3)                            # a NumPy stack gives the same bytes
    assert torch.equal(hr_n, hr) and torch.equal(lr_n, lr)
