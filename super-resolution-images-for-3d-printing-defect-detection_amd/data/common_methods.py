"""The dataset's synthesis step (reference: data/common_methods.py, called once per extracted video frame by
data/preprocessing_functions.ipynb): degrade_image turns an HR frame into its LR partner by a Gaussian blur (70 % of frames), a horizontal
motion blur (30 %), a cv2.resize with a randomly chosen interpolation, Gaussian noise (70 %) and a JPEG round trip (70 %).  Every pixel
stage runs on the MI355X (csrc/degrade.hip: sr_degrade_gauss / _motion / _noise / _jpeg, and sr_resize); cv2 is not needed.  The contracts
of the 8-bit stages are stated in include/sr355.h.

The random decisions are made explicit: draw_degradation makes the reference's draws, in the reference's order, from the global
np.random state (or a RandomState handed in) and returns them as a record, without touching a device.  After np.random.seed(s),
degrade_image therefore takes the decisions the reference takes after the same seed, noise field included.  degrade_batch does a whole
stack in one pass with decisions from a seeded np.random.Generator and the noise from the kernel's counter-based Philox generator.

The crop that precedes it in the notebook's loop, smart_square_crop, runs on the device for a stack of frames: square_crop_batch (csrc/crop.hip:
Otsu threshold, hole filling and connected components in place of contour tracing, sr_object_boxes / sr_square_crop), and synthesize_pairs is
the loop's body -- crop, then degrade -- with nothing returning to the host in between.

Out of scope: smart_square_crop itself (Otsu threshold and contour tracing: host work on one image at a time) raises NotImplementedError;
square_crop_batch is its batched form.  Importing this module and draw_degradation need no GPU."""
import numpy as np

# cv2.INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4, in the order the reference hands them to np.random.choice
INTERP_CODES = (1, 2, 3, 4)
INTERP_NAMES = {1: "INTER_LINEAR", 2: "INTER_CUBIC", 3: "INTER_AREA", 4: "INTER_LANCZOS4"}
MIN_SIDE = 16


def _context():
    from sr355 import Context                  # loaded on first use: the drawing runs without a GPU
    return Context.get()


def smart_square_crop(img):
    raise NotImplementedError("smart_square_crop: Otsu thresholding and contour tracing are host work on one image at a time and are outside this "
                              "port's scope (crop the frames with the reference's own function before handing them to degrade_image, or hand a stack of "
                              "frames [B, H, W, 3] to square_crop_batch, which computes the same crop on the device)")


def lr_size(shape, scale_factor):
    """(w, h) of the LR image as the reference computes it: (int(w * scale_factor), int(h * scale_factor))."""
    h, w = int(shape[0]), int(shape[1])
    return int(w * scale_factor), int(h * scale_factor)


def draw_degradation(shape, scale_factor=0.5, rng=None, draw_noise=True):
    """The reference's random draws for one frame of `shape` (H, W, 3), in its order, from `rng` (the global np.random state when None, or a
    np.random.RandomState): rand; if < 0.7 choice([3, 5, 7]), uniform(0.8, 2.0); rand; if < 0.3 choice([5, 7, 9]); choice of the four
    interpolation codes; rand; if < 0.7 uniform(2, 10), normal(0, std, lr shape); rand; if < 0.7 randint(20, 60).
    -> dict: gauss_ksize (0: off), gauss_sigma (None: off), motion_size (0: off), interp_code, interp_name, lr_size (w, h), noise_std
    (None: off), noise (float32 [h, w, 3], or None), jpeg_quality (0: off).  draw_noise=False skips the normal() draw (the stream then
    differs from the reference's after that point): for callers that generate the field elsewhere."""
    r = np.random if rng is None else rng
    rec = {"gauss_ksize": 0, "gauss_sigma": None, "motion_size": 0, "noise_std": None, "noise": None, "jpeg_quality": 0}
    if r.rand() < 0.7:
        rec["gauss_ksize"] = int(r.choice([3, 5, 7]))
        rec["gauss_sigma"] = float(r.uniform(0.8, 2.0))
    if r.rand() < 0.3:
        rec["motion_size"] = int(r.choice([5, 7, 9]))
    rec["interp_code"] = int(r.choice(list(INTERP_CODES)))
    rec["interp_name"] = INTERP_NAMES[rec["interp_code"]]
    w, h = lr_size(shape, scale_factor)
    rec["lr_size"] = (w, h)
    if r.rand() < 0.7:
        rec["noise_std"] = float(r.uniform(2, 10))
        if draw_noise:
            rec["noise"] = r.normal(0, rec["noise_std"], (h, w) + tuple(shape[2:])).astype(np.float32)
    if r.rand() < 0.7:
        rec["jpeg_quality"] = int(r.randint(20, 60))
    return rec


def draw_degradation_generator(gen, shape, scale_factor=0.5):
    """The same decisions in the same order from a np.random.Generator (degrade_batch's source); the noise field is left to the kernel."""
    rec = {"gauss_ksize": 0, "gauss_sigma": None, "motion_size": 0, "noise_std": None, "noise": None, "jpeg_quality": 0}
    if gen.random() < 0.7:
        rec["gauss_ksize"] = int(gen.choice([3, 5, 7]))
        rec["gauss_sigma"] = float(gen.uniform(0.8, 2.0))
    if gen.random() < 0.3:
        rec["motion_size"] = int(gen.choice([5, 7, 9]))
    rec["interp_code"] = int(gen.choice(list(INTERP_CODES)))
    rec["interp_name"] = INTERP_NAMES[rec["interp_code"]]
    rec["lr_size"] = lr_size(shape, scale_factor)
    if gen.random() < 0.7:
        rec["noise_std"] = float(gen.uniform(2, 10))
    if gen.random() < 0.7:
        rec["jpeg_quality"] = int(gen.integers(20, 60))
    return rec


def _check_frames(a, ndim, who):
    import torch
    is_t = isinstance(a, torch.Tensor)
    dtype_ok = a.dtype == (torch.uint8 if is_t else np.uint8)
    if not is_t:
        a = np.asarray(a)
        dtype_ok = a.dtype == np.uint8
    if not dtype_ok:
        raise NotImplementedError(f"{who}: {a.dtype} images are not offered (the dataset's frames are 8-bit BGR)")
    if a.ndim != ndim or a.shape[-1] != 3:
        raise ValueError(f"{who}: expected uint8 BGR {'[B, H, W, 3]' if ndim == 4 else '[H, W, 3]'}, got shape {tuple(a.shape)}")
    H, W = int(a.shape[-3]), int(a.shape[-2])
    if H < MIN_SIDE or W < MIN_SIDE:
        raise ValueError(f"{who}: frames of {H} x {W} are below the device stages' minimum of {MIN_SIDE} pixels a side")
    return a, is_t


def _check_stack(a, who):
    """_check_frames for the crop's input: any frame of at least 2 x 2 pixels, and at least one of them.  Touches no device."""
    import torch
    is_t = isinstance(a, torch.Tensor)
    if not is_t:
        a = np.asarray(a)
    if a.dtype != (torch.uint8 if is_t else np.uint8):
        raise NotImplementedError(f"{who}: {a.dtype} images are not offered (the dataset's frames are 8-bit BGR)")
    if a.ndim != 4 or a.shape[-1] != 3:
        raise ValueError(f"{who}: expected uint8 BGR [B, H, W, 3], got shape {tuple(a.shape)}")
    if a.shape[0] < 1:
        raise ValueError(f"{who}: empty batch")
    if min(int(a.shape[1]), int(a.shape[2])) < 2:
        raise ValueError(f"{who}: frames of {int(a.shape[1])} x {int(a.shape[2])} are below the crop's minimum of 2 pixels a side")
    return a, is_t


def _run_stages(ctx, x, recs, field=None, seed=0):
    """x [B,H,W,3] uint8 on the device through the stages the records switch on -> LR batch on the device."""
    params = ctx.to_device(ctx.degrade_params(recs))
    if any(r["gauss_ksize"] for r in recs):
        x = ctx.degrade_gauss(x, params, check=False)
    if any(r["motion_size"] for r in recs):
        x = ctx.degrade_motion(x, params, check=False)
    w, h = recs[0]["lr_size"]
    codes = sorted({r["interp_code"] for r in recs})
    if len(codes) == 1:
        lr = ctx.resize(x, h, w, codes[0])
    else:                                            # one resize per interpolation code present, scattered back into batch order
        import torch
        lr = ctx.empty((x.shape[0], h, w, 3), torch.uint8)
        for code in codes:
            idx = torch.as_tensor([i for i, r in enumerate(recs) if r["interp_code"] == code], device=ctx.torch_device)
            lr[idx] = ctx.resize(x[idx].contiguous(), h, w, code)
    if any(r["noise_std"] is not None for r in recs):
        lr = ctx.degrade_noise(lr, params, field=field, seed=seed, check=False)
    if any(r["jpeg_quality"] for r in recs):
        lr = ctx.degrade_jpeg(lr, params, check=False)
    ctx.degrade_status()
    return lr


def degrade_image(hr_image, scale_factor=0.5):
    """The reference's degrade_image: hr_image uint8 BGR [H, W, 3] (NumPy array or device tensor) -> (lr_image, interp_name), lr_image of
    the input's kind.  Draws from the global np.random state exactly as the reference does."""
    a, is_t = _check_frames(hr_image, 3, "degrade_image")
    rec = draw_degradation(tuple(a.shape), scale_factor)
    if min(rec["lr_size"]) < MIN_SIDE:
        raise ValueError(f"degrade_image: the LR frame {rec['lr_size'][1]} x {rec['lr_size'][0]} is below the device stages' minimum of {MIN_SIDE} pixels a side")
    ctx = _context()
    x = (a.contiguous() if is_t else ctx.to_device(np.ascontiguousarray(a)))[None]
    field = None if rec["noise"] is None else ctx.to_device(rec["noise"][None])
    lr = _run_stages(ctx, x, [rec], field=field)[0]
    return (lr if is_t else lr.cpu().numpy()), rec["interp_name"]


def degrade_batch(hr_batch, scale_factor=0.5, seed=0):
    """degrade_image's stages for a stack [B, H, W, 3] uint8 BGR (NumPy array or device tensor) in one pass: decisions per frame from
    np.random.default_rng(seed) in the reference's order, noise from the kernel's Philox stream keyed by `seed`.
    -> (LR batch on the device, uint8 [B, h, w, 3]; the list of interpolation names, the entries interpolation_map.pkl wants)."""
    a, is_t = _check_frames(hr_batch, 4, "degrade_batch")
    gen = np.random.default_rng(seed)
    recs = [draw_degradation_generator(gen, tuple(a.shape[1:]), scale_factor) for _ in range(int(a.shape[0]))]
    if not recs:
        raise ValueError("degrade_batch: empty batch")
    if min(recs[0]["lr_size"]) < MIN_SIDE:
        raise ValueError(f"degrade_batch: the LR frames {recs[0]['lr_size'][1]} x {recs[0]['lr_size'][0]} are below the device stages' minimum of {MIN_SIDE} pixels a side")
    ctx = _context()
    x = a.contiguous() if is_t else ctx.to_device(np.ascontiguousarray(a))
    return _run_stages(ctx, x, recs, seed=int(seed)), [r["interp_name"] for r in recs]


def square_crop_batch(frames):
    """The reference's smart_square_crop for a stack: frames uint8 BGR [B, H, W, 3] (NumPy array or device tensor) -> (crops uint8
    [B, S, S, 3] on the device, S = min(H, W); boxes as a NumPy int32 array [B, 8]: found, x, y, w, h of the largest contour's bounding
    rectangle, left, top of the crop, Otsu's threshold).  The frames themselves never come back to the host."""
    a, is_t = _check_stack(frames, "square_crop_batch")
    ctx = _context()
    x = a.contiguous() if is_t else ctx.to_device(np.ascontiguousarray(a))
    boxes = ctx.object_boxes(x)
    return ctx.square_crop(x, boxes, check=False), boxes.cpu().numpy()


def synthesize_pairs(frames, scale_factor=0.5, seed=0):
    """The notebook's loop body for a stack of decoded frames: hr = smart_square_crop(frame), lr = degrade_image(hr), as square_crop_batch
    followed by degrade_batch's stages, the crops staying on the device.  -> (hr crops uint8 [B, S, S, 3] and lr uint8 [B, h, w, 3] on the
    device, the list of interpolation names)."""
    a, is_t = _check_stack(frames, "synthesize_pairs")
    S = min(int(a.shape[1]), int(a.shape[2]))
    if min(S, *lr_size((S, S), scale_factor)) < MIN_SIDE:
        raise ValueError(f"synthesize_pairs: crops of {S} x {S} at scale {scale_factor} are below the device stages' minimum of {MIN_SIDE} pixels a side")
    ctx = _context()
    x = a.contiguous() if is_t else ctx.to_device(np.ascontiguousarray(a))
    hr = ctx.square_crop(x)
    lr, names = degrade_batch(hr, scale_factor, seed)
    return hr, lr, names
