"""The four cv2.resize up-scalers of the reference's classical baseline on MI355X (reference:
classic_super_resolution_algorithms/classic_algorithms.py:7-21).  Each is `cv2.resize(lr_img, target_shape, interpolation=...)`:
target_shape is (width, height) as in OpenCV; uint8 input -> uint8 (OpenCV's fixed-point path), float input -> float32, no
clipping.  Bicubic runs the tiled INTER_CUBIC kernel (BASELINE cfg0 and the SRCNN pre-upscale), the others the tap-table
kernel behind sr_resize.

The module's other four algorithms (classic_algorithms.py:23-108) run on the device too (csrc/classic.hip), for the 2-D uint8
grayscale images the reference's notebook hands them (cv2.cvtColor(..., COLOR_RGB2GRAY)); any other rank or dtype raises
NotImplementedError.  The first argument is the HR image, used for its shape only -- except by back_projection, which starts its
estimate from it, as the reference does.
  back_projection(hr, lr, iterations=10) -> uint8: hr = float32(hr); repeat: hr += resize(float32(lr) - resize(hr, (w, h),
      INTER_LINEAR), (W, H), INTER_LINEAR); clip(hr, 0, 255) truncated.
  non_local_means(hr, lr) -> float64: sigma = median(|dd band of db2(lr)| != 0) / 0.6744897501960817 in 0..255 units;
      denoise_nl_means(lr / 255, h=1.15 sigma, patch 5, distance 6, fast mode) computed as
      y[p] = sum_t w P[p+t] / sum_t w, w = exp(-D / (h^2 25)) when that is <= 5 (D the 5x5 patch SSD); then INTER_LANCZOS4 to (W, H).
      A detail-free image (sigma 0 or NaN) raises ValueError: the reference divides by zero there.
  edge_guided_interpolation(hr, lr) -> uint8: clip(float32(resize_u8(lr, INTER_LINEAR)) + 0.3 float32(resize(hypot(Sobel_x,
      Sobel_y), INTER_LINEAR)), 0, 255) truncated (Sobel ksize 3, BORDER_REFLECT_101).
  frequency_extrapolation(hr, lr) -> float64: |ifft2(ifftshift(zero-pad(fftshift(fft2(lr)))))| as |A_H lr A_W^T| with
      A_{N,n}[y, x] = (1/N) sum_{k=-(n//2)}^{n-1-n//2} exp(2 pi i k (y n - x N) / (N n)); no rescaling."""
import numpy as np
import torch

from sr355 import Context


def _resize(lr_img, target_shape, interpolation):
    ctx = Context.get()
    out_w, out_h = int(target_shape[0]), int(target_shape[1])
    a = np.asarray(lr_img)
    gray = a.ndim == 2
    if gray:
        a = a[:, :, None]
    if a.dtype == np.uint8:
        x = ctx.to_device(a[None], torch.uint8)
    else:
        x = ctx.to_device(a[None].astype(np.float32, copy=False))
    y = ctx.resize(x, out_h, out_w, interpolation)[0].cpu().numpy()
    return y[:, :, 0] if gray else y


def interpolate_bilinear(lr_img, target_shape):
    """Bilinear upscaling (classic_algorithms.py:7-9)."""
    return _resize(lr_img, target_shape, "INTER_LINEAR")


def interpolate_bicubic(lr_img, target_shape):
    """Bicubic upscaling (classic_algorithms.py:11-13)."""
    return _resize(lr_img, target_shape, "INTER_CUBIC")


def interpolate_area(lr_img, target_shape):
    """Area (resampling) upscaling (classic_algorithms.py:15-17)."""
    return _resize(lr_img, target_shape, "INTER_AREA")


def interpolate_lanczos(lr_img, target_shape):
    """Lanczos-4 upscaling (classic_algorithms.py:19-21)."""
    return _resize(lr_img, target_shape, "INTER_LANCZOS4")


def _gray_u8(name, *imgs):
    out = []
    for a in imgs:
        a = np.asarray(a)
        if a.ndim != 2 or a.dtype != np.uint8:
            raise NotImplementedError(f"{name}: runs on 2-D uint8 grayscale images (the reference's notebook passes cv2.COLOR_RGB2GRAY "
                                      f"conversions); got a {a.ndim}-D {a.dtype} array")
        out.append(a)
    return out


def _hw(name, ground_truth):
    shp = np.shape(ground_truth)
    if len(shp) < 2:
        raise ValueError(f"{name}: the first argument must be an image (its shape gives the output size)")
    return int(shp[0]), int(shp[1])


def _dev(ctx, a):
    return ctx.to_device(a[None], torch.uint8)


def back_projection(hr_image, lr_image, iterations=10):
    """Iterative back-projection, starting from hr_image (classic_algorithms.py:23-43) -> uint8 [H,W]."""
    hr, lr = _gray_u8("back_projection", hr_image, lr_image)
    ctx = Context.get()
    return ctx.back_projection(_dev(ctx, hr), _dev(ctx, lr), int(iterations))[0].cpu().numpy()


def non_local_means(hr_g, lr_g):
    """NL-means denoising of lr_g with the estimated noise sigma, then Lanczos-4 up to hr_g's size (classic_algorithms.py:45-62)
    -> float64 [H,W]."""
    (lr,) = _gray_u8("non_local_means", lr_g)
    H, W = _hw("non_local_means", hr_g)
    ctx = Context.get()
    return ctx.non_local_means(_dev(ctx, lr), H, W)[0].cpu().numpy().astype(np.float64)


def edge_guided_interpolation(ground_truth, image):
    """Bilinear up-scaling sharpened by 0.3 x the up-scaled Sobel magnitude (classic_algorithms.py:64-85) -> uint8 [H,W]."""
    (x,) = _gray_u8("edge_guided_interpolation", image)
    H, W = _hw("edge_guided_interpolation", ground_truth)
    ctx = Context.get()
    return ctx.edge_guided(_dev(ctx, x), H, W)[0].cpu().numpy()


def frequency_extrapolation(ground_truth, image):
    """Zero-padding of the centred spectrum to the HR size (classic_algorithms.py:87-108) -> float64 [H,W]."""
    (x,) = _gray_u8("frequency_extrapolation", image)
    H, W = _hw("frequency_extrapolation", ground_truth)
    if H < x.shape[0] or W < x.shape[1]:
        raise ValueError(f"frequency_extrapolation: target {H}x{W} is smaller than the {x.shape[0]}x{x.shape[1]} input")
    ctx = Context.get()
    return ctx.freq_extrapolate(_dev(ctx, x), H, W)[0].cpu().numpy()
