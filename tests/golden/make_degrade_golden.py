"""Writes tests/golden/degrade_jpeg.npz: seeded uint8 BGR images round-tripped through a real baseline-JPEG codec -- Pillow on
libjpeg-turbo, which shares libjpeg's defaults with OpenCV's codec (4:2:0 as saved here, "islow" DCTs, fancy up-sampling,
jpeg_set_quality(q, force_baseline)).  The pin of sr_degrade_jpeg's contract (include/sr355.h) and of its NumPy restatement
(tests/degrade_ref.py).  Needs Pillow; run from the repository root:  python tests/golden/make_degrade_golden.py

Keys: sizes [n, 2] (H, W); qualities; in_<H>x<W> the input; out_<H>x<W>_q<q> the decoded image; qt_q<q> [2, 64] the luminance and
chrominance tables Pillow reports for the file, row-major; versions (Pillow, libjpeg)."""
import io
import os

import numpy as np
from PIL import Image, features

SIZES = ((16, 16), (17, 23), (23, 17), (40, 24), (33, 16))          # one MCU; partial MCUs, odd both ways; even but no MCU multiple; one odd side
QUALITIES = (20, 49, 50, 59)


def make_image(H, W, seed):
    """Left half noise, right half smooth ramps with a saturated patch: range limiting and zeroed coefficients both occur."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    ramp = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), (xx + yy) * 255 // (H + W - 2)], -1).astype(np.uint8)
    img[:, W // 2:] = ramp[:, W // 2:]
    img[H // 4:H // 2, W // 2:3 * W // 4 + 1] = 255
    return img


def pillow_roundtrip(bgr, quality):
    """-> (decoded BGR, [luminance, chrominance] tables as Pillow reports them)"""
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(buf, format="JPEG", quality=int(quality), subsampling=2)
    buf.seek(0)
    with Image.open(buf) as im:
        tables = [np.asarray(im.quantization[i], np.int32) for i in (0, 1)]
        return np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8)[..., ::-1]), tables


def main():
    out = {"sizes": np.array(SIZES, np.int32), "qualities": np.array(QUALITIES, np.int32),
           "versions": np.array([f"Pillow {Image.__version__ if hasattr(Image, '__version__') else features.version('pil')}",
                                 f"libjpeg {features.version('jpg')} (libjpeg-turbo: {features.check_feature('libjpeg_turbo')})"])}
    for n, (H, W) in enumerate(SIZES):
        img = make_image(H, W, 100 + n)
        out[f"in_{H}x{W}"] = img
        for q in QUALITIES:
            dec, tables = pillow_roundtrip(img, q)
            out[f"out_{H}x{W}_q{q}"] = dec
            out[f"qt_q{q}"] = np.stack(tables)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "degrade_jpeg.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
