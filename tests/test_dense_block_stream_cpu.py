"""The pure host functions of the streamed dense-block kernel (csrc/dense_block_stream.hip) -- sr_dense_block_stream_lds_bytes: which widths the row ring
takes; sr_dense_block_stream_bands: how images are cut into bands of rows -- their declarations, and the validation of ESRGAN's infer_dense_block option.
No device needed."""
import ctypes as C
import os
import re

import pytest

from sr355 import _lib as L
from sr355.runtime import Context

LDS_OF_A_CU = 160 * 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sr_dense_block_stream_lds_bytes", "sr_dense_block_stream_bands", "sr_model_set_dense_block_stream", "sr_debug_set_block_stream_bands")


def lds(g, w):
    return Context.dense_block_stream_lds_bytes(g, w)


def test_every_width_up_to_96_fits_a_cu():
    for w in range(1, 97):
        assert 0 < lds(8, w) <= LDS_OF_A_CU, w
    assert lds(8, 48) >= 12 * 400 * 16                    # at least a ring of 8 rows of 50 slots in 12 planes


def test_non_decreasing_in_width_until_the_first_rejection():
    prev, rejected = 0, None
    for w in range(1, 400):
        v = lds(8, w)
        if rejected is not None:
            assert v == -1, (w, v)                         # once too wide, every wider image is too
            continue
        if v == -1:
            rejected = w
            continue
        assert prev <= v <= LDS_OF_A_CU, (w, prev, v)
        prev = v
    assert rejected is not None and rejected > 96, rejected


def test_rejects_what_the_kernel_does_not_take():
    for g in (0, 16, 32):
        for w in (1, 24, 48, 96):
            assert lds(g, w) == -1, (g, w)
    for w in (0, -1, -48):
        assert lds(8, w) == -1, w


@pytest.mark.parametrize("cus", (1, 256))
def test_bands_cover_the_image_exactly_once(cus):
    lib = L.load()
    for B in (1, 3, 100, 256, 1000):
        for H in (1, 5, 6, 13, 48, 239):
            y0 = Context.dense_block_stream_bands(B, H, cus)
            n = len(y0)
            assert 1 <= n <= H, (B, H, cus, y0)
            assert y0[0] == 0 and all(a < b for a, b in zip(y0, y0[1:])) and y0[-1] < H, (B, H, cus, y0)      # non-empty, ascending: band b = [y0[b], y0[b + 1]), the last to H
            covered = [0] * H
            for a, b in zip(y0, y0[1:] + [H]):
                for y in range(a, b):
                    covered[y] += 1
            assert covered == [1] * H, (B, H, cus, y0)
            if B >= cus:
                assert n == 1, (B, H, cus, y0)
            # the count alone, and a capacity that does not hold the bands: reported, nothing written
            assert lib.sr_dense_block_stream_bands(B, H, cus, None, 0) == n
            if n > 1:
                buf = (C.c_int32 * n)(*([-7] * n))
                assert lib.sr_dense_block_stream_bands(B, H, cus, buf, n - 1) == -1
                assert list(buf) == [-7] * n
    assert len(Context.dense_block_stream_bands(1, 239, 256)) > 1      # few images on many CUs: the case bands exist for
    for bad in ((0, 5, 4), (1, 0, 4), (1, 5, 0)):
        assert lib.sr_dense_block_stream_bands(*bad, None, 0) == -1, bad


def test_exported_declared_and_bound():
    lib = L.load()
    with open(os.path.join(ROOT, "include", "sr355.h")) as f:
        header = f.read()
    for name in NEW:
        assert name in L.SIGNATURES, name
        assert getattr(lib, name) is not None, name
        assert re.search(r"\b" + name + r"\(", header), name
    assert re.search(r"int64_t\s+sr_dense_block_stream_lds_bytes\(int growth_channels, int W\);", header)
    assert re.search(r"int\s+sr_dense_block_stream_bands\(int B, int H, int num_cus, int32_t\* y0_out, int cap\);", header)
    assert re.search(r"int\s+sr_model_set_dense_block_stream\(sr_model\* m, int mode\);", header)
    assert re.search(r"int\s+sr_debug_set_block_stream_bands\(sr_ctx\* ctx, int n\);", header)
    assert lib.sr_dense_block_stream_lds_bytes(8, 48) == lds(8, 48)


def test_the_wrapper_validates_infer_dense_block():
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    with pytest.raises(ValueError):
        ESRGAN(infer_dense_block="x")
    assert ESRGAN().infer_dense_block == "layers"
    # an explicit opt-in on a model the kernel cannot serve raises before anything is built on a device
    with pytest.raises(ValueError):
        ESRGAN(compute_dtype="f32", infer_dense_block="stream").setup_model(scale_factor=2, growth_channels=8, num_rrdb_blocks=1)
    with pytest.raises(ValueError):
        ESRGAN(compute_dtype="bf16", infer_dense_block="stream").setup_model(scale_factor=2, growth_channels=32, num_rrdb_blocks=1)


def test_the_wrapper_validates_a_growth_width_read_from_a_checkpoint(tmp_path):
    import numpy as np
    from SRModels.deep_learning_models.ESRGAN_model import ESRGAN
    from sr355.weights import save_npz
    path = str(tmp_path / "g16.npz")
    save_npz(path, {"rrdb_0_dense1_conv1": (np.zeros((3, 3, 64, 16), np.float32), np.zeros(16, np.float32))})
    with pytest.raises(ValueError, match="growth_channels"):       # asked for 8, the checkpoint says 16
        ESRGAN(compute_dtype="bf16", infer_dense_block="stream").setup_model(scale_factor=2, growth_channels=8, from_trained=True, generator_pretrained_path=path)
