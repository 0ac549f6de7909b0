"""sr_dense_block_lds_bytes (csrc/dense_block.hip): which images the LDS-resident dense-block kernel takes.  A pure function of the ABI, asked by
sr_forward's router, by the kernel's launcher and by the GPU tests -- no device needed."""
import os
import re

from sr355 import _lib as L
from sr355.runtime import Context

LDS_OF_A_CU = 160 * 1024
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lds(g, h, w):
    return Context.dense_block_lds_bytes(g, h, w)


def test_accepts_every_image_of_at_most_676_padded_pixels():
    for shape in ((8, 1, 1), (8, 13, 21), (8, 24, 24)):
        assert 0 < lds(*shape) <= LDS_OF_A_CU, shape
    n = 0
    for h in range(1, 675):
        for w in range(1, 675):
            if (h + 2) * (w + 2) > 676:
                break
            assert 0 < lds(8, h, w) <= LDS_OF_A_CU, (h, w)
            n += 1
    assert n > 1000                                       # 24 x 24 among them: 26 * 26 = 676
    assert (24 + 2) * (24 + 2) == 676


def test_rejects_what_the_kernel_does_not_take():
    for shape in ((8, 48, 48), (16, 24, 24), (32, 24, 24), (8, 0, 5), (8, 5, 0), (8, -1, 24), (0, 24, 24)):
        assert lds(*shape) == -1, shape


def test_non_decreasing_in_height_up_to_the_boundary():
    for w in (1, 5, 24, 31):
        prev, rejected = 0, False
        for h in range(1, 400):
            v = lds(8, h, w)
            if v == -1:
                rejected = True                              # once too large, every taller image is too
                continue
            assert not rejected and prev <= v <= LDS_OF_A_CU, (h, w, prev, v)
            prev = v
        assert rejected, w


def test_exported_declared_and_bound():
    assert "sr_dense_block_lds_bytes" in L.SIGNATURES
    lib = L.load()
    assert lib.sr_dense_block_lds_bytes(8, 24, 24) == lds(8, 24, 24)
    with open(os.path.join(ROOT, "include", "sr355.h")) as f:
        header = f.read()
    assert re.search(r"int64_t\s+sr_dense_block_lds_bytes\(int growth_channels, int H, int W\);", header)
