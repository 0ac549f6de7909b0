"""tests/grid_caps.py against the source it restates: every case crosses its cap raggedly, and every capped launch site of csrc/ is
either crossed by a case, covered by a named test elsewhere, or listed with the reason nothing can cross it.  No GPU."""
import os
import re
import shutil

import pytest

import grid_caps as G
import image_ops_cases as T

ROOT = G.ROOT


def test_the_caps_are_the_ones_in_the_source():
    assert G.CAPS == {"train_ops.hip": 65535 * 256, "imgops.hip": 8192 * 256, "study.hip": 8192 * 256, "classic.hip": 65535 * 256,
                      "metrics.hip": 65535 * 256, "eda.hip": 65535 * 256}
    assert G.PAIRS_CAP == 8192 * 256 and G.WARP_PATCH_CAP == 1024 * 256 and G.AFFINE_CAP == 1024 * 256 and G.CROP_MASK_CAP == 1024 * 256
    assert G.PACK_CAP == 4096 * 256 and G.SITES[("degrade.hip", "degrade_motion_kernel")] == (1 << 20) * 256
    assert G.SITES[("cgemm_f64.h", "dft_full_operator_kernel")] == 65535 * 256
    for k in ("sqdiff_partial_kernel", "absdiff_partial_kernel"):           # grid_for's result clamped again to 1024 blocks
        assert G.SITES[("imgops.hip", k)] == G.REDUCE_BLOCKS * 256


@pytest.mark.parametrize("case", G.CASES, ids=[c.id for c in G.CASES])
def test_every_case_crosses_its_cap_raggedly(case):
    for site in case.sites:
        assert G.SITES[site] == case.cap, (site, G.SITES[site], case.cap)
    assert case.threads > case.cap, f"{case.id}: {case.threads} threads no longer exceed the cap of {case.cap}"
    assert case.threads % case.cap != 0, f"{case.id}: the last round is a full one"


def test_the_last_round_ends_inside_a_block_somewhere_in_every_family():
    """A shape set by its op (even sides for space_to_depth, 48 x 48 x 3 patches) may be a multiple of the block; each file whose ops leave
    the size free has a case whose last block is part-filled."""
    ragged = {f for c in G.CASES if c.threads % G.BLOCK for f, _ in c.sites}
    assert ragged >= {"train_ops.hip", "imgops.hip", "head_train.hip", "classic.hip", "metrics.hip"}, ragged


def test_every_capped_launch_site_is_accounted_for():
    cased = {s for c in G.CASES for s in c.sites}
    listed = set(G.COVERED_ELSEWHERE) | set(G.UNREACHABLE)
    found = set(G.SITES)
    assert not (cased & listed), cased & listed
    assert not (set(G.COVERED_ELSEWHERE) & set(G.UNREACHABLE))
    assert found - cased - listed == set(), f"capped launches without a case: {sorted(found - cased - listed)}"
    assert (cased | listed) - found == set(), f"named in the tables but not found in the source: {sorted((cased | listed) - found)}"
    assert all(len(r) > 20 for r in list(G.COVERED_ELSEWHERE.values()) + list(G.UNREACHABLE.values()))
    assert len(found) >= 50


def test_design_md_has_a_row_for_every_site():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("**Every capped launch grid is crossed"):text.index("**Synthetic weights: attention logits conditioned.**")]
    missing = [s for s in sorted(G.SITES) if f"| `{s[0]}` `{s[1]}` |" not in section]
    assert not missing, missing


def test_the_tests_named_as_covering_a_site_exist_with_that_shape():
    src = open(os.path.join(ROOT, "tests", "test_classifier_ops_gpu.py")).read()
    assert "def test_maxpool2_signed_and_odd" in src and "(6, 194, 130, 64)" in src
    assert 6 * 97 * 65 * 64 > G.IMG_CAP
    assert "def test_psnr_mse_sizes" in open(os.path.join(ROOT, "tests", "test_image_ops_gpu.py")).read()
    (shape, _) = T.REDUCE_CASES[0]
    assert shape[1] * shape[2] * shape[3] > G.REDUCE_BLOCKS * 256 and T.MAX_REDUCE_BLOCKS == G.REDUCE_BLOCKS


def test_the_unreachable_sites_are_what_the_source_says():
    metrics = open(os.path.join(G.CSRC, "metrics.hip")).read()
    chunk = G._value(re.search(r"FFT_CHUNK_BYTES\s*=\s*\(size_t\)\s*" + G._NUM, metrics).group(1))
    assert "per_img = sizeof(double) * (size_t)HW * 3" in metrics                 # X and T's two parts: 24 bytes per gray value
    assert chunk // 24 < G.MET_CAP
    # eda.hip's two chunked loops: 32 bytes per value for the spectra (never crosses), 16 with a caller's DCT buffer (the eda_dct case)
    eda = open(os.path.join(G.CSRC, "eda.hip")).read()
    assert "per_img = sizeof(double) * (size_t)HW * 4" in eda and "(dct_f64 ? 2 : 3)" in eda
    assert G.EDA_CHUNK_BYTES // 32 < G.CAPS["eda.hip"] < G.EDA_CHUNK_BYTES // 16
    assert 4095 * 4095 < G.CLS_CAP < 4096 * 4096                                  # the three operator kernels: one thread per element of N x N
    assert 391 * 478 * 478 * 3 <= G.SITES[("degrade.hip", "degrade_motion_kernel")] < 392 * 478 * 478 * 3


def test_cases_take_the_kernels_they_name():
    kernel_of = {"nearest": "resize_nearest_kernel", "float_taps": "resize_apply_f32_kernel", "fixed_u8": "resize_apply_u8_kernel",
                 "area_fast_u8": "resize_area_fast_u8_kernel", "area_taps_u8": "resize_apply_area_u8_kernel"}
    for cid, dtype, shape, interp, kernel in G.RESIZE_CASES:
        route = T.resize_route(dtype, shape, G.RS_OUT, interp)
        assert kernel.startswith(kernel_of[route.kernel]) and not route.rewritten, (cid, route)
    for cid, dtype, shape, kernel in G.BICUBIC_CASES:
        assert T.bicubic_route(dtype, shape, G.RS_OUT).kernel == {"bicubic_f32_kernel": "pixel", "bicubic_u8_kernel": "u8"}[kernel], cid
    (F, H, W, C), p, s = G.BY_ID["extract_batch_quad"].arg
    assert p * C % 4 == 0 and G.SCALAR_PATCH * 3 % 4 != 0                          # extract_patches_batch's choice between its two kernels
    n, H, W, C = G.BY_ID["affine_warp_v4"].arg
    assert H * W * C % 4 == 0 and 513 * 513 % 4 != 0
    # the classic batch: a round of the HR-sized launches ends inside images 73, 146, 220 and 293, of the LR-sized ones inside image 293
    assert G.images_crossed(G.CLS_CAP, G.CLS_HR ** 2, G.CLS_NH) == [73, 146, 220, 293]
    assert G.images_crossed(G.CLS_CAP, G.CLS_LR ** 2, G.CLS_NL) == [293]
    assert G.EDA_CHUNK == 4096 == 2 * G.EDA_PAIRS


def test_a_changed_cap_is_reported_case_by_case(tmp_path):
    """imgops.hip's cap doubled in a scratch copy of csrc/: the sites keep their names, and exactly the cases that no longer cross are named."""
    scratch = tmp_path / "csrc"
    shutil.copytree(G.CSRC, scratch)
    p = scratch / "imgops.hip"
    text = p.read_text()
    assert text.count("const int64_t cap = 256 * 8 * 4;") == 1
    p.write_text(text.replace("const int64_t cap = 256 * 8 * 4;", "const int64_t cap = 256 * 8 * 8;"))
    sites = G.capped_sites(str(scratch))
    assert set(sites) == set(G.SITES)
    lost = sorted(c.id for c in G.CASES if any(c.threads <= sites[s] for s in c.sites))
    assert lost == sorted(c.id for c in G.CASES if c.sites[0][0] == "imgops.hip" and c.cap == G.IMG_CAP and c.threads <= 2 * G.IMG_CAP), lost
    assert "l1" not in lost and "tap_copy" not in lost and "extract_batch_quad" not in lost and "resize_linear_f32" in lost and len(lost) >= 25


def test_a_new_capped_launch_is_found(tmp_path):
    scratch = tmp_path / "csrc"
    shutil.copytree(G.CSRC, scratch)
    p = scratch / "study.hip"
    p.write_text(p.read_text() + "\nint extra_launch(int64_t n, hipStream_t st) {\n    hipLaunchKernelGGL(extra_kernel, dim3(grid_for(n)), dim3(256), 0, st, n);\n"
                 "    const unsigned gx = (unsigned)std::min<int64_t>((n + 255) / 256, 512);\n    hipLaunchKernelGGL(extra2_kernel, dim3(gx, 3), dim3(256), 0, st, n);\n    return 0;\n}\n")
    new = set(G.capped_sites(str(scratch))) - set(G.SITES)
    assert new == {("study.hip", "extra_kernel"), ("study.hip", "extra2_kernel")}
    assert G.capped_sites(str(scratch))[("study.hip", "extra2_kernel")] == 512 * 256
