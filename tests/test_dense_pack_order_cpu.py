"""csrc/dense_plan.h, frag_at: the order chain_pack_weights packs a fused pair's weight fragments in.  The kernel's stage k of a granule uses
the granule's fragment k, so the order must be the stage lists' own; and it must hold every (conv, chunk, ky, kx, cout block) of the two convs
exactly once.  The tables are the header's (tests/dense_plan.py)."""
import pytest

import dense_plan


@pytest.mark.parametrize("cfg", dense_plan.SHAPES)
def test_fragment_order_is_the_stage_order_and_covers_both_convs_once(cfg):
    ext, nb0, nb1, mode = cfg
    t = dense_plan.shape(cfg)
    frags = [tuple(f) for f in t["frags"]]
    assert len(frags) == 3 * ext * 3 * (nb0 + nb1) + 9 * nb1
    # conv 0 reads chunks [0, ext), conv 1 chunks [0, ext]; every (ky, kx) tap and cout block of each
    want = [(0, c, ky, kx, n) for c in range(ext) for ky in range(3) for kx in range(3) for n in range(nb0)]
    want += [(1, c, ky, kx, n) for c in range(ext + 1) for ky in range(3) for kx in range(3) for n in range(nb1)]
    assert sorted(frags) == sorted(want) and len(set(frags)) == len(frags)
    # external granule (chunk c, kx): fragment k is stage k's weight -- its layer's conv, ky = d - 1 for layer 0 (row 8s+w reads staged row w+1+ky),
    # ky = d for layer 1 (row 8s+w-1 reads staged row w+ky)
    stages = t["ext_stages"]
    per = len(stages)
    assert per == 3 * (nb0 + nb1) and t["npieces"][0] == per
    for g in range(3 * ext):
        for k, (d, layer, n, first) in enumerate(stages):
            assert frags[g * per + k] == (layer, g // 3, d - 1 if layer == 0 else d, g % 3, n), (cfg, g, k)
    # a row's first stage is marked, rows come in order, and every stage's ky is a real tap
    assert [s[0] for s in stages] == sorted(s[0] for s in stages)
    assert [k for k, s in enumerate(stages) if s[3]] == [min(k for k, s in enumerate(stages) if s[0] == d) for d in range(4)]
    assert all(0 <= (d - 1 if layer == 0 else d) <= 2 for d, layer, n, first in stages)
    # ring granule kx (conv 1 on conv 0's output = its chunk ext): fragment k is (ky = k / nb1, n = k % nb1)
    ring = t["ring_stages"]
    assert len(ring) == 3 * nb1 == t["npieces"][3 * ext]
    for kx in range(3):
        for k in range(3 * nb1):
            assert tuple(ring[k]) == (k // nb1, k % nb1)
            assert frags[3 * ext * per + kx * 3 * nb1 + k] == (1, ext, k // nb1, kx, k % nb1), (cfg, kx, k)
