"""csrc/dense_fused.hip, compute waves: a model check of the operand reads a granule issues for its SUCCESSOR (one continuous software
pipeline per compute wave, `CarryPlan`), in the style of test_loader_schedule_cpu.py.

During granule G -- between barrier G, which opens it, and barrier G + 1 -- a compute wave requests the first WDEPTH weight fragments of
granule G + 1 from the next weight slot and, where the plan allows it, the pixel fragments of granule G + 1's row 0.  Those reads are legal
only if, for every LDS location they touch,
  (a) the last write to it was issued in an iteration that ended at barrier G or earlier, and has landed when barrier G opens: a resident
      piece (ds_write_b128) is drained by the loader's lgkmcnt(0) in front of the next barrier; an LDS-DMA piece lands when the loader's
      counted vmcnt says so (in-order retirement, as in test_loader_schedule_cpu.py); a ring row is written in the layer-0 epilogue;
  (b) no write to it is issued before barrier G + 2, the barrier that ends the consuming granule G + 1.
The loaders' schedule (LoaderPlan) and the plan are the kernels' own -- csrc/dense_plan.h, dumped by tests/dense_plan.py -- and are replayed
together in the loader loop's order of issue: all four loaders, the tail (EXT 5, NB 2 / 4) and both growth pairs (EXT 2 and 3, NB 2 / 2),
several steps.  The growth pairs carry nothing (their two weight slots are written
one granule ahead, i.e. while the pre-read would run: the model shows it); the test still walks them, so that switching their plan on
without a weight ring that allows it fails here.  The header's LDS byte sums are pinned and checked against the 160 KiB of a CU."""
import pytest

import dense_plan

_P = dense_plan.plan()
NLOAD, NCOMP, WDEPTH, WINR = _P["NLOAD"], _P["NCOMP"], _P["WDEPTH"], _P["WINR"]
LDS_LIMIT = 160 * 1024


class Cfg:
    """One shape's dumped tables, with the hooks of the negative tests: carry=True reads the plan as if it were switched on,
    carry_x_across_chunks=True lets pixel pre-reads follow every weight pre-read, `dma` turns resident pieces (iw, k) into DMA pieces."""

    def __init__(self, ext, nb0, nb1, mode, carry=None, carry_x_across_chunks=False):
        t = self.t = dense_plan.shape((ext, nb0, nb1, mode))
        self.ext, self.nb0, self.nb1, self.mode = ext, nb0, nb1, mode
        self.extg, self.ngr, self.wl, self.sl = t["extg"], t["ngr"], t["wl"], t["sl"]
        self.nsb, self.nws = t["lds"]["nsb"], t["lds"]["nws"]
        self.carry = t["carry_forced" if carry else "carry"]
        self.x_across_chunks = carry_x_across_chunks
        self.dma = lambda iw, k: False

    def lds_bytes(self):
        return self.t["lds"]["bytes"]

    def rows(self, lw, kx):
        return self.t["loaders"][lw]["rows"][kx]

    def npieces(self, iw):
        return self.t["npieces"][iw]

    def resident(self, iw, k):
        return bool(self.t["loaders"][k % NLOAD]["resident"][iw][k]) and not self.dma(iw, k)

    def wait_n(self, lw, i):
        """The plan's count; a piece a hook took out of the registers is one more DMA piece of the granule whose weights iteration i issues."""
        t = self.t["loaders"][lw]
        iw = t["issue_w"][i]
        return t["wait_n"][i] + sum(1 for k in range(lw, self.npieces(iw), NLOAD) if self.dma(iw, k))

    # ---- what granule i of a step (external: i < extg; ring: kx = i - extg) finds requested by its predecessor
    def pre_w(self, i):
        return bool(self.carry["pre_w"][i])

    def pre_x(self, i):
        return self.pre_w(i) if self.x_across_chunks else bool(self.carry["pre_x"][i])


class Write:
    __slots__ = ("issued", "landed")

    def __init__(self, issued, landed=None):
        self.issued, self.landed = issued, landed        # iteration it was issued in (-1: prologue); barrier at which it is visible


def replay(cfg, nsteps):
    """-> (writes, granules): writes[location] = [Write, ...] in issue order; granules[G] = (position in the step, chunk number, step).
    Iteration G runs from barrier G to barrier G + 1.  Locations: ("w", slot, piece), ("s", staging buffer, row), ("r", ring row)."""
    writes, granules = {}, []

    def put(loc, w):
        writes.setdefault(loc, []).append(w)

    for lw in range(NLOAD):
        queue, done = [], 0                                # this loader's DMA operations in issue order (in-order retirement)

        def weights(iw, gw, it):
            for k in range(lw, cfg.npieces(iw), NLOAD):
                loc = ("w", gw % cfg.nws, k)
                if cfg.resident(iw, k):
                    put(loc, Write(it, it + 1))            # ds_write_b128, drained by lgkmcnt(0) in front of the next barrier
                else:
                    w = Write(it)
                    put(loc, w)
                    queue.append(w)

        def rows(kx, chunk_no, it):
            for j in cfg.rows(lw, kx):
                for _ in range(3):                         # three 1 KiB pieces per row
                    w = Write(it)
                    put(("s", chunk_no % cfg.nsb, j), w)
                    queue.append(w)

        for g in range(cfg.wl):
            weights(g % cfg.ngr, g, -1)
        for c0 in range(cfg.sl):
            for kx in (0, 1):
                rows(kx, c0, -1)
        for w in queue:
            w.landed = 0                                   # vmcnt(0) and lgkmcnt(0) before the first barrier
        for loc in writes:
            for w in writes[loc]:
                if w.issued == -1:
                    w.landed = 0
        done = len(queue)
        G, nch = 0, 0
        for s in range(nsteps):
            for i in range(cfg.ngr):
                if lw == 0:
                    granules.append((i, nch, s))
                weights(cfg.t["loaders"][lw]["issue_w"][i], G + cfg.wl, G)
                if i < cfg.extg:
                    rows(i % 3, nch + cfg.sl, G)
                n = cfg.wait_n(lw, i)
                for w in queue[done:max(done, len(queue) - n)]:
                    w.landed = G + 1
                done = max(done, len(queue) - n)
                if i < cfg.extg and i % 3 == 2:
                    nch += 1
                G += 1
    # compute waves: wave w writes ring row (8 s + w) % WINR in the layer-0 epilogue, in the iteration of the step's last external granule
    for s in range(nsteps):
        it = s * cfg.ngr + cfg.extg - 1
        for w in range(NCOMP):
            put(("r", (8 * s + w) % WINR), Write(it, it + 1))      # sync() behind an epilogue waits lgkmcnt(0)
    for loc in writes:
        writes[loc].sort(key=lambda w: w.issued)
    return writes, granules


def prereads(cfg, granules, G):
    """LDS locations a compute wave reads during granule G for granule G + 1 (all eight waves), per the plan."""
    if G + 1 >= len(granules):
        return []
    i1, nch1, s1 = granules[G + 1]
    if granules[G][2] != s1:
        return []                                          # nothing is carried across the bias re-initialisation
    locs = []
    if cfg.pre_w(i1):
        locs += [("w", (G + 1) % cfg.nws, k) for k in range(WDEPTH)]
    if cfg.pre_x(i1):
        if i1 < cfg.extg:
            locs += [("s", nch1 % cfg.nsb, w) for w in range(NCOMP)]                     # staged row d = 0 of wave w is row w
        else:
            locs += [("r", (8 * s1 + w - 2) % WINR) for w in range(NCOMP)]               # ring row of ky = 0: stream row 8 s + w - 2
    return locs


def check(cfg, nsteps=6):
    writes, granules = replay(cfg, nsteps)
    covered = 0
    for G in range(len(granules)):
        locs = prereads(cfg, granules, G)
        covered += bool(locs)
        for loc in locs:
            ws = writes.get(loc, [])
            before = [w for w in ws if w.issued < G]
            if loc[0] != "r" or before:                     # (ring rows start as zeros: rows above the first image)
                assert before, (loc, "never written before granule", G)
                last = before[-1]
                assert last.landed is not None and last.landed <= G, (loc, "granule", G, "last write issued in iteration", last.issued, "lands at barrier", last.landed)
            early = [w for w in ws if G <= w.issued < G + 2]
            assert not early, (loc, "granule", G, "rewritten in iteration", early[0].issued if early else None, "before barrier", G + 2)
    return covered, len(granules)


TAIL, PAIR2, PAIR3 = (5, 2, 4, 1), (2, 2, 2, 0), (3, 2, 2, 0)


@pytest.mark.parametrize("shape", [TAIL, PAIR2, PAIR3])
def test_every_preread_is_published_and_not_rewritten(shape):
    cfg = Cfg(*shape)
    covered, total = check(cfg, nsteps=6)
    assert total == 6 * cfg.ngr
    if cfg.mode == 1:
        assert covered == 6 * 16 and cfg.ngr == 18          # 16 of a tail step's 18 barriers have pre-reads in flight
    else:
        assert covered == 0                                 # the growth pairs restart their pipeline behind every barrier


def test_tail_plan_in_detail():
    cfg = Cfg(*TAIL)
    # weights: every granule but a step's first and ring kx = 0; pixels: additionally not across a chunk boundary
    assert [i for i in range(cfg.ngr) if cfg.pre_w(i)] == [i for i in range(cfg.ngr) if i not in (0, cfg.extg)]
    assert [i for i in range(cfg.ngr) if cfg.pre_x(i)] == [i for i in range(cfg.ngr) if i not in (0, cfg.extg) and (i > cfg.extg or i % 3 != 0)]
    # the pre-read fragments are pieces the loaders keep in registers and write a granule early (t < RT_E / RT_R), for every granule position
    for iw in range(cfg.ngr):
        assert all(cfg.resident(iw, k) for k in range(WDEPTH))
        assert [k for k in range(cfg.npieces(iw)) if cfg.resident(iw, k)] == list(range(8))     # (a granule's first eight fragments, as the packer says)


def test_model_catches_pixels_across_a_tail_chunk_boundary():
    """Two staging buffers: the next chunk's rows are published by the very barrier in between."""
    with pytest.raises(AssertionError):
        check(Cfg(*TAIL, carry_x_across_chunks=True))


@pytest.mark.parametrize("shape", [PAIR2, PAIR3])
def test_model_catches_weight_prereads_from_a_two_slot_ring(shape):
    """Growth pairs: the slot of granule G + 1 is written while granule G runs, so its head cannot be read a granule early (it would take a
    ring of its own, written two granules ahead)."""
    with pytest.raises(AssertionError):
        check(Cfg(*shape, carry=True))


def test_model_catches_a_dma_piece_among_the_head_fragments():
    """A head fragment that came by LDS-DMA is waited for one iteration too late for the pre-read (the old fragment order: stage 2 used piece 8)."""
    cfg = Cfg(*TAIL)
    assert all(cfg.resident(iw, 2) for iw in range(cfg.ngr))
    cfg.dma = lambda iw, k: k == 2
    with pytest.raises(AssertionError):
        check(cfg)


def test_lds_byte_sums():
    tail, pair = Cfg(*TAIL), Cfg(*PAIR3)
    assert tail.lds_bytes() == 2 * 33 * 1024 + 30 * 1024 + 3 * 18 * 1024 + 6 * 64 == 153984
    assert pair.lds_bytes() == Cfg(*PAIR2).lds_bytes() == 3 * 33 * 1024 + 30 * 1024 + 2 * 12 * 1024 + 4 * 64 == 156928
    assert tail.lds_bytes() <= LDS_LIMIT and pair.lds_bytes() <= LDS_LIMIT
