"""csrc/dense_fused.hip, compute waves: a model check of the operand reads a granule issues for its SUCCESSOR (one continuous software
pipeline per compute wave, `CarryPlan`), in the style of test_loader_schedule_cpu.py.

During granule G -- between barrier G, which opens it, and barrier G + 1 -- a compute wave requests the first WDEPTH weight fragments of
granule G + 1 from the next weight slot and, where the plan allows it, the pixel fragments of granule G + 1's row 0.  Those reads are legal
only if, for every LDS location they touch,
  (a) the last write to it was issued in an iteration that ended at barrier G or earlier, and has landed when barrier G opens: a resident
      piece (ds_write_b128) is drained by the loader's lgkmcnt(0) in front of the next barrier; an LDS-DMA piece lands when the loader's
      counted vmcnt says so (in-order retirement, as in test_loader_schedule_cpu.py); a ring row is written in the layer-0 epilogue;
  (b) no write to it is issued before barrier G + 2, the barrier that ends the consuming granule G + 1.
The loaders' schedule (LoaderPlan, the loader loop) and the plan are restated here and replayed together: all four loaders, the tail (EXT 5,
NB 2 / 4) and both growth pairs (EXT 2 and 3, NB 2 / 2), several steps.  The growth pairs carry nothing (their two weight slots are written
one granule ahead, i.e. while the pre-read would run: the model shows it); the test still walks them, so that switching their plan on
without a weight ring that allows it fails here.  The LDS byte sums of both kernels are restated and checked against the 160 KiB of a CU."""
import pytest

NLOAD, NCOMP, WDEPTH = 4, 8, 3
ROWB, NSTG, WINR = 3072, 11, 10
LDS_LIMIT = 160 * 1024


class Cfg:
    def __init__(self, ext, nb0, nb1, mode, carry=None, carry_x_across_chunks=None):
        self.ext, self.nb0, self.nb1, self.mode = ext, nb0, nb1, mode
        self.nbt, self.extg, self.ngr = nb0 + nb1, 3 * ext, 3 * (ext + 1)
        self.rt_e, self.rt_r = (2 if mode == 1 else 3), 2
        self.nsb, self.nws = (3, 2) if mode == 0 else (2, 3)
        self.wl, self.sl = self.nws - 1, self.nsb - 1
        self.wslot = self.nbt * 3 * 1024
        # CarryPlan / kCarry: the tail carries, the growth pairs do not; pixels across a chunk boundary only with three staging buffers
        self.carry = (mode == 1) if carry is None else carry
        self.x_across_chunks = (mode == 0) if carry_x_across_chunks is None else carry_x_across_chunks

    def lds_bytes(self):
        return self.nsb * NSTG * ROWB + WINR * ROWB + self.nws * self.wslot + self.nbt * 16 * 4

    # ---- LoaderPlan
    def rows(self, lw, kx):
        return [lw, lw + 4] if kx == 0 else ([8 + lw] if (kx == 1 and lw < 3) else [])

    def nst_at(self, lw, i):
        i %= self.ngr
        return 3 * len(self.rows(lw, i % 3)) if i < self.extg else 0

    def npieces(self, iw):
        return self.nbt * 3 if iw < self.extg else self.nb1 * 3

    def resident(self, iw, k):
        return k // NLOAD < (self.rt_e if iw < self.extg else self.rt_r)

    def nwdma(self, lw, iw):
        return sum(1 for k in range(lw, self.npieces(iw), NLOAD) if not self.resident(iw, k))

    def wait_n(self, lw, i):
        if self.mode == 0:
            return self.nst_at(lw, i) + self.nst_at(lw, i - 1) + self.nst_at(lw, i - 2)
        third = i < self.extg and i % 3 == 2
        return self.nwdma(lw, (i + self.wl) % self.ngr) + self.nst_at(lw, i) + (0 if third else self.nst_at(lw, i - 1))

    # ---- CarryPlan: what granule i of a step (external: i < extg; ring: kx = i - extg) finds requested by its predecessor
    def pre_w(self, i):
        return self.carry and ((0 < i < self.extg) or i > self.extg)

    def pre_x(self, i):
        if not self.pre_w(i):
            return False
        return i > self.extg or i % 3 != 0 or self.x_across_chunks


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
                weights((i + cfg.wl) % cfg.ngr, G + cfg.wl, G)
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
    real = cfg.resident
    cfg.resident = lambda iw, k: real(iw, k) and k != 2
    cfg.nwdma = lambda lw, iw: sum(1 for k in range(lw, cfg.npieces(iw), NLOAD) if not cfg.resident(iw, k))
    with pytest.raises(AssertionError):
        check(cfg)


def test_lds_byte_sums():
    tail, pair = Cfg(*TAIL), Cfg(*PAIR3)
    assert tail.lds_bytes() == 2 * 33 * 1024 + 30 * 1024 + 3 * 18 * 1024 + 6 * 64 == 153984
    assert pair.lds_bytes() == Cfg(*PAIR2).lds_bytes() == 3 * 33 * 1024 + 30 * 1024 + 2 * 12 * 1024 + 4 * 64 == 156928
    assert tail.lds_bytes() <= LDS_LIMIT and pair.lds_bytes() <= LDS_LIMIT
