"""GPU tests of jfsx_gather_batch (gather_pages_k): pages assembled from pieces
of source blocks and zeros in one launch, in host and in device memory.  Every
destination is surrounded by 0xA5 guard bytes that must stay; every expected
byte is numpy's (tests/compact_model.gather_want)."""
import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import compact_model as CM

pytestmark = pytest.mark.gpu

MEMS = [E.MEM_HOST, E.MEM_DEVICE]
MEM_IDS = ["host", "device"]
GUARD = 64
T = E.GATHER_TILE


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


def _rand(seed, n):
    return np.random.default_rng(seed).integers(1, 256, n, dtype=np.uint8).tobytes()


class GBatch:
    """One call laid out in host memory (sources and destinations at odd
    addresses) or device memory (16-byte aligned), 0xA5 around every
    destination."""

    def __init__(self, eng, sources, pages, pieces, mem):
        self.eng, self.mem = eng, mem
        self.sources, self.pages, self.pieces = [bytes(s) for s in sources], list(pages), list(pieces)
        dev = mem == E.MEM_DEVICE
        lead = 0 if dev else 3
        self.soff, self.doff = [], []
        so = do = 16
        for s in self.sources:
            self.soff.append(so + lead)
            so += (len(s) + 31) & ~15
        for _, _, n in self.pages:
            self.doff.append(do + GUARD + lead)
            do += GUARD + ((n + 31) & ~15)
        src = np.zeros(so + 16, np.uint8)
        for s, o in zip(self.sources, self.soff):
            src[o:o + len(s)] = np.frombuffer(s, np.uint8)
        self.fill = np.full(do + GUARD, 0xA5, np.uint8)
        if dev:
            self.sbuf, self.dbuf = eng.alloc(src.size), eng.alloc(self.fill.size)
            self.sbuf.upload(src)
            self.dbuf.upload(self.fill)
            sp, dp = self.sbuf.ptr, self.dbuf.ptr
            assert sp % 16 == 0 and dp % 16 == 0
        else:
            self.src, self.dst = src, self.fill.copy()
            sp, dp = src.ctypes.data, self.dst.ctypes.data
        self.gs = (E.jfsx_gsrc * max(len(self.sources), 1))()
        for i, s in enumerate(self.sources):
            self.gs[i].data, self.gs[i].len = (sp + self.soff[i] if len(s) else None), len(s)
        self.gd = (E.jfsx_gdst * max(len(self.pages), 1))()
        for j, (first, count, n) in enumerate(self.pages):
            self.gd[j].data, self.gd[j].len = (dp + self.doff[j] if n else None), n
            self.gd[j].piece_first, self.gd[j].piece_count = first, count
        self.pa, self.n_piece = E.make_pieces(self.pieces)

    def run(self):
        self.eng.gather_batch(len(self.sources), self.gs, len(self.pages), self.gd, self.n_piece, self.pa, self.mem)
        return self

    def check(self):
        if self.mem == E.MEM_DEVICE:
            got = self.dbuf.download()
        else:
            got = self.dst
        at = 0
        for o, w in zip(self.doff, CM.gather_want(self.sources, self.pages, self.pieces)):
            assert (got[at:o] == 0xA5).all(), "guard in front of a page"
            assert np.array_equal(got[o:o + w.size], w)
            at = o + w.size
        assert (got[at:] == 0xA5).all(), "guard behind the last page"
        if self.mem == E.MEM_DEVICE:
            self.sbuf.free()
            self.dbuf.free()


@pytest.mark.parametrize("mem", MEMS, ids=MEM_IDS)
def test_alignment_matrix(eng, mem):
    """All 16 x 16 pairs of (src_off mod 16, destination offset mod 16) x the
    piece lengths, packed into a few pages of one call."""
    sources = [_rand(0x6A70 + i, 1024 + 16 + 4097) for i in range(2)]
    pages, pieces = CM.alignment_matrix(CM.MATRIX_LENGTHS, len(sources[0]), 300007)
    assert len(pages) == 4 and CM.matrix_seen(pages, pieces) == CM.matrix_full(CM.MATRIX_LENGTHS)
    GBatch(eng, sources, pages, pieces, mem).run().check()


@pytest.mark.parametrize("mem", MEMS, ids=MEM_IDS)
def test_single_piece_pages(eng, mem):
    lens = [0, 1, 13, 15, 16, 17, 4095, 32767, 32768, 32769, 65536 + 5, 1 << 20]
    sources = [_rand(0x6A80, (1 << 20) + 1)]
    pages, pieces = [], []
    for so in (0, 1):
        for n in lens:
            pages.append((len(pieces), 1 if n else 0, n))
            if n:
                pieces.append((0, so, n))
    GBatch(eng, sources, pages, pieces, mem).run().check()


@pytest.mark.parametrize("mem", MEMS, ids=MEM_IDS)
def test_tile_boundaries(eng, mem):
    """A page of three tiles + 5 bytes with piece boundaries at k T - 1, k T and
    k T + 1: data next to data, data next to a hole."""
    sources = [_rand(0x6A90, 4 * T)]
    cuts = sorted({k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)} | {0, 3 * T + 5})
    for holes in (lambda i: False, lambda i: i % 3 == 2, lambda i: i % 2 == 0):
        pieces = [(-1 if holes(i) else 0, 17 * i + 1, b - a) for i, (a, b) in enumerate(zip(cuts, cuts[1:]))]
        GBatch(eng, sources, [(0, len(pieces), 3 * T + 5)], pieces, mem).run().check()


@pytest.mark.parametrize("mem", MEMS, ids=MEM_IDS)
def test_piece_list_shapes(eng, mem):
    sources = [_rand(0x6AA0, 5000), _rand(0x6AA1, 100)]
    # 4096 one-byte pieces cycling through two sources and a hole
    pieces = [((k % 3) - 1, k % 97, 1) for k in range(4096)]
    pages = [(0, 4096, 4096)]
    # an all-hole page
    pages.append((len(pieces), 2, 4097))
    pieces += [(-1, 0, 1000), (-1, 0, 3097)]
    # the same source range read twice, by one page and by the next
    pages.append((len(pieces), 2, 6000))
    pieces += [(0, 5, 3000), (0, 5, 3000)]
    pages.append((len(pieces), 1, 3000))
    pieces += [(0, 5, 3000)]
    GBatch(eng, sources, pages, pieces, mem).run().check()


def test_engine_gather_applies_a_plan(eng):
    """Engine.gather on what Engine.compact_plan returns is the byte model of Compact."""
    rng = np.random.default_rng(0x6AC)
    slices, data = CM.seeded_slices(rng, 4096, 9)
    srcs, pages, pieces = eng.compact_plan(4096, slices)
    assert (srcs, pages, pieces) == CM.plan(4096, slices)
    blocks = CM.slice_blocks(data, 4096)
    got = eng.gather([blocks[(sid, indx)] for sid, indx, _ in srcs], pages, pieces)
    assert got == CM.compact_bytes(slices, data, 4096)


@pytest.mark.parametrize("mem", MEMS, ids=MEM_IDS)
def test_batch_sizes_grow_and_shrink(eng, mem):
    """1 ... 257 destinations in one call, growing and then shrinking: the
    engine's buffers are grow-only and every call sizes its own launch."""
    sources = [_rand(0x6AB0, 3000), _rand(0x6AB1, 777)]
    for n in (1, 2, 3, 16, 64, 257, 65, 4, 1):
        pages, pieces = [], []
        for j in range(n):
            a, b, h = 1 + (37 * j) % 1500, 1 + (53 * j) % 700, (11 * j) % 40
            run = [(0, j % 1400, a)] + ([(-1, 0, h)] if h else []) + [(1, j % 70, b)]
            pages.append((len(pieces), len(run), a + h + b))
            pieces += run
        GBatch(eng, sources, pages, pieces, mem).run().check()
