"""Checker for slice compaction (vfs.Compact, pkg/vfs/compact.go:54-109): a byte
model and a planner that share nothing with juicefs_amd/csrc/jfsx_compact.h.

  compact_bytes   the new slice as Compact writes it: b"".join of the slices'
                  ranges, zeros for id 0, cut into pages of block_size
  plan            sources, pages and canonical pieces, found byte by byte: every
                  byte of the new slice is labelled with the source block and
                  the offset it comes from, and the labels are run-length
                  encoded with a break at every page boundary
  apply_plan      a plan applied to the source blocks with numpy
  gather_want     jfsx_gather_batch's pages with numpy; alignment_matrix
                  builds the piece list its tests share, matrix_seen says which
                  (source residue, in-page destination residue, length) it holds

Slices are (id, size, off, len) tuples in Compact's order; `data` maps an id to
the bytes of its whole slice."""
import numpy as np


def slice_blocks(data, block_size):
    """{(id, indx): stored block} of every slice in data, as wSlice cuts them."""
    return {(sid, i // block_size): b[i:i + block_size] for sid, b in data.items()
            for i in range(0, len(b), block_size)}


def compact_bytes(slices, data, block_size):
    buf = b"".join(bytes(ln) if sid == 0 else data[sid][off:off + ln] for sid, _, off, ln in slices)
    assert all(sid == 0 or len(data[sid][off:off + ln]) == ln for sid, _, off, ln in slices)
    return [buf[i:i + block_size] for i in range(0, len(buf), block_size)]


def plan(block_size, slices):
    """-> (sources [(id, indx, bsize)], pages [(piece_first, piece_count, len)],
    pieces [(src, src_off, len)]), src -1 for zeros."""
    sources, index = [], {}
    src_of, off_of = [], []
    for sid, size, off, ln in slices:
        p = np.arange(off, off + ln, dtype=np.int64)
        if sid == 0:
            src_of.append(np.full(ln, -1, np.int64))
            off_of.append(np.zeros(ln, np.int64))
            continue
        indx = p // block_size
        for i in range(int(indx[0]), int(indx[-1]) + 1):
            if (sid, i) not in index:
                index[(sid, i)] = len(sources)
                sources.append((sid, i, min(block_size, size - i * block_size)))
        lut = np.array([index[(sid, i)] for i in range(int(indx[0]), int(indx[-1]) + 1)], np.int64)
        src_of.append(lut[indx - indx[0]])
        off_of.append(p % block_size)
    if not src_of:
        return [], [], []
    s, o = np.concatenate(src_of), np.concatenate(off_of)
    pos = np.arange(s.size, dtype=np.int64)
    brk = np.ones(s.size, bool)
    brk[1:] = (s[1:] != s[:-1]) | ((s[1:] >= 0) & (o[1:] != o[:-1] + 1)) | (pos[1:] % block_size == 0)
    starts = np.flatnonzero(brk)
    ends = np.append(starts[1:], s.size)
    pieces = [(int(s[a]), int(o[a]), int(b - a)) for a, b in zip(starts, ends)]
    pages = []
    for first in range(0, s.size, block_size):
        last = min(first + block_size, s.size)
        k0 = int(np.searchsorted(starts, first))
        k1 = int(np.searchsorted(starts, last))
        pages.append((k0, k1 - k0, last - first))
    return sources, pages, pieces


def apply_plan(sources, pages, pieces, blocks):
    """blocks: {(id, indx): bytes}.  -> the pages."""
    out = []
    for first, count, ln in pages:
        parts = []
        for src, off, n in pieces[first:first + count]:
            if src < 0:
                parts.append(np.zeros(n, np.uint8))
            else:
                sid, indx, bsize = sources[src]
                b = np.frombuffer(blocks[(sid, indx)], np.uint8)
                assert b.size == bsize and off + n <= bsize
                parts.append(b[off:off + n])
        page = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        assert page.size == ln
        out.append(page.tobytes())
    return out


def seeded_slices(rng, block_size, n, max_blocks=3):
    """A slice list with holes at the head, middle and tail, ids that repeat,
    ranges that end on and one byte beside block boundaries, and a single-byte
    slice.  -> (slices, data)."""
    data, sizes, slices = {}, {}, []

    def hole(ln):
        slices.append((0, ln, 0, ln))

    def live(sid, off, ln):
        slices.append((sid, sizes[sid], off, ln))

    for sid in range(1, n + 1):
        sizes[sid] = int(rng.integers(1, max_blocks * block_size + 2))
        data[sid] = rng.integers(0, 256, sizes[sid], dtype=np.uint8).tobytes()
    hole(int(rng.integers(1, block_size + 2)))
    for sid in range(1, n + 1):
        size = sizes[sid]
        kind = int(rng.integers(0, 6))
        if kind == 0 or size < 3:
            live(sid, 0, size)
        elif kind == 1:  # ends on a block boundary
            end = min(size, block_size * max(1, size // block_size))
            off = int(rng.integers(0, end))
            live(sid, off, end - off)
        elif kind == 2:  # one byte beside a block boundary
            end = min(size, block_size * max(1, size // block_size) + int(rng.choice([-1, 1])))
            end = max(end, 1)
            off = int(rng.integers(0, end))
            live(sid, off, end - off)
        elif kind == 3:  # the same id in two records that touch one block
            a = int(rng.integers(1, size))
            live(sid, 0, a)
            hole(int(rng.integers(1, 40)))
            off = int(rng.integers(0, size))
            live(sid, off, int(rng.integers(1, size - off + 1)))
        elif kind == 4:
            off = int(rng.integers(0, size))
            live(sid, off, 1)
        else:
            off = int(rng.integers(0, size))
            live(sid, off, int(rng.integers(1, size - off + 1)))
        if rng.integers(0, 4) == 0:
            hole(int(rng.integers(1, 2 * block_size)))
    hole(int(rng.integers(1, block_size)))
    return slices, data


MATRIX_LENGTHS = [1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 4097]


def alignment_matrix(lengths, source_len, page_len):
    """All 16 x 16 pairs of (src_off mod 16, destination offset in its page mod
    16) x piece lengths, packed into pages of page_len (the last shorter).  The
    destination residue is steered by a hole of 1..16 bytes in front of each
    data piece; a data piece that would not fit with its hole goes to the next
    page, and a hole fills what is left of this one, so no data piece is cut
    and every residue is the one in its own page.  Sources are 16-byte aligned,
    so src_off mod 16 is the source address's.  -> (pages, pieces)"""
    pages, pieces, first, dst = [], [], 0, 0
    for so in range(16):
        for dr in range(16):
            for k, ln in enumerate(lengths):
                hole = (dr - dst - 1) % 16 + 1
                if dst + hole + ln > page_len:
                    if dst < page_len:
                        pieces.append((-1, 0, page_len - dst))
                    pages.append((first, len(pieces) - first, page_len))
                    first, dst = len(pieces), 0
                    hole = (dr - 1) % 16 + 1
                pieces.append((-1, 0, hole))
                base = (7 * so + 13 * dr + 29 * k) % 64 * 16  # spread over the source, residue so
                assert base + so + ln <= source_len and dst + hole + ln <= page_len
                pieces.append((so & 1, base + so, ln))
                dst += hole + ln
    pages.append((first, len(pieces) - first, dst))
    return pages, pieces


def matrix_seen(pages, pieces):
    """{(src_off mod 16, destination offset in the page mod 16, len)} of the data pieces."""
    seen = set()
    for first, count, _ in pages:
        at = 0
        for s, o, ln in pieces[first:first + count]:
            if s >= 0:
                seen.add((o % 16, at % 16, ln))
            at += ln
    return seen


def matrix_full(lengths):
    return {(so, dr, ln) for so in range(16) for dr in range(16) for ln in lengths}


def gather_want(sources, pages, pieces):
    """jfsx_gather_batch's pages with numpy: sources are bytes, pages
    (piece_first, piece_count, len), pieces (src, src_off, len)."""
    out = []
    for first, count, n in pages:
        parts = [np.zeros(ln, np.uint8) if s < 0 else np.frombuffer(sources[s], np.uint8)[o:o + ln]
                 for s, o, ln in pieces[first:first + count]]
        page = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        assert page.size == n
        out.append(page)
    return out
