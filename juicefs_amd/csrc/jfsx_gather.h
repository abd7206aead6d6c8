// jfsx_gather.h -- the arithmetic of jfsx_gather_batch that both sides run: how
// a lane of gather_pages_k (jfsx_gather.hip) finds the page of its tile and the
// piece of its chunk, and how it builds a 16-byte destination chunk from the
// one or two aligned 16-byte source chunks it overlaps.  The host build
// (tests/harness/compact_host.cpp) runs the same functions lane by lane.
//
// The kernel is destination-centric.  A page of `len` bytes is cut into tiles
// of kTile bytes; a workgroup of kThreads lanes owns one tile at a time and
// covers it in kPasses passes of kThreads chunks of 16 bytes, lane l taking
// chunk l of each pass, so that every destination byte has exactly one writer
// and a wave's stores are contiguous.  The host resolves the caller's pieces
// to {source address or null, dst_off, len} per page, in dst_off order, with
// the lengths summing to the page's.
//   a chunk inside one data piece   the aligned source chunk at sp - a, a =
//                                   sp mod 16, and for a != 0 the next one,
//                                   funnel-shifted by a bytes; one 16-byte store
//   a chunk inside one hole         one 16-byte store of zeros
//   a chunk that straddles pieces,  byte by byte: only bytes of the pieces are
//   or the page's last partial one  loaded, only bytes below len are stored
// Loads therefore stay inside the aligned 16-byte chunks that overlap a
// piece's source bytes, and stores inside [dst, dst + len).
//
// Every access to a source or a destination goes through a policy `Mem` with
// ld16 / st16 (an aligned 16-byte chunk) and ld8 / st8 (one byte).  The
// addresses come out of GPiece / GPage in memory, so the compiler cannot tell
// their address space: the kernel's policy casts them to global memory, which
// turns flat loads and stores into global ones; the host harness's policy
// checks every address against the contract.
#pragma once
#include <stdint.h>

#ifndef JFSX_HD
#define JFSX_HD static inline
#endif

namespace jfsx_gather {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kChunk = 16;
constexpr uint32_t kTile = 16384;  // bytes of a page one workgroup owns at a time (engine.GATHER_TILE)
constexpr uint32_t kPasses = kTile / (kThreads * kChunk);
static_assert(kPasses * kThreads * kChunk == kTile, "a tile is whole passes");

struct alignas(16) U4 {
    uint32_t x, y, z, w;
};

struct GPiece {
    const uint8_t *src;  // the piece's first source byte; null: zeros
    uint64_t dst_off;    // in its page
    uint64_t len;        // > 0
};

struct GPage {
    uint8_t *dst;         // 16-byte aligned
    uint64_t len;         // > 0: empty pages are not launched
    uint64_t tile_first;  // tiles of the pages in front
    uint32_t piece_first, piece_count;
};

JFSX_HD uint64_t tiles_of(uint64_t len) { return (len + kTile - 1) / kTile; }

// the page that owns `tile`: the last one with tile_first <= tile
JFSX_HD uint32_t find_page(const GPage *pages, uint32_t n_pages, uint64_t tile) {
    uint32_t lo = 0, hi = n_pages;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pages[mid].tile_first <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the piece that holds byte `off` of the page: the last one with dst_off <= off
JFSX_HD uint32_t find_piece(const GPiece *pp, uint32_t count, uint64_t off) {
    uint32_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (pp[mid].dst_off <= off) lo = mid;
        else hi = mid;
    }
    return lo;
}

JFSX_HD uint32_t sel4(uint32_t q, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return q == 0 ? a : q == 1 ? b : q == 2 ? c : d;
}

JFSX_HD uint32_t shr_pair(uint32_t lo, uint32_t hi, uint32_t bits) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> bits);
}

// bytes [a, a + 16) of the 32 bytes lo | hi, 0 < a < 16 (little-endian words)
JFSX_HD U4 funnel(U4 lo, U4 hi, uint32_t a) {
    const uint32_t q = a >> 2, r = (a & 3) * 8;
    const uint32_t v0 = sel4(q, lo.x, lo.y, lo.z, lo.w), v1 = sel4(q, lo.y, lo.z, lo.w, hi.x),
                   v2 = sel4(q, lo.z, lo.w, hi.x, hi.y), v3 = sel4(q, lo.w, hi.x, hi.y, hi.z),
                   v4 = sel4(q, hi.x, hi.y, hi.z, hi.w);
    return U4{shr_pair(v0, v1, r), shr_pair(v1, v2, r), shr_pair(v2, v3, r), shr_pair(v3, v4, r)};
}

// One chunk: dst[off, min(off + 16, len)), off a multiple of 16 below len.  p
// is the lane's piece cursor: on entry some piece at or in front of the one
// that holds off, on return the one that holds off.
template <class Mem>
JFSX_HD void gather_chunk(const GPiece *pp, uint32_t count, uint32_t &p, uint8_t *dst, uint64_t len, uint64_t off,
                          Mem &m) {
    if (pp[p].dst_off + pp[p].len <= off) {  // consecutive chunks mostly share a piece; else search what is left
        p += 1;
        p += find_piece(pp + p, count - p, off);
    }
    const GPiece g = pp[p];
    if (off + kChunk <= g.dst_off + g.len) {
        U4 v{0, 0, 0, 0};
        if (g.src) {
            const uint8_t *sp = g.src + (off - g.dst_off);
            const uint32_t a = (uint32_t)((uintptr_t)sp & (kChunk - 1));
            v = m.ld16(sp - a);
            if (a) v = funnel(v, m.ld16(sp - a + kChunk), a);
        }
        m.st16(dst + off, v);
        return;
    }
    const uint64_t stop = off + kChunk < len ? off + kChunk : len;
    uint32_t q = p;
    for (uint64_t o = off; o < stop; o++) {
        while (pp[q].dst_off + pp[q].len <= o) q++;
        m.st8(dst + o, pp[q].src ? m.ld8(pp[q].src + (o - pp[q].dst_off)) : (uint8_t)0);
    }
}

// everything lane `lane` of the workgroup that owns `tile` does
template <class Mem>
JFSX_HD void gather_lane(const GPage *pages, uint32_t n_pages, const GPiece *pieces, uint64_t tile, uint32_t lane,
                         Mem &m) {
    const GPage pg = pages[find_page(pages, n_pages, tile)];
    const GPiece *pp = pieces + pg.piece_first;
    uint64_t off = (tile - pg.tile_first) * kTile + (uint64_t)lane * kChunk;
    if (off >= pg.len) return;
    uint32_t p = find_piece(pp, pg.piece_count, off);
    for (uint32_t k = 0; k < kPasses && off < pg.len; k++, off += kThreads * kChunk)
        gather_chunk(pp, pg.piece_count, p, pg.dst, pg.len, off, m);
}

}  // namespace jfsx_gather
