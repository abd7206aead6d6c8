// Host harness over juicefs_amd/csrc/jfsx_compact.h and jfsx_gather.h
// (tests/test_compact_plan.py): the planner of jfsx_compact_plan as g++ builds
// it, gather_pages_k's per-lane arithmetic run lane by lane over every tile
// with a loader that checks each load against the contract, and the layouts
// of the compaction records as the C compiler sees include/jfsx.h.  Built as a
// shared library for the test and, with its main, as a stand-alone program
// that runs an alignment matrix and the reference's TestCompact shape against
// memcpy (the sanitizer build).
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../juicefs_amd/csrc/jfsx_compact.h"
#include "../../juicefs_amd/csrc/jfsx_gather.h"

namespace {

using jfsx_gather::GPage;
using jfsx_gather::GPiece;
using jfsx_gather::U4;

struct Resolved {
    std::vector<GPage> pages;
    std::vector<GPiece> pieces;
    uint64_t tiles = 0;
};

// as the engine resolves a call's records (gather_enqueue, jfsx_api.cpp)
Resolved resolve(const jfsx_gsrc *src, int n_dst, const jfsx_gdst *dst, const jfsx_piece *pieces) {
    Resolved r;
    for (int j = 0; j < n_dst; j++) {
        if (!dst[j].len) continue;
        GPage g{};
        g.dst = (uint8_t *)dst[j].data;
        g.len = dst[j].len;
        g.tile_first = r.tiles;
        g.piece_first = (uint32_t)r.pieces.size();
        g.piece_count = dst[j].piece_count;
        uint64_t off = 0;
        for (uint32_t k = 0; k < dst[j].piece_count; k++) {
            const jfsx_piece &p = pieces[dst[j].piece_first + k];
            r.pieces.push_back(GPiece{p.src < 0 ? nullptr : (const uint8_t *)src[p.src].data + p.src_off, off, p.len});
            off += p.len;
        }
        r.tiles += jfsx_gather::tiles_of(dst[j].len);
        r.pages.push_back(g);
    }
    return r;
}

}  // namespace

extern "C" {

// sizeof and field offsets of the six records, in declaration order
int compact_layout(uint64_t *out, int cap) {
    const uint64_t v[] = {
        sizeof(jfsx_slice), offsetof(jfsx_slice, id), offsetof(jfsx_slice, size), offsetof(jfsx_slice, off),
        offsetof(jfsx_slice, len), offsetof(jfsx_slice, reserved),
        sizeof(jfsx_csrc), offsetof(jfsx_csrc, id), offsetof(jfsx_csrc, indx), offsetof(jfsx_csrc, bsize),
        sizeof(jfsx_cpage), offsetof(jfsx_cpage, piece_first), offsetof(jfsx_cpage, piece_count),
        offsetof(jfsx_cpage, src_bad), offsetof(jfsx_cpage, reserved),
        sizeof(jfsx_piece), offsetof(jfsx_piece, src), offsetof(jfsx_piece, reserved), offsetof(jfsx_piece, src_off),
        offsetof(jfsx_piece, len),
        sizeof(jfsx_gsrc), offsetof(jfsx_gsrc, data), offsetof(jfsx_gsrc, len),
        sizeof(jfsx_gdst), offsetof(jfsx_gdst, data), offsetof(jfsx_gdst, len), offsetof(jfsx_gdst, piece_first),
        offsetof(jfsx_gdst, piece_count),
    };
    const int n = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < n && i < cap; i++) out[i] = v[i];
    return n;
}

int compact_constants(int *out) {
    out[0] = (int)jfsx_gather::kTile;
    out[1] = (int)jfsx_gather::kThreads;
    out[2] = (int)jfsx_gather::kChunk;
    out[3] = JFSX_ESRC;
    out[4] = JFSX_ABI_VERSION;
    return 5;
}

// the planner of the header, with jfsx_compact_plan's calling convention
int compact_plan_host(uint32_t block_size, int n, const jfsx_slice *slices, int src_cap, jfsx_csrc *srcs, int *n_src,
                      int page_cap, jfsx_cpage *pages, uint64_t *page_len, int *n_page, int piece_cap,
                      jfsx_piece *pieces, int *n_piece) {
    jfsx_compact::Plan p;
    const int rc = jfsx_compact::plan(block_size, n, slices, p);
    if (rc) return rc;
    *n_src = (int)p.srcs.size();
    *n_page = (int)p.pages.size();
    *n_piece = (int)p.pieces.size();
    if (*n_src > src_cap || *n_page > page_cap || *n_piece > piece_cap) return JFSX_ENOMEM;
    std::copy(p.srcs.begin(), p.srcs.end(), srcs);
    std::copy(p.pages.begin(), p.pages.end(), pages);
    std::copy(p.page_len.begin(), p.page_len.end(), page_len);
    std::copy(p.pieces.begin(), p.pieces.end(), pieces);
    return 0;
}

// gather_pages_k lane by lane: every tile, every lane of its workgroup.  The
// records have passed the engine's checks; sources and destinations are
// 16-byte aligned, and the memory of every aligned 16-byte chunk that overlaps
// a source is readable.  Returns the number of accesses that broke the
// contract: a 16-byte load or store at an address that is not 16-byte aligned,
// a loaded chunk that overlaps no piece's source bytes of the lane's page, a
// loaded byte outside them, a store that leaves [dst, dst + len) of the page.
// n_loads counts the 16-byte loads.
uint64_t gather_host(const jfsx_gsrc *src, int n_dst, const jfsx_gdst *dst, const jfsx_piece *pieces,
                     uint64_t *n_loads) {
    const Resolved r = resolve(src, n_dst, dst, pieces);
    uint64_t bad = 0, loads = 0;
    for (uint64_t tile = 0; tile < r.tiles; tile++) {
        const GPage &pg = r.pages[jfsx_gather::find_page(r.pages.data(), (uint32_t)r.pages.size(), tile)];
        struct CheckedMem {
            const Resolved &r;
            const GPage &pg;
            uint64_t &bad, &loads;
            bool in_piece(const uint8_t *q, size_t n) const {  // [q, q + n) overlaps a piece's source bytes
                for (uint32_t k = 0; k < pg.piece_count; k++) {
                    const GPiece &g = r.pieces[pg.piece_first + k];
                    if (g.src && q < g.src + g.len && q + n > g.src) return true;
                }
                return false;
            }
            bool in_page(const uint8_t *q, size_t n) const { return q >= pg.dst && q + n <= pg.dst + pg.len; }
            U4 ld16(const uint8_t *q) {
                loads++;
                if (((uintptr_t)q & 15) || !in_piece(q, 16)) bad++;
                U4 v;
                memcpy(&v, q, 16);
                return v;
            }
            void st16(uint8_t *q, U4 v) {
                if (((uintptr_t)q & 15) || !in_page(q, 16)) bad++;
                else memcpy(q, &v, 16);
            }
            uint8_t ld8(const uint8_t *q) {
                if (!in_piece(q, 1)) bad++;
                return *q;
            }
            void st8(uint8_t *q, uint8_t v) {
                if (!in_page(q, 1)) bad++;
                else *q = v;
            }
        } m{r, pg, bad, loads};
        for (uint32_t lane = 0; lane < jfsx_gather::kThreads; lane++)
            jfsx_gather::gather_lane(r.pages.data(), (uint32_t)r.pages.size(), r.pieces.data(), tile, lane, m);
    }
    if (n_loads) *n_loads = loads;
    return bad;
}

}  // extern "C"

namespace {

struct Buf {  // len bytes at a 16-byte aligned address, whole chunks readable, guards around
    uint8_t *base;
    uint8_t *p;
    size_t len;
    explicit Buf(size_t n) : len(n) {
        const size_t body = (n + 15) & ~(size_t)15;
        base = (uint8_t *)aligned_alloc(16, body + 32);
        memset(base, 0xA5, body + 32);
        p = base + 16;
    }
    ~Buf() { free(base); }
    bool guards_ok() const {
        for (size_t i = 0; i < 16; i++)
            if (base[i] != 0xA5) return false;
        const size_t body = (len + 15) & ~(size_t)15;
        for (size_t i = len; i < body + 16; i++)
            if (p[i] != 0xA5) return false;
        return true;
    }
};

int fail(const char *what, long a, long b, long c) {
    printf("compact_host FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
    return 1;
}

}  // namespace

int main() {
    // 1. the alignment matrix: (src_off mod 16, destination offset mod 16) x lengths, one page per case
    const size_t lens[] = {1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 4097, 16384 + 7, 40000};
    Buf source(50000);
    for (size_t i = 0; i < source.len; i++) source.p[i] = (uint8_t)(i * 131 + (i >> 8) * 7 + 1);
    for (size_t so = 0; so < 16; so++)
        for (size_t dr = 0; dr < 16; dr++)
            for (size_t len : lens) {
                const size_t hole = dr;  // steers the destination residue
                std::vector<jfsx_piece> pc;
                if (hole) pc.push_back(jfsx_piece{-1, 0, 0, hole});
                pc.push_back(jfsx_piece{0, 0, so + 3, len});
                pc.push_back(jfsx_piece{-1, 0, 0, 5});
                pc.push_back(jfsx_piece{0, 0, so, 9});
                const size_t total = hole + len + 5 + 9;
                Buf page(total);
                const jfsx_gsrc gs{source.p, source.len};
                jfsx_gdst gd{page.p, total, 0, (uint32_t)pc.size()};
                uint64_t loads = 0;
                if (gather_host(&gs, 1, &gd, pc.data(), &loads)) return fail("load outside a piece", so, dr, len);
                std::vector<uint8_t> want(total, 0);
                memcpy(want.data() + hole, source.p + so + 3, len);
                memcpy(want.data() + hole + len + 5, source.p + so, 9);
                if (memcmp(want.data(), page.p, total)) return fail("bytes", so, dr, len);
                if (!page.guards_ok()) return fail("guard", so, dr, len);
            }
    // 2. the reference's TestCompact shape through the planner and the gather
    {
        std::vector<jfsx_slice> sl;
        for (uint32_t i = 0; i < 100; i++) sl.push_back(jfsx_slice{i, 100 + 100 * i, 0, 100 + 100 * i, 0});
        jfsx_compact::Plan p;
        if (jfsx_compact::plan(256 << 10, (int)sl.size(), sl.data(), p)) return fail("plan", 0, 0, 0);
        if (p.srcs.size() != 99 || p.pieces.size() != 101 || p.pages.size() != 2)
            return fail("plan counts", p.srcs.size(), p.pieces.size(), p.pages.size());
        if (p.pages[0].piece_count != 72 || p.page_len[0] != 262144 || p.pages[1].piece_count != 29 ||
            p.page_len[1] != 242856)
            return fail("plan pages", p.pages[0].piece_count, p.page_len[0], p.page_len[1]);
        std::vector<Buf *> blocks;
        std::vector<jfsx_gsrc> gs;
        for (const jfsx_csrc &s : p.srcs) {
            Buf *b = new Buf(s.bsize);
            for (size_t i = 0; i < b->len; i++) b->p[i] = (uint8_t)(s.id * 31 + i);
            blocks.push_back(b);
            gs.push_back(jfsx_gsrc{b->p, b->len});
        }
        Buf p0(p.page_len[0]), p1(p.page_len[1]);
        jfsx_gdst gd[2] = {{p0.p, p.page_len[0], p.pages[0].piece_first, p.pages[0].piece_count},
                           {p1.p, p.page_len[1], p.pages[1].piece_first, p.pages[1].piece_count}};
        if (gather_host(gs.data(), 2, gd, p.pieces.data(), nullptr)) return fail("load outside a piece", -1, 0, 0);
        std::vector<uint8_t> want;
        for (const jfsx_slice &s : sl)
            for (uint32_t i = 0; i < s.len; i++) want.push_back(s.id ? (uint8_t)(s.id * 31 + i) : 0);
        if (memcmp(want.data(), p0.p, p0.len) || memcmp(want.data() + p0.len, p1.p, p1.len))
            return fail("compacted bytes", 0, 0, 0);
        if (!p0.guards_ok() || !p1.guards_ok()) return fail("guard", -1, 0, 0);
        for (Buf *b : blocks) delete b;
    }
    // 3. the planner's argument errors
    {
        jfsx_compact::Plan p;
        const jfsx_slice ok{1, 10, 0, 10, 0}, zero{1, 10, 0, 0, 0}, past{1, 10, 5, 6, 0}, res{1, 10, 0, 10, 1};
        const jfsx_slice big[2] = {{0, 0, 0, 0xFFFFFFFFu, 0}, {0, 0, 0, 1, 0}};
        if (jfsx_compact::plan(0, 1, &ok, p) != JFSX_EINVAL || jfsx_compact::plan(8, 1, &zero, p) != JFSX_EINVAL ||
            jfsx_compact::plan(8, 1, &past, p) != JFSX_EINVAL || jfsx_compact::plan(8, 1, &res, p) != JFSX_EINVAL ||
            jfsx_compact::plan(1u << 30, 2, big, p) != JFSX_EINVAL || jfsx_compact::plan(1, 1, big, p) != JFSX_ENOMEM ||
            jfsx_compact::plan(8, 1, &ok, p) != 0)
            return fail("plan errors", 0, 0, 0);
    }
    printf("compact_host ok\n");
    return 0;
}
