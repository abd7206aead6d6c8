// jfsx_compact.h -- the planner of jfsx_compact_plan: from the slice list
// vfs.Compact receives (pkg/vfs/compact.go:54-109) to the stored blocks it
// reads, the pages of the new slice and the pieces each page is assembled
// from.  Plain C++ without a device, so that the host harness
// (tests/harness/compact_host.cpp) builds it with g++.
//
// The new slice is the concatenation of the slices' ranges [off, off + len),
// zeros for a slice with id 0, cut into pages of block_size.  A range of slice
// id is read block by block as rSlice.ReadAt does (cached_store.go:96-190):
// byte p lies in block indx = p / block_size, whose stored length is
// bsize = min(block_size, size - indx * block_size) (:65-71).  A piece ends at
// the first of: the end of its range, of its source block, of its page.
// Neighbours in one page that continue each other are merged, which makes the
// piece list canonical: one slice list has one plan.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "../../include/jfsx.h"

namespace jfsx_compact {

struct Plan {
    std::vector<jfsx_csrc> srcs;
    std::vector<jfsx_cpage> pages;
    std::vector<uint64_t> page_len;
    std::vector<jfsx_piece> pieces;
};

// 0, or JFSX_EINVAL / JFSX_ENOMEM with `out` in an unspecified state
inline int plan(uint32_t block_size, int n, const jfsx_slice *slices, Plan &out) {
    if (block_size == 0 || n < 0 || (n > 0 && !slices)) return JFSX_EINVAL;
    uint64_t total = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_slice &s = slices[i];
        if (s.reserved || s.len == 0) return JFSX_EINVAL;
        if (s.id != 0 && (uint64_t)s.off + s.len > s.size) return JFSX_EINVAL;
        total += s.len;
        if (total > 0xFFFFFFFFull) return JFSX_EINVAL;
    }
    // the page count is known before anything is built: one that no int holds needs no attempt
    if ((total + block_size - 1) / block_size > 0x7FFFFFFFull) return JFSX_ENOMEM;
    out = Plan();
    std::map<std::pair<uint64_t, uint32_t>, int32_t> seen;  // (id, indx) -> source
    uint64_t pos = 0;                                       // in the new slice
    for (int i = 0; i < n; i++) {
        const jfsx_slice &s = slices[i];
        uint64_t p = s.off, left = s.len;
        while (left) {
            const uint64_t in_page = pos % block_size;
            uint64_t take = std::min<uint64_t>(left, block_size - in_page);
            jfsx_piece pc{};
            pc.src = -1;
            if (s.id != 0) {
                const uint32_t indx = (uint32_t)(p / block_size);
                const uint64_t in_blk = p % block_size;
                const uint32_t bsize = (uint32_t)std::min<uint64_t>(block_size, s.size - (uint64_t)indx * block_size);
                take = std::min<uint64_t>(take, bsize - in_blk);
                auto it = seen.find({s.id, indx});
                if (it == seen.end()) {
                    it = seen.emplace(std::make_pair(s.id, indx), (int32_t)out.srcs.size()).first;
                    out.srcs.push_back(jfsx_csrc{s.id, indx, bsize});
                }
                pc.src = it->second;
                pc.src_off = in_blk;
            }
            pc.len = take;
            if (in_page == 0) {
                out.pages.push_back(jfsx_cpage{(uint32_t)out.pieces.size(), 0, -1, 0});
                out.page_len.push_back(0);
            }
            jfsx_cpage &pg = out.pages.back();
            jfsx_piece *prev = pg.piece_count ? &out.pieces.back() : nullptr;
            if (prev && prev->src == pc.src && (pc.src < 0 || prev->src_off + prev->len == pc.src_off)) {
                prev->len += take;
            } else {
                out.pieces.push_back(pc);
                pg.piece_count++;
            }
            out.page_len.back() += take;
            pos += take;
            p += take;
            left -= take;
        }
    }
    return 0;
}

}  // namespace jfsx_compact
