// jfsx_crc.hip -- CRC32C per 32 KiB segment over ranges (gfx950), the Hadoop
// file checksum's kernels (CRC32C per 512-byte chunk, MD5 per DFS block), and
// the synthetic-input generator.
//
// crc32c_segments replaces the CRC loops of checksum() (pkg/chunk/disk_cache.go:
// 1218-1231) and of cacheFile.ReadAt (disk_cache.go:1315-1327) for cache hits,
// none-cipher volumes and the staging re-read (pkg/chunk/cached_store.go:961-971).
// One wave per 32 KiB segment, 64 lanes x 16 B per row, slice-by-16 tables in
// LDS; lane CRCs are shifted to the segment end (GF(2) multiply by x^(8d) mod P)
// and XOR-reduced across the wave.
#include "jfsx_dev.h"

#define JFSX_MD5_HD __host__ __device__ __forceinline__
#include "jfsx_md5.h"

namespace jfsx {

// Slice-by-16 reads 20 random table dwords per 16 B; with one copy of each
// table, 32 lanes of random bytes land on the 32 LDS banks with ~3.5-way
// conflicts and the kernel is LDS-bound near 4.2 TB/s.  Here the tables are
// the slice-by-4 byte tables U12..U15, each entry replicated 32x, one replica
// per bank, so lane l always reads bank l mod 32: conflict-free.  A v_perm
// builds each address in one VALU op (entry stride 256 B, two tables
// interleaved per 64 KiB: address = byte << 8 | 4 * (lane mod 32) |
// region << 16, with the region bytes carried in lb) -- 16 lookups and about
// 28 VALU per 16 B at 144 KiB of LDS (one 16-wave workgroup per CU).
// In whole segments a lane owns 64 contiguous bytes of every 4 KiB span, a
// chain of 16 slice-by-4 steps; two spans' chains run interleaved, and the
// lane CRC moves from span to span by one 4096-B shift, A' = S4096(A) ^
// crc_raw(0, chunk), through nibble tables (the tables are linear: T[b] =
// T[b & 15] ^ T[b & 240]) in region 2.  The guarded path (ragged segment
// ends) keeps 1 KiB rows and takes its 1024-B shift from global memory.
// Each workgroup stages the tables once per task (0.5 to 4 MiB) and every
// wave loops over segments.  6.03-6.05 TB/s at 64 GiB against 5.33 for the
// round-3 nibble-table kernel on the same box (profiles/r4/ab_crc.txt)
constexpr uint32_t kCrcWaves = 16;
constexpr uint32_t kCrcLds = 0x24000;  // 147456 B: byte tables 128 KiB + shift nibble tables 16 KiB

// the lane's 64-byte chunk of span r of a segment: piece j.  Instruction j
// loads the span's bytes 1024j + 16l (one fully coalesced 1 KiB row, 8 whole
// lines; with 64l + 16j each load would touch 32 cache lines, 32 B of each);
// after quad_xpose lane l = 4m + t holds the chunk at 64 (16t + m) of the
// span.  The loads carry the non-temporal hint (the data is read once; A/B
// in profiles/r4/ab_crc.txt)
__device__ __forceinline__ uint4 crc_chunk_ld(const uint8_t *seg, uint32_t lane, int r, int j) {
    return gld16_nt(seg + 4096 * r + 1024 * j + 16 * lane);
}
// lane chunk index within a span (the final shift to the segment end)
__device__ __forceinline__ uint32_t crc_chunk_idx(uint32_t lane) {
    return 16u * (lane & 3u) + (lane >> 2);
}
// 4 x 4 transpose of 16-byte pieces across the 4 lanes of a quad: afterwards
// v[i] of lane t is what v[t] of lane i held.  Two butterfly stages (lane bit
// 0, then bit 1), each a DPP quad swap of the piece the partner needs.
__device__ __forceinline__ uint32_t dpp_swap(uint32_t x, int ctrl) {
    return ctrl == 0xB1 ? (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, true)
                        : (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xF, 0xF, true);
}
__device__ __forceinline__ void xpose_stage(uint32_t &a, uint32_t &b, bool odd, int ctrl) {
    const uint32_t r = dpp_swap(odd ? a : b, ctrl);
    a = odd ? r : a;
    b = odd ? b : r;
}
__device__ __forceinline__ void quad_xpose(uint4 (&v)[4], uint32_t lane) {
    const bool o1 = lane & 1u, o2 = lane & 2u;
#define XS(f)                                 \
    xpose_stage(v[0].f, v[1].f, o1, 0xB1);    \
    xpose_stage(v[2].f, v[3].f, o1, 0xB1);    \
    xpose_stage(v[0].f, v[2].f, o2, 0x4E);    \
    xpose_stage(v[1].f, v[3].f, o2, 0x4E);
    XS(x) XS(y) XS(z) XS(w)
#undef XS
}
// byte k of x through U(12 + k): region k >> 1 (lb byte 2 = 1), half k & 1
#define BYT(x, k)                                                                                              \
    lds_u32(lds, __builtin_amdgcn_perm((x), lb, 0x0c000000u | ((k) >= 2 ? 0x00020000u : 0x000c0000u) |        \
                                                    ((4u + (k)) << 8)) +                                       \
                     ((k)&1) * 128u)
// 4096-B shift nibble tables in region 2 (lb byte 3 = 2)
#define NIBS(t, h, xm) lds_u32(lds, __builtin_amdgcn_perm((xm), lb, 0x0c030000u | ((4u + (t)) << 8)) + ((t)*4096u + (h)*128u))
#define X3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)
// one slice-by-4 step: crc_raw of the 4 bytes of x (= state ^ word)
__device__ __forceinline__ uint32_t crc_step4(const char *lds, uint32_t lb, uint32_t x) {
    return X3(BYT(x, 0), BYT(x, 1), BYT(x, 2)) ^ BYT(x, 3);
}
// crc_raw of the 4 bytes of x, XORed with w
__device__ __forceinline__ uint32_t crc_step4x(const char *lds, uint32_t lb, uint32_t x, uint32_t w) {
    return X3(X3(BYT(x, 0), BYT(x, 1), BYT(x, 2)), BYT(x, 3), w);
}
__device__ __forceinline__ uint32_t crc_shift4096(const char *lds, uint32_t lb, uint32_t A) {
    const uint32_t xl = A & 0x0f0f0f0fu, xh = (A >> 4) & 0x0f0f0f0fu;
    return X3(X3(NIBS(0, 0, xl), NIBS(0, 1, xh), NIBS(1, 0, xl)), X3(NIBS(1, 1, xh), NIBS(2, 0, xl), NIBS(2, 1, xh)),
              NIBS(3, 0, xl) ^ NIBS(3, 1, xh));
}
#undef X3
__device__ __forceinline__ uint32_t crc_u16_byte(const char *lds, uint32_t lb, uint4 p) {
    uint32_t c = crc_step4(lds, lb, p.x);
    c = crc_step4(lds, lb, c ^ p.y);
    c = crc_step4(lds, lb, c ^ p.z);
    return crc_step4(lds, lb, c ^ p.w);
}

// the guarded path's row step with the 1024-B shift from global byte tables
__device__ __forceinline__ uint32_t crc_row_g(const char *lds, const uint32_t *__restrict__ T, uint32_t lb, uint32_t A,
                                              uint4 p) {
    const uint32_t s = T[24 * 256 + (A & 0xffu)] ^ T[25 * 256 + ((A >> 8) & 0xffu)] ^
                       T[26 * 256 + ((A >> 16) & 0xffu)] ^ T[27 * 256 + (A >> 24)];
    return crc_u16_byte(lds, lb, p) ^ s;
}

// ragged tails (segment length not a multiple of 16 B: the last segment of an
// odd-sized block only) read the byte tables from global memory:
// crc_raw(shift(A, 1008 B), first n bytes of p)
__device__ __noinline__ uint32_t crc_partial_g(const uint32_t *__restrict__ T, uint32_t A, const uint32_t p[4], int n) {
    uint32_t c = T[16 * 256 + (A & 0xffu)] ^ T[17 * 256 + ((A >> 8) & 0xffu)] ^ T[18 * 256 + ((A >> 16) & 0xffu)] ^
                 T[19 * 256 + (A >> 24)];
    for (int i = 0; i < n; i++) {
        const uint32_t byte = (p[i >> 2] >> (8 * (i & 3))) & 0xffu;
        c = T[15 * 256 + ((c ^ byte) & 0xffu)] ^ (c >> 8);
    }
    return c;
}

constexpr int kCrcWpe = 4;     // waves per SIMD the compiler plans for (one 16-wave workgroup per CU)
constexpr int kCrcChains = 2;  // spans whose slice-by-4 chains run interleaved
__global__ __launch_bounds__(kCrcWaves * 64) __attribute__((amdgpu_waves_per_eu(kCrcWpe))) void crc_segments_k(const Task *__restrict__ tasks,
                                                                const BlkDev *__restrict__ blks, DevTables tab) {
    __shared__ __attribute__((aligned(16))) char lds[kCrcLds];
    const Task task = tasks[blockIdx.x];
    const BlkDev blk = blks[task.blk];
    const uint32_t tid = threadIdx.x;
    // stage: byte tables U12..U15, i = (table t, entry e, replica quad rq)
    for (uint32_t i = tid; i < 4 * 256 * 8; i += kCrcWaves * 64) {
        const uint32_t rq = i & 7, e = (i >> 3) & 255, t = i >> 11;
        const uint32_t v = tab.crc[(12 + t) * 256 + e];
        *reinterpret_cast<uint4 *>(lds + (t >> 1) * 0x10000u + e * 256 + (t & 1) * 128 + 16 * rq) =
            make_uint4(v, v, v, v);
    }
    // the 4096-B shift as nibble tables in region 2: i = (table t, hi, nibble, rq)
    for (uint32_t i = tid; i < 4 * 2 * 16 * 8; i += kCrcWaves * 64) {
        const uint32_t rq = i & 7, nib = (i >> 3) & 15, hi = (i >> 7) & 1, t = i >> 8;
        const uint32_t v = tab.crc[(28 + t) * 256 + (hi ? nib << 4 : nib)];
        *reinterpret_cast<uint4 *>(lds + 0x20000u + t * 4096 + nib * 256 + hi * 128 + 16 * rq) =
            make_uint4(v, v, v, v);
    }
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const uint32_t lb = ((lane & 31) << 2) | 0x10000u | 0x2000000u;
    const uint8_t *src = blk.src;
    for (uint64_t seg0 = task.c0 + (uint64_t)wave * kSeg; seg0 < task.c1; seg0 += (uint64_t)kCrcWaves * kSeg) {
        const uint64_t seg1 = seg0 + kSeg < task.c1 ? seg0 + kSeg : task.c1;
        uint32_t A = 0, lend = 0;
        const uint64_t nrows = (seg1 - seg0 + 1023) / 1024;
        if (seg1 - seg0 == (uint64_t)kSeg) {
            // full segment, 64-B lane chunks of the 8 spans of 4 KiB; CH spans
            // are CH independent slice-by-4 chains, and each piece's load for
            // the span CH further on is issued as soon as the piece is consumed
            constexpr int CH = kCrcChains;
            uint4 buf[CH][4];
#pragma unroll
            for (int k = 0; k < CH; k++)
#pragma unroll
                for (int j = 0; j < 4; j++) buf[k][j] = crc_chunk_ld(src + seg0, lane, k, j);
#pragma unroll
            for (int r = 0; r < 8; r += CH) {
#pragma unroll
                for (int k = 0; k < CH; k++) quad_xpose(buf[k], lane);
                // x = state ^ next word; each step folds the next word into
                // its 4-way XOR (two v_bitop3)
                uint32_t x[CH];
#pragma unroll
                for (int k = 0; k < CH; k++) x[k] = buf[k][0].x;
#pragma unroll
                for (int j = 0; j < 4; j++) {
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].y);
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].z);
                    if (j < 3) {
#pragma unroll
                        for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].w);
#pragma unroll
                        for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j + 1].x);
                    } else {
#pragma unroll
                        for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].w);
                    }
                    // piece j of every chain consumed (its .x was read one step ago)
                    if (r + CH < 8 && j > 0) {
#pragma unroll
                        for (int k = 0; k < CH; k++) buf[k][j - 1] = crc_chunk_ld(src + seg0, lane, r + CH + k, j - 1);
                    }
                }
                if (r + CH < 8) {
#pragma unroll
                    for (int k = 0; k < CH; k++) buf[k][3] = crc_chunk_ld(src + seg0, lane, r + CH + k, 3);
                }
#pragma unroll
                for (int k = 0; k < CH; k++) A = crc_step4x(lds, lb, x[k], crc_shift4096(lds, lb, A));
            }
            lend = kSeg;
        } else {
            for (uint64_t r = 0; r < nrows; r++) {
                const uint64_t o = seg0 + 1024 * r + 16 * lane;
                const uint4 p = load_piece(src, o, seg1);
                if (o + 16 <= seg1) {
                    A = crc_row_g(lds, tab.crc, lb, A, p);
                    lend = (uint32_t)(o + 16 - seg0);
                } else if (o < seg1) {
                    const uint32_t pw[4] = {p.x, p.y, p.z, p.w};
                    A = crc_partial_g(tab.crc, A, pw, (int)(seg1 - o));
                    lend = (uint32_t)(seg1 - seg0);
                }
            }
        }
        const uint32_t Lseg = (uint32_t)(seg1 - seg0);
        uint32_t v, K;
        if (Lseg == (uint32_t)kSeg) {
            // lane chunk end to segment end: 64 * (63 - chunk index) bytes
            v = crc_mulmod(tab.crcx[128 + crc_chunk_idx(lane)], A);
            K = tab.crcx[96];
        } else {
            v = crc_mulmod(crc_xpow8(Lseg - lend, tab.crcx + 64), A);
            K = crc_mulmod(crc_xpow8(Lseg, tab.crcx + 64), 0xffffffffu);
        }
        const uint32_t raw = wave_xor(v);
        if (lane == 0) {
            const uint32_t crc = ~(K ^ raw);
            const uint64_t si = seg0 / kSeg;
            if (blk.crc_calc)
                blk.crc_calc[si] = crc;
            else
                *reinterpret_cast<uint32_t *>(blk.crc + 4 * si) = __builtin_bswap32(crc);
        }
    }
}

// ---------------------------------------------------------------------------
// Hadoop file checksum (MD5-of-MD5-of-CRC32C), CRC phase: one CRC32C per
// 512-byte chunk of a file (getFileChecksum, sdk/java/.../JuiceFileSystemImpl
// .java:1297-1342; bytesPerCRC = 512), written as one big-endian word per
// chunk at index offset / 512 of the file's chunk-CRC array (blk.crc_calc).
//
// Same machine as crc_segments_k's default path: byte tables U12..U15 in LDS
// (one replica per bank), quad-transposed coalesced non-temporal loads, two
// interleaved slice-by-4 chains, a wave takes a 32 KiB run of 8 spans of 4 KiB
// and a lane a 64-byte piece of each span.  The piece with span index
// ci = crc_chunk_idx(lane) is position pos = ci & 7 of chunk ci >> 3, so the
// lane CRC has to move 64 * (7 - pos) bytes to the chunk end: a multiply by
// x^(8 * 64 * (7 - pos)) (crcx[128 + 56 + pos]).  pos is fixed per lane, and
// lanes l and l + 32 share both their LDS bank and their pos, so the multiply
// is a linear map looked up in region 2, where crc_segments_k keeps its
// 4096-byte shift: the nibble tables of bank b hold the map of pos(b)
// (crc_chunk_mul, 1024 words built by the host).  That is 8 conflict-free
// lookups per span, what the span shift costs crc_segments_k, against about
// 190 VALU operations for a crc_mulmod -- more than the 16 table steps of the
// span itself.  The 8 lanes of a chunk are then XORed together: after the
// quad transpose they are the lanes 4 apart inside a 32-lane half (lane bits
// 2..4), reduced by two DPP row rotates (row_ror:4, row_ror:8: all lanes of a
// 16-lane row with the same lane & 3) and one ds_swizzle (xor 16); no LDS
// memory and no barrier.  K512 = x^(8 * 512) * 0xffffffff, the init/xorout
// term of a 512-byte message, comes from the host.
// A run shorter than 32 KiB (the end of a file) goes span by span through
// crc_chunks_span_g: guarded loads (load_piece), the last 1..3 bytes of the
// file through the global byte table, and for the file's short last chunk a
// crc_mulmod by the distance to its end.
__device__ __forceinline__ uint32_t chunk_xor8(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xF, 0xF, true);  // row_ror:4
    v ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);  // row_ror:8
    v ^= (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x401F);              // lane ^ 16
    return v;
}

// one span [s0, min(s0 + 4096, end)) of a file, every load guarded
__device__ __noinline__ void crc_chunks_span_g(const char *lds, uint32_t lb, const uint32_t *__restrict__ T,
                                               const uint32_t *__restrict__ crcx, const uint8_t *src, uint64_t s0,
                                               uint64_t end, uint32_t *__restrict__ out, uint32_t lane,
                                               uint32_t K512) {
    const uint32_t ci = crc_chunk_idx(lane);
    const uint64_t o = s0 + 64 * ci;
    const uint32_t n = o >= end ? 0u : (end - o < 64 ? (uint32_t)(end - o) : 64u);
    uint32_t pw[16];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint4 p = load_piece(src, o + 16 * j, end);
        pw[4 * j] = p.x, pw[4 * j + 1] = p.y, pw[4 * j + 2] = p.z, pw[4 * j + 3] = p.w;
    }
    uint32_t c = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; w++) {
        if (4 * w + 4 <= n) {
            c = crc_step4(lds, lb, c ^ pw[w]);
        } else if (4 * w < n) {
            for (uint32_t i = 0; i < n - 4 * w; i++)
                c = T[15 * 256 + ((c ^ (pw[w] >> (8 * i))) & 0xffu)] ^ (c >> 8);
        }
    }
    const uint64_t cs = s0 + 512 * (uint64_t)(ci >> 3);  // the chunk's first byte
    uint32_t v = 0, K = K512;
    if (cs + 512 <= end) {
        v = crc_shift4096(lds, lb, c);  // a whole chunk: the lane's map (crc_chunk_mul)
    } else if (n) {
        // the file's short last chunk [cs, end): the piece ends d bytes before it does
        const uint64_t d = end - (o + n);
        v = d ? crc_mulmod(crc_xpow8(d, crcx + 64), c) : c;
        K = crc_mulmod(crc_xpow8(end - cs, crcx + 64), 0xffffffffu);
    }
    const uint32_t raw = chunk_xor8(v);
    if ((ci & 7u) == 0 && cs < end) out[cs >> 9] = __builtin_bswap32(~(K ^ raw));
}

__global__ __launch_bounds__(kCrcWaves * 64) __attribute__((amdgpu_waves_per_eu(kCrcWpe))) void crc_chunks_k(
    const Task *__restrict__ tasks, const BlkDev *__restrict__ blks, DevTables tab,
    const uint32_t *__restrict__ crc_chunk_mul, uint32_t K512) {
    __shared__ __attribute__((aligned(16))) char lds[kCrcLds];
    const Task task = tasks[blockIdx.x];
    const BlkDev blk = blks[task.blk];
    const uint32_t tid = threadIdx.x;
    // stage: byte tables U12..U15, i = (table t, entry e, replica quad rq)
    for (uint32_t i = tid; i < 4 * 256 * 8; i += kCrcWaves * 64) {
        const uint32_t rq = i & 7, e = (i >> 3) & 255, t = i >> 11;
        const uint32_t v = tab.crc[(12 + t) * 256 + e];
        *reinterpret_cast<uint4 *>(lds + (t >> 1) * 0x10000u + e * 256 + (t & 1) * 128 + 16 * rq) =
            make_uint4(v, v, v, v);
    }
    // region 2, the chunk-end multiply as nibble tables: i = (table t, hi,
    // nibble, bank); bank b holds the map of the pos its two lanes have
    for (uint32_t i = tid; i < 4 * 2 * 16 * 32; i += kCrcWaves * 64) {
        const uint32_t bank = i & 31, nib = (i >> 5) & 15, hi = (i >> 9) & 1, t = i >> 10;
        const uint32_t pos = crc_chunk_idx(bank) & 7u;
        *reinterpret_cast<uint32_t *>(lds + 0x20000u + t * 4096 + nib * 256 + hi * 128 + 4 * bank) =
            crc_chunk_mul[((t * 2 + hi) * 16 + nib) * 8 + pos];
    }
    __syncthreads();
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const uint32_t lb = ((lane & 31) << 2) | 0x10000u | 0x2000000u;
    const uint8_t *src = blk.src;
    uint32_t *__restrict__ out = blk.crc_calc;
    const uint32_t ci = crc_chunk_idx(lane);
    for (uint64_t seg0 = task.c0 + (uint64_t)wave * kSeg; seg0 < task.c1; seg0 += (uint64_t)kCrcWaves * kSeg) {
        if (seg0 + kSeg > task.c1) {
            for (uint64_t s0 = seg0; s0 < task.c1; s0 += 4096)
                crc_chunks_span_g(lds, lb, tab.crc, tab.crcx, src, s0, task.c1, out, lane, K512);
            continue;
        }
        // a whole 32 KiB run: the loop of crc_segments_k's default path, with
        // the span shift replaced by the chunk combine
        constexpr int CH = kCrcChains;
        uint4 buf[CH][4];
#pragma unroll
        for (int k = 0; k < CH; k++)
#pragma unroll
            for (int j = 0; j < 4; j++) buf[k][j] = crc_chunk_ld(src + seg0, lane, k, j);
#pragma unroll
        for (int r = 0; r < 8; r += CH) {
#pragma unroll
            for (int k = 0; k < CH; k++) quad_xpose(buf[k], lane);
            uint32_t x[CH];
#pragma unroll
            for (int k = 0; k < CH; k++) x[k] = buf[k][0].x;
#pragma unroll
            for (int j = 0; j < 4; j++) {
#pragma unroll
                for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].y);
#pragma unroll
                for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].z);
                if (j < 3) {
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].w);
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j + 1].x);
                } else {
#pragma unroll
                    for (int k = 0; k < CH; k++) x[k] = crc_step4x(lds, lb, x[k], buf[k][j].w);
                }
                if (r + CH < 8 && j > 0) {
#pragma unroll
                    for (int k = 0; k < CH; k++) buf[k][j - 1] = crc_chunk_ld(src + seg0, lane, r + CH + k, j - 1);
                }
            }
            if (r + CH < 8) {
#pragma unroll
                for (int k = 0; k < CH; k++) buf[k][3] = crc_chunk_ld(src + seg0, lane, r + CH + k, 3);
            }
#pragma unroll
            for (int k = 0; k < CH; k++) {
                // x[k] = crc_raw(0, the lane's piece of span r + k), still to
                // go through its last table step
                const uint32_t raw = chunk_xor8(crc_shift4096(lds, lb, crc_step4(lds, lb, x[k])));
                if ((ci & 7u) == 0) out[((seg0 + 4096 * (r + k)) >> 9) + (ci >> 3)] = __builtin_bswap32(~(K512 ^ raw));
            }
        }
    }
}

// Hadoop file checksum, block phase: lane b hashes the nw[b] chunk-CRC words
// of DFS block b (4 * min(crcPerBlock, chunks left) bytes at words + w0[b];
// the words are the big-endian CRC bytes as stored, so the little-endian load
// already is MD5's message word) and writes the 16-byte digest.  Serial per
// block by nature, about 16384 compressions for a 128 MiB block; the next
// 64 bytes are loaded while the current ones are hashed.
__global__ __launch_bounds__(64) void md5_blocks_k(const Md5Job *__restrict__ jobs, uint32_t njobs,
                                                  const uint32_t *__restrict__ words,
                                                  uint32_t *__restrict__ digests) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b >= njobs) return;
    const Md5Job job = jobs[b];
    const uint32_t *p = words + job.w0;
    const uint64_t nfull = job.nw / 16;
    uint32_t st[4], cur[16], nxt[16];
#pragma unroll
    for (int i = 0; i < 16; i++) nxt[i] = 0;
    jfsx_md5::iv(st);
    if (nfull) {
#pragma unroll
        for (int i = 0; i < 16; i++) cur[i] = p[i];
    }
    for (uint64_t k = 0; k < nfull; k++) {
        if (k + 1 < nfull) {
#pragma unroll
            for (int i = 0; i < 16; i++) nxt[i] = p[16 * (k + 1) + i];
        }
        jfsx_md5::compress(st, cur);
#pragma unroll
        for (int i = 0; i < 16; i++) cur[i] = nxt[i];
    }
    jfsx_md5::finish_words(st, job.nw, [&](uint64_t i) { return p[i]; });
#pragma unroll
    for (int i = 0; i < 4; i++) digests[4 * b + i] = st[i];
}

void launch_crc_chunks(hipStream_t s, int ntasks, const Task *tasks, const BlkDev *blks, DevTables t,
                       const uint32_t *crc_chunk_mul, uint32_t K512) {
    if (ntasks > 0)
        hipLaunchKernelGGL(crc_chunks_k, dim3(ntasks), dim3(kCrcWaves * 64), 0, s, tasks, blks, t, crc_chunk_mul, K512);
}

void launch_md5_blocks(hipStream_t s, uint32_t njobs, const Md5Job *jobs, const uint32_t *words, uint32_t *digests) {
    if (njobs > 0)
        hipLaunchKernelGGL(md5_blocks_k, dim3((njobs + 63) / 64), dim3(64), 0, s, jobs, njobs, words, digests);
}

// zero-length ranges/blocks still produce one zero CRC (Go's checksum(): 4 bytes)
__global__ __launch_bounds__(64) void crc_finalize_k(const BlkDev *__restrict__ blks, int crc_mode,
                                                    BlkOut *__restrict__ out) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const BlkDev blk = blks[b];
    BlkOut o;
    for (int q = 0; q < 4; q++) o.tag[q] = 0;
    o.status = JFSX_OK;
    o.bad_seg = -1;
    o.got = o.expect = 0;
    if (crc_mode == JFSX_CRC_GEN && blk.len == 0 && lane == 0) *reinterpret_cast<uint32_t *>(blk.crc) = 0;
    if (crc_mode == JFSX_CRC_VERIFY) {
        crc_verify_block(blk, o, lane);
        if (o.bad_seg >= 0) o.status = JFSX_ECRC;
    }
    if (lane == 0) out[b] = o;
}

// SplitMix64 stream: word k of block b = mix64(seed + G*((b << 40) + k + 1))
// (identical to oracle/jfs_oracle.c orc_gen_block)
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void gen_synthetic_k(uint8_t *__restrict__ dst, uint64_t len, uint64_t seed,
                                                      uint64_t block) {
    const uint64_t G = 0x9E3779B97F4A7C15ULL;
    const uint64_t nw2 = len / 16;
    const uint64_t base = seed + G * ((block << 40) + 1);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nw2;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = mix64(base + G * (2 * i)), b = mix64(base + G * (2 * i + 1));
        *reinterpret_cast<ulonglong2 *>(dst + 16 * i) = make_ulonglong2(a, b);
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        const uint64_t i = nw2 * 16 + threadIdx.x;
        if (i < len) {
            const uint64_t w = mix64(base + G * (i / 8));
            dst[i] = (uint8_t)(w >> (8 * (i % 8)));
        }
    }
}

// batched generator: grid (x = workgroups per block, y = block), block i of
// the batch is the stream of global block block0 + i, lens[i] bytes at
// dst + i * stride (one launch for a whole bench batch)
__global__ __launch_bounds__(256) void gen_synthetic_batch_k(uint8_t *__restrict__ dst, uint64_t stride,
                                                            const uint64_t *__restrict__ lens, uint64_t seed,
                                                            uint64_t block0) {
    const uint64_t G = 0x9E3779B97F4A7C15ULL;
    const uint32_t bi = blockIdx.y;
    const uint64_t len = lens[bi];
    uint8_t *d = dst + stride * bi;
    const uint64_t nw2 = len / 16;
    const uint64_t base = seed + G * (((block0 + bi) << 40) + 1);
    for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < nw2;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t a = mix64(base + G * (2 * i)), b = mix64(base + G * (2 * i + 1));
        *reinterpret_cast<ulonglong2 *>(d + 16 * i) = make_ulonglong2(a, b);
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) {
        const uint64_t i = nw2 * 16 + threadIdx.x;
        if (i < len) {
            const uint64_t w = mix64(base + G * (i / 8));
            d[i] = (uint8_t)(w >> (8 * (i % 8)));
        }
    }
}

// dst[0, bytes) = src[0, bytes) for a small region (a pipeline group's
// descriptors) read by the GPU straight out of pinned host memory, which the
// host rewrote since the previous group: system-scope loads, so no cache level
// can hand back the previous group's words.  bytes is a multiple of 4.
__global__ __launch_bounds__(256) void pull_k(uint32_t *__restrict__ dst, uint32_t *__restrict__ src, uint32_t n4) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256)
        dst[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

void launch_pull(hipStream_t s, void *dst, const void *src, size_t bytes) {
    const uint32_t n4 = (uint32_t)(bytes / 4);
    if (!n4) return;
    const uint32_t grid = (n4 + 255) / 256 < 128 ? (n4 + 255) / 256 : 128;
    hipLaunchKernelGGL(pull_k, dim3(grid), dim3(256), 0, s, (uint32_t *)dst, (uint32_t *)src, n4);
}

void launch_gen_synthetic_batch(hipStream_t s, uint8_t *dst, uint64_t stride, int n, const uint64_t *lens,
                                uint64_t seed, uint64_t block0) {
    // y <= 65535 blocks per launch
    for (int i0 = 0; i0 < n; i0 += 65535) {
        const int m = n - i0 < 65535 ? n - i0 : 65535;
        hipLaunchKernelGGL(gen_synthetic_batch_k, dim3(16, (unsigned)m), dim3(256), 0, s, dst + stride * i0, stride,
                           lens + i0, seed, block0 + i0);
    }
}

void launch_crc_segments(hipStream_t s, int ntasks, const Task *tasks, const BlkDev *blks, DevTables t) {
    if (ntasks > 0) hipLaunchKernelGGL(crc_segments_k, dim3(ntasks), dim3(kCrcWaves * 64), 0, s, tasks, blks, t);
}

void launch_crc_finalize(hipStream_t s, int n, int crc_mode, const BlkDev *blks, BlkOut *out) {
    if (n > 0) hipLaunchKernelGGL(crc_finalize_k, dim3(n), dim3(64), 0, s, blks, crc_mode, out);
}

void launch_gen_synthetic(hipStream_t s, uint8_t *dst, uint64_t len, uint64_t seed, uint64_t block) {
    uint64_t nw2 = len / 16;
    uint64_t blocks = (nw2 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(gen_synthetic_k, dim3((unsigned)blocks), dim3(256), 0, s, dst, len, seed, block);
}

}  // namespace jfsx
