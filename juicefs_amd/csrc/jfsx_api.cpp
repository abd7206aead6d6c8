// jfsx_api.cpp -- C-ABI of libjfsx.so (include/jfsx.h): contexts, tables,
// batch planning, staging, launches.  Host code, compiled by hipcc.
//
// A batch runs as: H2D of descriptors (one pinned copy) -> keysetup kernel ->
// main transform kernel (one workgroup per task) -> finalize kernel -> D2H of
// per-block results (tags, status, first failing CRC) -> stream sync.
#include <ctype.h>
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <stdexcept>
#include <thread>
#include <vector>

#include "jfsx_internal.h"

#define JFSX_HD static inline
#include "jfsx_rsa.h"
#include "jfsx_md5.h"
#include "jfsx_store.h"
#include "jfsx_objload.h"
#include "jfsx_compact.h"
#include "jfsx_gather.h"

using namespace jfsx;

// Every HIP failure is recorded with its call site before the engine returns
// JFSX_EIO, so a caller can tell a device fault from an out-of-resources
// launch or a bad copy (jfsx_last_error).
#define HIP_OK(x)                                                      \
    do {                                                               \
        const hipError_t e_ = (x);                                     \
        if (e_ != hipSuccess) {                                        \
            note_hip_error(e_, __FILE__, __LINE__, #x);                \
            return JFSX_EIO;                                           \
        }                                                              \
    } while (0)

namespace {

// last failure: per calling thread, and per context for calls made on one
struct ErrRec {
    int hip = 0;
    char msg[320] = {0};
};
thread_local ErrRec tl_err;
thread_local jfsx_ctx *tl_ctx = nullptr;  // context of the entry point running on this thread
void note_ctx_error(jfsx_ctx *c, const ErrRec &e);

void note_hip_error(hipError_t e, const char *file, int line, const char *expr) {
    const char *base = strrchr(file, '/');
    snprintf(tl_err.msg, sizeof(tl_err.msg), "%s (%s) at %s:%d in %s", hipGetErrorName(e), hipGetErrorString(e),
             base ? base + 1 : file, line, expr);
    tl_err.hip = (int)e;
    if (tl_ctx) note_ctx_error(tl_ctx, tl_err);
    (void)hipGetLastError();  // a handled failure must not resurface at the next launch check
}

// hipGetLastError() after a launch also returns the error of any earlier
// failed HIP call of this thread (a handled hipMalloc failure, say): clear the
// slot before launching, so the check that follows sees only the launch
inline void launch_begin() { (void)hipGetLastError(); }

// an entry point's scope: failures inside it are also kept on the context
struct CtxScope {
    jfsx_ctx *prev;
    explicit CtxScope(jfsx_ctx *c) : prev(tl_ctx) { tl_ctx = c; }
    ~CtxScope() { tl_ctx = prev; }
};

// Device allocations made through jfsx_alloc_device, by address: a
// multi-device context routes each block of a device-memory batch to the GPU
// that owns its buffers (jfsx_mctx_seal_batch and friends).
std::shared_mutex g_alloc_mu;
std::map<uintptr_t, std::pair<uintptr_t, int>> g_allocs;  // base -> (end, device)

void note_alloc(void *p, size_t bytes, int device) {
    std::unique_lock<std::shared_mutex> g(g_alloc_mu);
    g_allocs[(uintptr_t)p] = {(uintptr_t)p + bytes, device};
}
void forget_alloc(void *p) {
    std::unique_lock<std::shared_mutex> g(g_alloc_mu);
    g_allocs.erase((uintptr_t)p);
}

// Page-locked host allocations made through jfsx_alloc_pinned(_node), by
// address: a host call streams such blocks with no bounce copy.
std::shared_mutex g_pin_mu;
std::map<uintptr_t, uintptr_t> g_pinned;  // base -> end

void note_pinned(void *p, size_t bytes) {
    std::unique_lock<std::shared_mutex> g(g_pin_mu);
    g_pinned[(uintptr_t)p] = (uintptr_t)p + bytes;
}
void forget_pinned(void *p) {
    std::unique_lock<std::shared_mutex> g(g_pin_mu);
    g_pinned.erase((uintptr_t)p);
}
// base of the engine-pinned allocation holding p, 0 if none
uintptr_t pinned_base(const void *p) {
    const uintptr_t a = (uintptr_t)p;
    std::shared_lock<std::shared_mutex> g(g_pin_mu);
    auto it = g_pinned.upper_bound(a);
    if (it == g_pinned.begin()) return 0;
    --it;
    return a < it->second ? it->first : 0;
}

// JFSX_HOST_STAGE: how a pageable host block reaches the DMA engines.
//   bounce (default)    copy it into the context's pinned bounce buffers on
//                       the calling thread (20 per-object callers: 41.7 GB/s,
//                       0.22 host CPU-s per GB, profiles/r6)
//   register            pin the caller's own pages for the call
//                       (hipHostRegister / hipHostUnregister around it), and
//                       bounce where the runtime refuses; no copies (0.10 CPU-s
//                       per GB) but 28-31 GB/s: under 20 concurrent callers
//                       the runtime's registration and lookup calls contend
//   none                hand the pageable pointer to hipMemcpyAsync as it is
//                       (the runtime's own staged copy: 15.3 GB/s, A/B only)
//   all                 bounce every host block, pinned or not (tests)
enum { kStageNone = 0, kStageRegister = 1, kStageBounce = 2, kStageAll = 3 };
int stage_policy() {
    static const int v = [] {
        const char *e = getenv("JFSX_HOST_STAGE");
        if (!e || !strcmp(e, "bounce")) return (int)kStageBounce;
        if (!strcmp(e, "register")) return (int)kStageRegister;
        if (!strcmp(e, "none")) return (int)kStageNone;
        return (int)kStageAll;
    }();
    return v;
}
}  // namespace

namespace jfsx {
// true when [p, p + n) may be handed to the DMA engines as it is: engine-pinned
// memory, or host memory the HIP runtime reports as registered (another
// library's pinned buffers).  Everything else -- the Go heap, malloc, numpy --
// is pageable and goes through the context's bounce pool.
bool host_pinned(const void *p, uint64_t n) {
    const int pol = stage_policy();
    if (pol == kStageNone || pol == kStageAll || !n) return pol != kStageAll || !n;
    const uintptr_t a = (uintptr_t)p;
    {
        std::shared_lock<std::shared_mutex> g(g_pin_mu);
        auto it = g_pinned.upper_bound(a);
        if (it != g_pinned.begin()) {
            --it;
            if (a < it->second) return a + n <= it->second;
        }
    }
    hipPointerAttribute_t at;
    const bool reg = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost;
    (void)hipGetLastError();
    return reg;
}

// Pin a pageable caller range for the duration of one call (JFSX_HOST_STAGE
// register): true when it is now page-locked and must be released with
// host_unpin once the call's DMA has finished; false where the policy is not
// register or the runtime refuses (the caller then bounces the block).  The
// Go heap does not move objects, and the range is released before the call
// returns, so cgo's rule that C keeps no Go pointer past the call holds.
bool host_pin(const void *p, uint64_t n) {
    if (stage_policy() != kStageRegister || !n) return false;
    const hipError_t e = hipHostRegister(const_cast<void *>(p), n, hipHostRegisterPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    note_pinned(const_cast<void *>(p), n);  // host_pinned() then answers from the registry
    return true;
}
void host_unpin(const void *p) {
    forget_pinned(const_cast<void *>(p));
    if (hipHostUnregister(const_cast<void *>(p)) != hipSuccess) (void)hipGetLastError();
}
}  // namespace jfsx

namespace {

// ---------------------------------------------------------------------------
// table construction (host)
// ---------------------------------------------------------------------------
uint8_t gf8_mul(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    while (b) {
        if (b & 1) p ^= a;
        a = (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1B : 0));
        b >>= 1;
    }
    return p;
}

void make_aes_table(std::vector<uint32_t> &t) {
    // S-box = affine(inverse) over GF(2^8) (FIPS-197 5.1.1)
    uint8_t sbox[256];
    for (int x = 0; x < 256; x++) {
        uint8_t inv = 0;
        if (x) {
            uint8_t r = 1, base = (uint8_t)x;
            for (int e = 254; e; e >>= 1) {
                if (e & 1) r = gf8_mul(r, base);
                base = gf8_mul(base, base);
            }
            inv = r;
        }
        uint8_t s = inv, v = inv;
        for (int k = 1; k <= 4; k++) v ^= (uint8_t)((s << k) | (s >> (8 - k)));
        sbox[x] = v ^ 0x63;
    }
    t.assign(256 * 64, 0);
    for (int x = 0; x < 256; x++) {
        uint32_t s = sbox[x];
        uint32_t t0 = gf8_mul((uint8_t)s, 2) | (s << 8) | (s << 16) | ((uint32_t)gf8_mul((uint8_t)s, 3) << 24);
        uint32_t t2 = (t0 << 16) | (t0 >> 16);
        for (int r = 0; r < 32; r++) {
            t[x * 64 + r] = t0;
            t[x * 64 + 32 + r] = t2;
        }
    }
}

uint32_t crc_mulmod_h(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & 0x80000000u) p ^= b;
        a <<= 1;
        b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

// crcb (nullable): the composed tables of gcm_main's two-row loop, which
// carries B = x^8064 * A (the lane CRC already shifted across the 1008-byte
// gap to its next piece): TT_0..15, TT_k[v] = x^8064 * U_k[v] (16 x 256
// dwords), then the 64 lane constants xlB[l] = xl[l] * x^-8064 that bring a
// B-form state to the segment end (xlB[63] = x^-8064 itself)
void make_crc_tables(std::vector<uint32_t> &crc, std::vector<uint32_t> &crcx, std::vector<uint32_t> *crcb = nullptr) {
    uint32_t T[256];
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
        T[i] = c;
    }
    uint32_t x8[32];
    x8[0] = 0x00800000u;  // x^8
    for (int k = 1; k < 32; k++) x8[k] = crc_mulmod_h(x8[k - 1], x8[k - 1]);
    auto xpow8 = [&](uint64_t n) {
        uint32_t r = 0x80000000u;
        for (int k = 0; n; k++, n >>= 1)
            if (n & 1) r = crc_mulmod_h(x8[k], r);
        return r;
    };
    crc.assign(32 * 256, 0);
    for (int j = 0; j < 16; j++) {
        const uint32_t xp = xpow8(15 - j);
        for (int b = 0; b < 256; b++) crc[j * 256 + b] = crc_mulmod_h(xp, T[b]);
    }
    // S tables: shift a lane CRC across the gap to its next piece -- 1008 B for
    // 16-B pieces at 1 KiB row stride (GCM), 4032 B for 64-B chunks at 4 KiB (ChaCha)
    // (and 1024 B / 4096 B: a whole row / a whole 4 KiB span of 64-B lane chunks,
    // for the CRC-only kernel's A' = S(A) ^ crc_raw(0, chunk))
    const uint32_t x1008 = xpow8(1008), x4032 = xpow8(4032), x1024 = xpow8(1024), x4096 = xpow8(4096);
    for (int k = 0; k < 4; k++)
        for (uint32_t v = 0; v < 256; v++) {
            crc[(16 + k) * 256 + v] = crc_mulmod_h(x1008, v << (8 * k));
            crc[(20 + k) * 256 + v] = crc_mulmod_h(x4032, v << (8 * k));
            crc[(24 + k) * 256 + v] = crc_mulmod_h(x1024, v << (8 * k));
            crc[(28 + k) * 256 + v] = crc_mulmod_h(x4096, v << (8 * k));
        }
    crcx.assign(192, 0);
    for (int l = 0; l < 64; l++) crcx[l] = xpow8(16 * (63 - l));
    for (int k = 0; k < 32; k++) crcx[64 + k] = x8[k];
    crcx[96] = crc_mulmod_h(xpow8(kSeg), 0xffffffffu);
    // x^(8 * 1024 k), k = 1..31: whole-row shifts (crc_xpow8_fast, jfsx_internal.h)
    for (int k = 1; k < 32; k++) crcx[96 + k] = xpow8(1024 * (uint64_t)k);
    for (int l = 0; l < 64; l++) crcx[128 + l] = xpow8(64 * (63 - l));
    if (crcb) {
        crcb->assign(16 * 256 + 64, 0);
        for (int i = 0; i < 16 * 256; i++) (*crcb)[i] = crc_mulmod_h(x1008, crc[i]);
        // P(0) = 1, so x * ((P - 1) / x) = 1 mod P: x^-1 is P without its
        // constant term, divided by x (one bit to the left in this bit order,
        // x^32 / x landing on bit 0); x^-8064 by square and multiply
        uint32_t sq = ((kCrcPoly & 0x7fffffffu) << 1) | 1u, inv = 0x80000000u;
        for (uint32_t n = 8 * 1008; n; n >>= 1, sq = crc_mulmod_h(sq, sq))
            if (n & 1) inv = crc_mulmod_h(sq, inv);
        for (int l = 0; l < 64; l++) (*crcb)[16 * 256 + l] = crc_mulmod_h(crcx[l], inv);
    }
}

// crc_chunks_k's chunk-end multiplies (jfsx_crc.hip): the lane CRC of the
// 64-byte piece at position pos of a 512-byte chunk times x^(8 * 64 * (7 - pos)),
// as 8 nibble tables per pos: m[((t * 2 + hi) * 16 + nib) * 8 + pos] is the
// product for nibble hi of byte t.  *k512 = x^(8 * 512) * 0xffffffff, the
// init/xorout term of a whole chunk.
void make_crc_chunk_mul(std::vector<uint32_t> &m, uint32_t *k512) {
    uint32_t x64 = 0x00800000u;  // x^8, squared six times: x^(8 * 64)
    for (int k = 0; k < 6; k++) x64 = crc_mulmod_h(x64, x64);
    uint32_t xp[8];
    xp[7] = 0x80000000u;  // x^0
    for (int pos = 6; pos >= 0; pos--) xp[pos] = crc_mulmod_h(xp[pos + 1], x64);
    m.assign(4 * 2 * 16 * 8, 0);
    for (uint32_t t = 0; t < 4; t++)
        for (uint32_t hi = 0; hi < 2; hi++)
            for (uint32_t nib = 0; nib < 16; nib++)
                for (uint32_t pos = 0; pos < 8; pos++)
                    m[((t * 2 + hi) * 16 + nib) * 8 + pos] = crc_mulmod_h(xp[pos], (nib << (4 * hi)) << (8 * t));
    *k512 = crc_mulmod_h(crc_mulmod_h(xp[0], x64), 0xffffffffu);
}

inline uint64_t nseg_of(uint64_t len) { return len ? (len + kSeg - 1) / kSeg : 1; }

struct Plan {
    std::vector<Task> tasks;  // in plan order: block by block, c0 ascending
    uint64_t nslots = 0;
    uint64_t task_bytes = 0;  // every task but a block's last has this many bytes
    int kind = 0;
    // the tasks in the order the kernel is given them (plan_batch)
    void dispatch(Task *out) const;
};

// Device + pinned-host scratch for one in-flight batch.
struct Workspace {
    char *d = nullptr;  // descriptors, schedules, partials, results (device)
    size_t dcap = 0;
    char *h = nullptr;  // pinned mirror: descriptors up, results down
    size_t hcap = 0;
    char *stage = nullptr;  // host-ingest staging for block data (device)
    size_t scap = 0;
    int n = 0;              // blocks of the batch in flight
    uint64_t nt = 0;        // tasks of the batch in flight
    const void *dout = nullptr;  // device BlkOut[n] of the batch in flight
    size_t down = 0;        // bytes of the result download (BlkOut[n], then the CRC words with host_crc)
    size_t crc_off = 0;     // host_crc GEN: offset of the CRC words in that download
    size_t res_off = 0;     // offset of the results (BlkOut[n], CRC words) in h
    bool crc_back = false;  // host_crc GEN: finish_aead copies the CRC words to the callers' arrays
    int crc_mult = 1;       // CRC arrays per block (2 with JFSX_CRC_BOTH)
    bool timed = false;     // the batch's main kernel is bracketed by timing events
};

constexpr int kRing = 1;  // workspace of the synchronous paths (device batches, CRC, codecs, generator)
#ifndef JFSX_PIPE
#define JFSX_PIPE 8
#endif
// Host-memory AEAD pipeline (run_aead_host): kPipe staging slots shared by every
// thread that calls on the context.  A batch is cut into groups; each group
// takes the next slot, is enqueued as H2D (s_in) -> keysetup/main/finalize
// (stream) -> D2H (s_out) and the call moves on; it then waits for its own
// groups' D2H events only.  The ring never drains between calls: while one
// caller waits for its results, the next caller's H2D is already running
// (per-object callers: the aggregator's dispatchers, cached_store.go:415-472).
constexpr int kPipe = JFSX_PIPE;

struct PipeGroup;
struct PipeSlot {
    std::mutex mu;               // held while the slot is completed or refilled
    Workspace w;
    hipEvent_t ev_in = nullptr, ev_comp = nullptr, ev_out = nullptr;
    hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;  // main-kernel timing
    hipEvent_t ev_ks = nullptr;                   // descriptors pulled and keysetup done (s_ks)
    PipeGroup *owner = nullptr;  // group in flight in this slot (its results not yet collected)
};
// one group of one host batch: where its results go once its D2H is done
struct PipeGroup {
    PipeSlot *slot = nullptr;
    jfsx_blk *dv = nullptr;  // the call's per-block result records of this group
    bool open = false;
    int rc = 0;
    char *bounce = nullptr;  // pinned bounce region of the group's pageable blocks (owner only)
    size_t bcap = 0;
    std::vector<const void *> pins;  // caller ranges pinned for the group (owner only)
};

// Engine-owned pinned staging for callers' pageable memory (SURVEY §8b
// "Ownership": the reference's pages and objects are Go-heap slices,
// pkg/chunk/page.go:42-50, pkg/object/encrypt.go:183, :258).  A host call
// copies its pageable blocks into a bounce buffer on its own thread before it
// enqueues them, and out of it on its own thread after its D2H, so concurrent
// callers copy in parallel and the DMA engines only ever see page-locked
// memory.  Grow-only per context: idle buffers are kept (up to a retention
// cap) and handed to the next call whose group fits.
struct BouncePool {
    std::mutex mu;
    std::multimap<size_t, char *> idle;  // capacity -> buffer
    size_t idle_bytes = 0;
    std::atomic<uint64_t> allocs{0}, bytes_in{0}, bytes_out{0};
};

}  // namespace

struct jfsx_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // transform stream
    hipStream_t s_in = nullptr;    // host-ingest H2D
    hipStream_t s_out = nullptr;   // host-ingest D2H
    hipStream_t s_ks = nullptr;    // host pipeline: descriptor pull + keysetup of the next group
    std::mutex mu;                 // enqueue order on the streams; the synchronous paths' workspace
    uint32_t *d_tab = nullptr;  // aes | crc | crcx | crc_chunk_mul
    const uint32_t *d_chunk_mul = nullptr;  // crc_chunks_k's chunk-end multiplies (make_crc_chunk_mul)
    uint32_t k512 = 0;
    DevTables tabs{};
    Workspace ws[kRing];
    hipEvent_t ev_k0[kRing] = {}, ev_k1[kRing] = {};  // main-kernel timing of the synchronous paths
    PipeSlot pipe[kPipe];
    int pipe_next = 0;  // next pipeline slot (under mu)
    // JFSX_PIPE_STATS=1: where host batches spend their time, printed at close
    // (groups, us enqueueing under mu, us waiting for a busy slot, us waiting
    // for one's own groups)
    std::atomic<uint64_t> ps_groups{0}, ps_enq_us{0}, ps_slot_us{0}, ps_own_us{0};
    // host-memory checks, bounce copies in (with the buffer's acquisition) and
    // out, waits for one's own groups (us, summed over callers)
    std::atomic<uint64_t> ps_pin_us{0}, ps_bin_us{0}, ps_bout_us{0}, ps_wait_us{0};
    std::atomic<uint64_t> ps_blocks{0}, ps_h2d{0}, ps_d2h{0};  // blocks, data copies up / down (coalesced runs)
    std::mutex stat_mu; // met, ms_total, launches
    std::atomic<size_t> slot_bytes{(size_t)256 << 20};
    int ncu = 256;  // compute units: persistent transform kernels launch one workgroup per CU
    size_t zstd_arena_budget = 0;  // device bytes the block-parallel zstd decoder may hold (see run_codec)
    bool timing = false;
    bool bitslice = false;  // JFSX_CTX_BITSLICE
    bool crc_l1 = false;    // crc_l1_choice, at open
    char *rsa_d = nullptr;  // batched RSA unwrap: ct | halves | em | len (device, grow-only)
    size_t rsa_dcap = 0;
    char *rsa_h = nullptr;  // pinned mirror of ct in / em + len out
    size_t rsa_hcap = 0;
    // jfsx_load_batch (run_load): its own grow-only buffers, so that no stage
    // overwrites what an earlier one left.  load_aead / load_crc are the
    // workspaces enqueue_aead (Open) and enqueue_crc plan into; load_d holds
    // LoadBlk | ZDev | ZOut | LoadRes | CRC words | the zstd decoder's arenas,
    // load_h its pinned mirror (LoadBlk up, LoadRes and CRC words down);
    // load_stage the images and pages of a host batch, or the opened images of
    // a device batch.
    Workspace load_aead, load_crc;
    Workspace obj_ct;  // jfsx_load_objects: the CRC stage over the stored images (JFSX_CRC_CT)
    hipEvent_t obj_ev[2] = {};
    char *load_d = nullptr;
    size_t load_dcap = 0;
    char *load_h = nullptr;
    size_t load_hcap = 0;
    char *load_stage = nullptr;
    size_t load_scap = 0;
    hipEvent_t load_ev[4] = {};  // main-kernel timing of its Open and CRC stages
    // jfsx_store_batch (run_store): likewise its own.  store_crc / store_aead /
    // store_ct are the workspaces the page CRC stage, the Seal and the image
    // CRC stage of a volume without a cipher plan into; store_d holds StoreBlk
    // | ZDev | ZOut | StoreRes | sinks | the compressor's tables and scratch,
    // store_h its pinned mirror (StoreBlk up, StoreRes down); store_stage the
    // pages of a host batch and the compressor's output slots; store_img the
    // packed images of a host batch (sized in phase B, from out_len).
    // jfsx_store_objects (run_store_objects) runs on the same buffers: store_d /
    // store_h also hold its SobjBlk | SobjRes in phase B, store_img the packed
    // objects of a host batch, and rsa_d / rsa_h the wrap's workspace.
    Workspace store_crc, store_aead, store_ct;
    char *store_d = nullptr;
    size_t store_dcap = 0;
    char *store_h = nullptr;
    size_t store_hcap = 0;
    char *store_stage = nullptr;
    size_t store_scap = 0;
    char *store_img = nullptr;
    size_t store_icap = 0;
    hipEvent_t store_ev[6] = {};  // main-kernel timing of its three stages
    // jfsx_gather_batch / jfsx_compact_objects: gat_d holds GPage | GPiece of a
    // launch, gat_h its pinned mirror, gat_stage the sources and destinations
    // of a host gather; cmp_d the images, source pages, new pages, packed
    // objects and page CRC words of a compaction.  The load and store stages
    // of a compaction run in the load_* / store_* buffers above.
    char *gat_d = nullptr;
    size_t gat_dcap = 0;
    char *gat_h = nullptr;
    size_t gat_hcap = 0;
    char *gat_stage = nullptr;
    size_t gat_scap = 0;
    char *cmp_d = nullptr;
    size_t cmp_dcap = 0;
    // jfsx_open_range_batch on host memory: the pinned staging of the callers'
    // pageable C on its way up and of the windows on their way down (grow-only;
    // the call holds mu throughout, so one buffer serves).  Its descriptors and
    // device staging are ws[0]'s.
    char *rng_h = nullptr;
    size_t rng_hcap = 0;
    double ms_total = 0;
    uint64_t launches = 0;
    BouncePool bounce;       // pinned staging of pageable caller memory (host calls)
    int numa_node = -1;      // host NUMA node of the device (bounce buffers are placed there)
    std::mutex err_mu;     // last HIP failure on this context (jfsx_last_error)
    ErrRec err;
    jfsx_metrics met{};      // jfsx_ctx_metrics (updated under mu)
};

namespace {
void add_kernel_ms(jfsx_ctx *c, float ms) {
    std::lock_guard<std::mutex> g(c->stat_mu);
    c->ms_total += ms;
    c->launches += 1;
}
// jfsx_ctx_metrics tallies after a batch returned 0
void tally_aead(jfsx_ctx *c, bool open, int n, const jfsx_blk *b) {
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &m = c->met;
    uint64_t bytes = 0, fail = 0;
    for (int i = 0; i < n; i++) {
        bytes += b[i].len;
        fail += b[i].status != JFSX_OK;
    }
    if (open) {
        m.open_batches++;
        m.open_blocks += n;
        m.open_bytes += bytes;
        m.open_fail += fail;
    } else {
        m.seal_batches++;
        m.seal_blocks += n;
        m.seal_bytes += bytes;
    }
}
void tally_crc(jfsx_ctx *c, int n, const jfsx_range *r) {
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &m = c->met;
    m.crc_batches++;
    m.crc_ranges += n;
    for (int i = 0; i < n; i++) {
        m.crc_bytes += r[i].len;
        m.crc_fail += r[i].status != JFSX_OK;
    }
}
void tally_codec(jfsx_ctx *c, uint64_t &blocks, uint64_t &in, uint64_t &out, uint64_t *fail, int n,
                 const jfsx_zblk *z) {
    std::lock_guard<std::mutex> g(c->stat_mu);
    blocks += n;
    for (int i = 0; i < n; i++) {
        in += z[i].src_len;
        out += z[i].out_len;
        if (fail) *fail += z[i].status != JFSX_OK;
    }
}
void note_ctx_error(jfsx_ctx *c, const ErrRec &e) {
    std::lock_guard<std::mutex> g(c->err_mu);
    c->err = e;
}
}  // namespace

namespace {

int ensure_dev(jfsx_ctx *c, char **buf, size_t *cap, size_t need) {
    if (need <= *cap) return 0;
    if (*buf) {
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(*buf));
        *buf = nullptr;
        *cap = 0;
    }
    size_t n = std::max(need, (size_t)1 << 20);
    n = (n + 0xFFFFF) & ~(size_t)0xFFFFF;
    const hipError_t e = hipMalloc((void **)buf, n);
    if (e != hipSuccess) {
        note_hip_error(e, __FILE__, __LINE__, "hipMalloc(workspace)");
        return JFSX_ENOMEM;
    }
    *cap = n;
    return 0;
}

int ensure_host(char **buf, size_t *cap, size_t need) {
    if (need <= *cap) return 0;
    if (*buf) {
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipHostFree(*buf));
        *buf = nullptr;
        *cap = 0;
    }
    size_t n = std::max(need, (size_t)1 << 20);
    n = (n + 0xFFFFF) & ~(size_t)0xFFFFF;
    const hipError_t e = hipHostMalloc((void **)buf, n, hipHostMallocDefault);
    if (e != hipSuccess) {
        note_hip_error(e, __FILE__, __LINE__, "hipHostMalloc(staging)");
        return JFSX_ENOMEM;
    }
    *cap = n;
    return 0;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Split each block into <= max_bytes tasks (a multiple of waves segments), one
// workgroup each; `slots` partial slots per task.
Plan plan_tasks(const std::vector<uint64_t> &lens, uint64_t max_bytes, uint32_t waves, uint32_t slots,
                uint64_t want, uint64_t min_task = 0) {
    Plan p;
    uint64_t total = 0;
    for (uint64_t l : lens) total += l;
    // tasks are whole segments; min_task (GCM: its row split keeps all 16
    // waves busy on any task) or else one segment per wave
    const uint64_t unit = min_task ? min_task : (uint64_t)waves * kSeg;
    uint64_t ch = max_bytes;
    // enough workgroups to fill the 256 CUs when the batch is small
    if (total / ch < want) {
        uint64_t c = (total / want + unit - 1) / unit * unit;
        ch = std::max(unit, std::min(ch, c));
    }
    p.task_bytes = ch;
    for (size_t b = 0; b < lens.size(); b++) {
        for (uint64_t c0 = 0; c0 < lens[b]; c0 += ch) {
            Task t;
            t.blk = (uint32_t)b;
            t.slot0 = (uint32_t)p.nslots;
            t.c0 = c0;
            t.c1 = std::min(c0 + ch, lens[b]);
            p.tasks.push_back(t);
            p.nslots += slots;
        }
    }
    return p;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// tasks reordered by size, largest first, in units of 4 KiB (stable within a unit)
void order_largest_first(Task *t, size_t n, size_t max_units) {
    bool sorted = true;
    for (size_t i = 1; i < n && sorted; i++) sorted = ((t[i - 1].c1 - t[i - 1].c0) >> 12) >= ((t[i].c1 - t[i].c0) >> 12);
    if (sorted) return;
    std::vector<size_t> start(max_units + 2, 0);
    for (size_t i = 0; i < n; i++) start[max_units - std::min<size_t>((t[i].c1 - t[i].c0) >> 12, max_units) + 1]++;
    for (size_t u = 1; u < start.size(); u++) start[u] += start[u - 1];
    std::vector<Task> tmp(t, t + n);
    for (size_t i = 0; i < n; i++) t[start[max_units - std::min<size_t>((tmp[i].c1 - tmp[i].c0) >> 12, max_units)]++] = tmp[i];
}

constexpr uint64_t kGcmMaxLen = (((uint64_t)1 << 32) - 2) * 16;
constexpr uint64_t kGcmMinTask = 2 * (uint64_t)kSeg;  // 64 KiB
// the cipher allows (2^32 - 1) * 64 B (x/crypto v0.19.0: (1<<38) - 64); the
// kernels hold a slot's Poly1305 exponent, a count of 16-byte blocks, in 32
// bits and 32 entries of r^(2^k) (cp_task's pexp, CpSched::r2k)
constexpr uint64_t kCpMaxLen = (((uint64_t)1 << 32) - 1) * 16;

// bytes per task of crc_segments_k: up to kCrcTaskBytes, but small enough that
// a small batch still spreads over every CU (~2 tasks per CU), and a whole
// number of 16-segment rounds (one 16-wave workgroup per task, jfsx_crc.hip)
uint64_t crc_task_bytes(uint64_t total) {
    const uint64_t round = 16 * (uint64_t)kSeg;
    return std::min<uint64_t>(kCrcTaskBytes, std::max<uint64_t>(round, (total / 512 + round - 1) / round * round));
}

// The task list of a batch: the one place that chooses it, for the AEAD
// transforms (enqueue_aead), for crc_segments_k (enqueue_crc, the ciphertext
// pass of JFSX_CRC_BOTH, the file checksum's rounds) and for jfsx_debug_plan.
// It depends on the blocks' lengths alone.
//   GCM:    a small batch (the per-object path) is cut into tasks down to
//           64 KiB so that it still spreads over the CUs (2 tasks per CU); a
//           64 GiB batch keeps 4 MiB tasks
//   ChaCha: 128 KiB (one segment per wave) to 1 MiB, 8 tasks per CU
//   CRC:    crc_task_bytes; no partial slots
enum { kPlanGcm = 0, kPlanCp = 1, kPlanCrc = 2 };

Plan plan_batch(int kind, const std::vector<uint64_t> &lens) {
    Plan p;
    if (kind == kPlanGcm) {
        p = plan_tasks(lens, kMaxTaskBytes, kWaves, kSlotsPerTask, 512, kGcmMinTask);
    } else if (kind == kPlanCp) {
        p = plan_tasks(lens, kCpTaskBytes, kCpWaves, kCpWaves, 2048);
    } else {
        uint64_t total = 0;
        for (uint64_t l : lens) total += l;
        const uint64_t per = crc_task_bytes(total);
        p.task_bytes = per;
        for (size_t i = 0; i < lens.size(); i++)
            for (uint64_t c0 = 0; c0 < lens[i]; c0 += per)
                p.tasks.push_back(Task{(uint32_t)i, 0, c0, std::min(c0 + per, lens[i])});
    }
    p.kind = kind;
    return p;
}

// The persistent transform kernels take tasks in array order: largest first,
// so that the last tasks handed out are short (slots stay per task).  A
// counting sort on 4 KiB units: O(n), on the host's critical path for every
// batch.  crc_segments_k is one workgroup per task (no queue): plan order.
void Plan::dispatch(Task *out) const {
    if (tasks.empty()) return;
    memcpy(out, tasks.data(), sizeof(Task) * tasks.size());
    if (kind == kPlanCrc) return;
#ifdef JFSX_ABLATE_TRACE
    for (size_t t = 0; t < tasks.size(); t++) out[t].trace = (uint32_t)t;
#endif
    order_largest_first(out, tasks.size(), (size_t)(kind == kPlanGcm ? kMaxTaskBytes : kCpTaskBytes) >> 12);
}

int check_aead_args(int algo, int n, const jfsx_blk *blks, int crc_mode, bool device) {
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;
    // NONE, GEN, VERIFY, GEN|CT, VERIFY|CT, GEN|BOTH
    if (crc_mode < 0 || (crc_mode & ~(3 | JFSX_CRC_CT | JFSX_CRC_BOTH)) || (crc_mode & 3) == 3 ||
        crc_mode == JFSX_CRC_CT || ((crc_mode & JFSX_CRC_BOTH) && crc_mode != (JFSX_CRC_GEN | JFSX_CRC_BOTH)) || n < 0)
        return JFSX_EINVAL;
    for (int i = 0; i < n; i++) {
        const jfsx_blk &b = blks[i];
        if (b.len && (!b.src || !b.dst)) return JFSX_EINVAL;
        if (device && b.len && (!aligned16(b.src) || !aligned16(b.dst))) return JFSX_EINVAL;
        // the ciphers' own limits: GCM's 32-bit counter runs from 2, so past
        // (2^32 - 2) blocks it would wrap onto J0 (the tag mask) -- Go's Seal
        // panics there (gcmMaxPlaintext); ChaCha20-Poly1305: the engine's own
        // limit of 2^32 - 1 Poly1305 blocks, below the cipher's (kCpMaxLen)
        if (algo == JFSX_AES256GCM && b.len > kGcmMaxLen) return JFSX_EINVAL;
        if (algo == JFSX_CHACHA20P1305 && b.len > kCpMaxLen) return JFSX_EINVAL;
        if (crc_mode && !b.crc) return JFSX_EINVAL;
    }
    return 0;
}

// Enqueue keysetup -> transform -> finalize -> result copy for n device-resident
// blocks on stream s, using workspace w.  Results land in w.h (BlkOut[n]) once
// the stream reaches that point; finish_aead() copies them into blks.
// Stages the batch's metadata and enqueues keysetup / main / finalize on s.
// Host ingest passes up = (s_in, ev): the metadata upload then rides the
// upload stream behind the data, ev is recorded there and s waits on it; with
// collect = false the caller downloads the BlkOut results on its own stream.
// The compute stream then carries kernels only, so the H2D and D2H DMA of
// neighbouring slots run concurrently (full duplex).
// host_crc: the blocks' CRC pointers are host arrays.  VERIFY arrays ride the
// descriptor upload (copied into the pinned mirror) and GEN arrays come back
// behind the BlkOut records in the same download, so a group of per-object
// blocks costs one small copy each way instead of one per block.
// With fin = (s_out, ev) the keysetup kernel also rides the upload stream
// (after the data and descriptors) and the finalize kernel runs on fin after
// ev marks the main kernel's end: the compute stream then carries only the
// main kernels, so a small batch's keysetup and finalize -- a few waves each,
// latency-bound -- overlap the neighbouring batches' main kernels instead of
// running between them.
// key_hook (jfsx_load_objects): called on the keysetup's stream between the
// descriptor upload and the keysetup kernel with the device KeyIn[n], for a
// caller whose keys are already in device memory (the blocks' key fields are
// then zero); null for everyone else.
using KeyHook = std::function<void(hipStream_t, KeyIn *)>;

// JFSX_KS_PHASES probe build (tools/taskedge_probe.py): where a device-resident
// batch's step goes outside the main kernel.  Host steady_clock stamps through
// enqueue_aead and run_aead, and events on the batch's stream around the
// upload, keysetup, the main kernel, finalize and the copy-back;
// jfsx_debug_edge_host reads them back.
#ifdef JFSX_KS_PHASES
struct EdgeHost {
    // seconds: enqueue_aead entered, planned, descriptors filled, tasks
    // dispatched, upload / keysetup / main / finalize and copy-back enqueued,
    // stream idle, results copied out
    double t[10] = {};
    hipEvent_t ev[7] = {};  // upload <, >, keysetup >, main <, >, finalize >, copy-back >
    bool have = false, ok = false;
};
EdgeHost g_edge;
inline double edge_now() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
#define EDGE_T(i) (g_edge.t[i] = edge_now())
#define EDGE_EV(i, st)                                       \
    do {                                                     \
        if (edge_on) (void)hipEventRecord(g_edge.ev[i], st); \
    } while (0)
#else
#define EDGE_T(i) ((void)0)
#define EDGE_EV(i, st) ((void)0)
#endif
int enqueue_aead(jfsx_ctx *c, Workspace &w, hipStream_t s, hipEvent_t k0, hipEvent_t k1, int algo, bool open, int n,
                 const jfsx_blk *blks, int crc_mode, hipStream_t up = nullptr, hipEvent_t up_ev = nullptr,
                 bool collect = true, hipStream_t fin = nullptr, hipEvent_t main_ev = nullptr,
                 bool host_crc = false, bool zc = false, hipStream_t ksst = nullptr, hipEvent_t ks_ev = nullptr,
                 const KeyHook *key_hook = nullptr) {
    const bool gcm = algo == JFSX_AES256GCM;
#ifdef JFSX_KS_PHASES
    // the plain device-resident call only: one stream, no pipeline
    const bool edge_on = !up && !fin && !zc && !ksst && collect;
    if (edge_on && !g_edge.have) {
        g_edge.have = true;
        for (hipEvent_t &e : g_edge.ev) (void)hipEventCreate(&e);
    }
    g_edge.ok = edge_on;
    EDGE_T(0);
#endif
    // JFSX_CRC_BOTH: the AEAD kernels checksum the plaintext (CRC_GEN) into the
    // first half of each CRC array and crc_segments_k checksums the ciphertext
    // in device memory into the second half -- before an in-place Open
    // overwrites it, after a Seal wrote it
    const bool both = (crc_mode & JFSX_CRC_BOTH) != 0;
    const int mult = both ? 2 : 1;
    crc_mode &= ~JFSX_CRC_BOTH;
    std::vector<uint64_t> lens(n);
    uint64_t crc_calc_words = 0, crc_words = 0;
    for (int i = 0; i < n; i++) {
        lens[i] = blks[i].len;
        if ((crc_mode & 3) == JFSX_CRC_VERIFY) crc_calc_words += nseg_of(blks[i].len);
        crc_words += mult * nseg_of(blks[i].len);
    }
    Plan cplan;  // the ciphertext pass (BOTH)
    if (both) cplan = plan_batch(kPlanCrc, lens);
    const std::vector<Task> &ctasks = cplan.tasks;
    const bool hc_in = host_crc && (crc_mode & 3) == JFSX_CRC_VERIFY;
    const bool hc_out = host_crc && (crc_mode & 3) == JFSX_CRC_GEN;
    const uint32_t slots = gcm ? kSlotsPerTask : kCpWaves;
    const Plan plan = plan_batch(gcm ? kPlanGcm : kPlanCp, lens);
    const size_t nt = plan.tasks.size();
    EDGE_T(1);
    // device workspace layout
    size_t off = 0;
    const size_t o_keys = off; off = align256(off + sizeof(KeyIn) * n);
    const size_t o_blk = off; off = align256(off + sizeof(BlkDev) * n);
    const size_t o_task = off; off = align256(off + sizeof(Task) * std::max<size_t>(nt, 1));
    const size_t o_tagin = off; off = align256(off + 16 * (size_t)n);
    const size_t o_queue = off; off = align256(off + 4);  // persistent kernel's task counter (uploaded as 0)
    const size_t o_crcin = off; if (hc_in) off = align256(off + 4 * crc_words);
    const size_t o_cblk = off; if (both) off = align256(off + sizeof(BlkDev) * n);
    const size_t o_ctask = off; if (both) off = align256(off + sizeof(Task) * std::max<size_t>(ctasks.size(), 1));
    const size_t h_bytes = off;  // everything above is uploaded from the pinned mirror
    const size_t o_out = off; off = align256(off + sizeof(BlkOut) * n);
    const size_t o_crcout = off; if (hc_out) off = align256(off + 4 * crc_words);
    const size_t down = hc_out ? o_crcout + 4 * crc_words - o_out : sizeof(BlkOut) * n;
    const size_t o_sched = off; off = align256(off + (gcm ? sizeof(GcmSched) : sizeof(CpSched)) * n);
    const size_t o_part = off; off = align256(off + 32 * std::max<uint64_t>(plan.nslots, 1));
    const size_t o_pexp = off; off = align256(off + 4 * std::max<uint64_t>(plan.nslots, 1));
    const size_t o_calc = off; off = align256(off + 4 * std::max<uint64_t>(crc_calc_words, 1));
    int rc;
    if ((rc = ensure_dev(c, &w.d, &w.dcap, off))) return rc;
    // zc: the results go straight to the pinned mirror, after the descriptors
    const size_t o_hres = zc ? h_bytes : 0;
    if ((rc = ensure_host(&w.h, &w.hcap, zc ? h_bytes + down : std::max(h_bytes, down)))) return rc;
    char *h = w.h, *d = w.d;
    KeyIn *hk = (KeyIn *)(h + o_keys);
    BlkDev *hb = (BlkDev *)(h + o_blk);
    *(uint32_t *)(h + o_queue) = 0;
    uint64_t calc = 0, cw = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_blk &b = blks[i];
        memcpy(hk[i].key, b.key, 32);
        memcpy(hk[i].nonce, b.nonce, 12);
        hk[i].pad = 0;
        hb[i].src = (const uint8_t *)b.src;
        hb[i].dst = (uint8_t *)b.dst;
        hb[i].len = b.len;
        hb[i].crc = b.crc;
        if (hc_in) {
            memcpy(h + o_crcin + 4 * cw, b.crc, 4 * nseg_of(b.len));
            hb[i].crc = (uint8_t *)(d + o_crcin + 4 * cw);
        } else if (hc_out) {
            hb[i].crc = zc ? (uint8_t *)(h + o_hres + (o_crcout - o_out) + 4 * cw) : (uint8_t *)(d + o_crcout + 4 * cw);
            if (zc && b.len == 0) memset(hb[i].crc, 0, 4 * mult);  // checksum() of nothing: one zero word
        }
        if (both) {
            BlkDev &cb = ((BlkDev *)(h + o_cblk))[i];
            memset(&cb, 0, sizeof(cb));
            cb.src = open ? hb[i].src : hb[i].dst;
            cb.len = b.len;
            cb.crc = hb[i].crc + 4 * nseg_of(b.len);
        }
        cw += mult * nseg_of(b.len);
        hb[i].crc_calc = nullptr;
        if ((crc_mode & 3) == JFSX_CRC_VERIFY) {
            hb[i].crc_calc = (uint32_t *)(d + o_calc) + calc;
            calc += nseg_of(b.len);
        }
        hb[i].slot0 = 0;
        hb[i].nslots = 0;
        hb[i].tag_in = open ? (const uint8_t *)(d + o_tagin + 16 * (size_t)i) : nullptr;
        memcpy(h + o_tagin + 16 * (size_t)i, b.tag, 16);
    }
    EDGE_T(2);
    uint32_t max_slots = 0;
    for (size_t t = 0; t < nt; t++) {
        BlkDev &bd = hb[plan.tasks[t].blk];
        if (bd.nslots == 0) bd.slot0 = plan.tasks[t].slot0;
        bd.nslots += slots;
        max_slots = std::max(max_slots, bd.nslots);
    }
    plan.dispatch((Task *)(h + o_task));
    cplan.dispatch((Task *)(h + o_ctask));
    EDGE_T(3);
    // the ciphertext pass of BOTH on stream st
    auto ct_pass = [&](hipStream_t st) {
        launch_crc_segments(st, (int)ctasks.size(), (const Task *)(d + o_ctask), (const BlkDev *)(d + o_cblk), c->tabs);
    };
    const KeyIn *dk = (const KeyIn *)(d + o_keys);
    const BlkDev *db = (const BlkDev *)(d + o_blk);
    const Task *dt = (const Task *)(d + o_task);
    uint32_t *dpart = (uint32_t *)(d + o_part);
    uint32_t *dpexp = (uint32_t *)(d + o_pexp);
    uint32_t *dq = (uint32_t *)(d + o_queue);
    BlkOut *dout = zc ? (BlkOut *)(h + o_hres) : (BlkOut *)(d + o_out);
    // keysetup on the upload stream when one is given (fin set), on the
    // keysetup stream ksst (with zc: the pull too) when given, else on s
    const bool kss = zc && ksst && ks_ev;
    hipStream_t ks = kss ? ksst : (up && fin) ? up : s, fs = fin ? fin : s;
    launch_begin();
    if (zc) {
        // the compute stream (or the keysetup stream) pulls the descriptors
        // out of the pinned mirror itself, so the upload stream carries only
        // the blocks' data
        launch_pull(kss ? ksst : s, d, h, h_bytes);
    } else {
        EDGE_EV(0, s);
        HIP_OK(hipMemcpyAsync(d, h, h_bytes, hipMemcpyHostToDevice, up ? up : s));
        EDGE_EV(1, s);
        EDGE_T(4);
    }
    // the compute stream waits for the upload before the first kernel that
    // reads what it carries: keysetup when the descriptors ride it, else main
    if (up && ks == s && !zc) {
        HIP_OK(hipEventRecord(up_ev, up));
        HIP_OK(hipStreamWaitEvent(s, up_ev, 0));
    }
    if (key_hook) (*key_hook)(ks, (KeyIn *)(d + o_keys));
    if (gcm) launch_gcm_keysetup(ks, n, dk, db, (GcmSched *)(d + o_sched), c->tabs, c->bitslice);
    else launch_cp_keysetup(ks, n, dk, db, (CpSched *)(d + o_sched));
    EDGE_EV(2, s);
    EDGE_T(5);
    if (kss) {  // the descriptors and schedules are ready for the compute stream
        HIP_OK(hipEventRecord(ks_ev, ksst));
        HIP_OK(hipStreamWaitEvent(s, ks_ev, 0));
    }
    if (up && (ks != s || zc)) {
        HIP_OK(hipEventRecord(up_ev, up));
        HIP_OK(hipStreamWaitEvent(s, up_ev, 0));
    }
    if ((crc_mode & 3) == JFSX_CRC_GEN && !(zc && hc_out))
        for (int i = 0; i < n; i++)
            if (blks[i].len == 0) HIP_OK(hipMemsetAsync(hb[i].crc, 0, 4 * mult, s));
    if (both && open) ct_pass(s);
    if (c->timing) HIP_OK(hipEventRecord(k0, s));
    EDGE_EV(3, s);
    if (gcm)
        launch_gcm_main(s, (int)nt, c->ncu, dq, open, crc_mode, c->bitslice, dt, db, (const GcmSched *)(d + o_sched),
                        dpart, dpexp, c->tabs, c->crc_l1);
    else
        launch_cp_main(s, (int)nt, c->ncu, dq, open, crc_mode, dt, db, (const CpSched *)(d + o_sched), dpart, dpexp,
                       c->tabs);
    EDGE_EV(4, s);
    EDGE_T(6);
    if (c->timing) HIP_OK(hipEventRecord(k1, s));
    if (both && !open) ct_pass(s);
    if (fin) {
        HIP_OK(hipEventRecord(main_ev, s));
        HIP_OK(hipStreamWaitEvent(fs, main_ev, 0));
    }
    if (gcm)
        launch_gcm_finalize(fs, n, open, crc_mode, db, (const GcmSched *)(d + o_sched), dpart, dpexp, dout, max_slots);
    else
        launch_cp_finalize(fs, n, open, crc_mode, db, (const CpSched *)(d + o_sched), dpart, dpexp, dout);
    HIP_OK(hipGetLastError());
    w.dout = dout;
    w.down = zc ? 0 : down;
    w.crc_off = o_crcout - o_out;
    w.crc_back = hc_out;
    w.crc_mult = mult;
    w.res_off = o_hres;
    EDGE_EV(5, s);
    if (collect && !zc) HIP_OK(hipMemcpyAsync(h, dout, down, hipMemcpyDeviceToHost, fs));
    EDGE_EV(6, s);
    EDGE_T(7);
    w.n = n;
    w.nt = nt;
    w.timed = c->timing;
    return 0;
}

// After the batch's stream work completed: per-block results into blks.
int finish_aead(jfsx_ctx *c, Workspace &w, hipEvent_t k0, hipEvent_t k1, bool open, jfsx_blk *blks) {
    if (w.timed && w.nt) {
        float ms = 0;
        w.timed = false;
        HIP_OK(hipEventElapsedTime(&ms, k0, k1));
        add_kernel_ms(c, ms);
    }
    const BlkOut *ho = (const BlkOut *)(w.h + w.res_off);
    for (int i = 0; i < w.n; i++) {
        jfsx_blk &b = blks[i];
        if (!open) memcpy(b.tag, ho[i].tag, 16);
        b.status = ho[i].status;
        b.crc_bad_seg = ho[i].bad_seg;
        b.crc_got = ho[i].got;
        b.crc_expect = ho[i].expect;
    }
    if (w.crc_back) {
        const char *hw = w.h + w.res_off + w.crc_off;
        for (int i = 0; i < w.n; i++) {
            const size_t cb = 4 * (size_t)w.crc_mult * nseg_of(blks[i].len);
            memcpy(blks[i].crc, hw, cb);
            hw += cb;
        }
        w.crc_back = false;
    }
    w.n = 0;
    w.nt = 0;
    return 0;
}

// Open releases nothing of a block whose tag failed: Go's in-place Open
// (encrypt.go:215; crypto/cipher gcm.go and x/crypto chacha20poly1305 both
// clear `out` on a mismatch) leaves zeros, and so does the engine -- dst, and
// a plaintext CRC_GEN array (it is a function of the unauthenticated
// plaintext).  Ciphertext CRCs (JFSX_CRC_CT) stay: the object checksum is
// checked before the tag (checksum.go:55-82).  Device memory: zeroed on s.
int wipe_failed(hipStream_t s, int n, const jfsx_blk *blks, int crc_mode, bool device) {
    const bool crc_pt = (crc_mode & 3) == JFSX_CRC_GEN && !(crc_mode & JFSX_CRC_CT);
    bool any = false;
    for (int i = 0; i < n; i++) {
        const jfsx_blk &b = blks[i];
        if (b.status != JFSX_ETAG) continue;
        any = true;
        if (device) {
            if (b.len) HIP_OK(hipMemsetAsync(b.dst, 0, b.len, s));
            if (crc_pt) HIP_OK(hipMemsetAsync(b.crc, 0, 4 * nseg_of(b.len), s));
        } else {
            if (b.len) memset(b.dst, 0, b.len);
            if (crc_pt) memset(b.crc, 0, 4 * nseg_of(b.len));
        }
    }
    if (any && device) HIP_OK(hipStreamSynchronize(s));
    return 0;
}

// Device-resident batch: one enqueue, one sync (under c->mu).
int run_aead(jfsx_ctx *c, int algo, bool open, int n, jfsx_blk *blks, int crc_mode) {
    int rc = check_aead_args(algo, n, blks, crc_mode, true);
    if (rc || n == 0) return rc;
    if ((rc = enqueue_aead(c, c->ws[0], c->stream, c->ev_k0[0], c->ev_k1[0], algo, open, n, blks, crc_mode))) {
        (void)hipStreamSynchronize(c->stream);  // nothing of this batch left in flight
        c->ws[0].timed = false;
        return rc;
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    EDGE_T(8);
    if ((rc = finish_aead(c, c->ws[0], c->ev_k0[0], c->ev_k1[0], open, blks))) return rc;
    EDGE_T(9);
    return open ? wipe_failed(c->stream, n, blks, crc_mode, true) : 0;
}

// staging bytes of one host block in a pipeline slot (its CRC array rides the
// slot's descriptor upload / result download instead)
inline size_t host_need(const jfsx_blk &b, int) { return align256(b.len); }

// The groups of a host batch: runs of blocks of up to slot_bytes; a batch
// smaller than a few slots is cut into about 6 groups (>= 16 MiB each) so that
// its own copies and transforms overlap too.
std::vector<std::pair<int, int>> host_groups(const jfsx_ctx *c, int n, const jfsx_blk *blks, int crc_mode) {
    std::vector<std::pair<int, int>> groups;  // [b0, b1)
    size_t total = 0;
    for (int i = 0; i < n; i++) total += host_need(blks[i], crc_mode);
    const size_t slot = std::min(c->slot_bytes.load(), std::max<size_t>((size_t)16 << 20, total / 6));
    int b0 = 0;
    size_t acc = 0;
    for (int i = 0; i < n; i++) {
        const size_t need = host_need(blks[i], crc_mode);
        if (i > b0 && acc + need > slot) {
            groups.push_back({b0, i});
            b0 = i;
            acc = 0;
        }
        acc += need;
    }
    groups.push_back({b0, n});
    return groups;
}

// Enqueue the CRC-only transform (crc_segments_k + crc_finalize_k) for n
// ranges of device memory, given as block records (src, len, crc), on stream
// s with workspace w: the counterpart of enqueue_aead for checksum() and the
// ReadAt verify (disk_cache.go:1218-1231, :1315-1327).  up / up_ev, collect,
// host_crc and zc mean what they mean for enqueue_aead: the host pipeline
// passes the data's upload stream, keeps the CRC arrays in the descriptor
// upload (VERIFY) and the result download (GEN), and lets the compute stream
// pull the descriptors out of the pinned mirror.
int enqueue_crc(jfsx_ctx *c, Workspace &w, hipStream_t s, hipEvent_t k0, hipEvent_t k1, int n, const jfsx_blk *blks,
                int mode, hipStream_t up = nullptr, hipEvent_t up_ev = nullptr, bool collect = true,
                bool host_crc = false, bool zc = false) {
    uint64_t calc_words = 0, crc_words = 0;
    std::vector<uint64_t> lens(n);
    for (int i = 0; i < n; i++) {
        lens[i] = blks[i].len;
        crc_words += nseg_of(blks[i].len);
        if (mode == JFSX_CRC_VERIFY) calc_words += nseg_of(blks[i].len);
    }
    const Plan plan = plan_batch(kPlanCrc, lens);
    const std::vector<Task> &tasks = plan.tasks;
    const bool hc_in = host_crc && mode == JFSX_CRC_VERIFY, hc_out = host_crc && mode == JFSX_CRC_GEN;
    const size_t nt = tasks.size();
    size_t off = 0;
    const size_t o_blk = off; off = align256(off + sizeof(BlkDev) * n);
    const size_t o_task = off; off = align256(off + sizeof(Task) * std::max<size_t>(nt, 1));
    const size_t o_crcin = off; if (hc_in) off = align256(off + 4 * crc_words);
    const size_t h_bytes = off;
    const size_t o_out = off; off = align256(off + sizeof(BlkOut) * n);
    const size_t o_crcout = off; if (hc_out) off = align256(off + 4 * crc_words);
    const size_t down = hc_out ? o_crcout + 4 * crc_words - o_out : sizeof(BlkOut) * n;
    const size_t o_calc = off; off = align256(off + 4 * std::max<uint64_t>(calc_words, 1));
    int rc;
    if ((rc = ensure_dev(c, &w.d, &w.dcap, off))) return rc;
    const size_t o_hres = zc ? h_bytes : 0;
    if ((rc = ensure_host(&w.h, &w.hcap, zc ? h_bytes + down : std::max(h_bytes, down)))) return rc;
    char *h = w.h, *d = w.d;
    BlkDev *hb = (BlkDev *)(h + o_blk);
    uint64_t calc = 0, cw = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_blk &b = blks[i];
        memset(&hb[i], 0, sizeof(BlkDev));
        hb[i].src = (const uint8_t *)b.src;
        hb[i].len = b.len;
        hb[i].crc = b.crc;
        if (hc_in) {
            memcpy(h + o_crcin + 4 * cw, b.crc, 4 * nseg_of(b.len));
            hb[i].crc = (uint8_t *)(d + o_crcin + 4 * cw);
        } else if (hc_out) {
            hb[i].crc = zc ? (uint8_t *)(h + o_hres + (o_crcout - o_out) + 4 * cw) : (uint8_t *)(d + o_crcout + 4 * cw);
        }
        cw += nseg_of(b.len);
        if (mode == JFSX_CRC_VERIFY) {
            hb[i].crc_calc = (uint32_t *)(d + o_calc) + calc;
            calc += nseg_of(b.len);
        }
    }
    plan.dispatch((Task *)(h + o_task));
    BlkOut *dout = zc ? (BlkOut *)(h + o_hres) : (BlkOut *)(d + o_out);
    launch_begin();
    if (zc) launch_pull(s, d, h, h_bytes);
    else HIP_OK(hipMemcpyAsync(d, h, h_bytes, hipMemcpyHostToDevice, up ? up : s));
    if (up) {
        HIP_OK(hipEventRecord(up_ev, up));
        HIP_OK(hipStreamWaitEvent(s, up_ev, 0));
    }
    if (c->timing) HIP_OK(hipEventRecord(k0, s));
    launch_crc_segments(s, (int)nt, (const Task *)(d + o_task), (const BlkDev *)(d + o_blk), c->tabs);
    if (c->timing) HIP_OK(hipEventRecord(k1, s));
    launch_crc_finalize(s, n, mode, (const BlkDev *)(d + o_blk), dout);
    HIP_OK(hipGetLastError());
    w.dout = dout;
    w.down = zc ? 0 : down;
    w.crc_off = o_crcout - o_out;
    w.crc_back = hc_out;
    w.crc_mult = 1;
    w.res_off = o_hres;
    if (collect && !zc) HIP_OK(hipMemcpyAsync(h, dout, down, hipMemcpyDeviceToHost, s));
    w.n = n;
    w.nt = nt;
    w.timed = c->timing;
    return 0;
}

// How a host thread waits for a pipeline slot's D2H (JFSX_WAIT_POLL_US): by
// default it queries the event and sleeps 20 us between queries; 0 =
// hipEventSynchronize, the runtime's wait, which keeps a core busy for the
// whole wait (with or without hipEventBlockingSync).  A group's wait is about
// a millisecond and several dispatchers wait at once: 20 per-object callers on
// pinned blocks kept 5.0 cores busy with the runtime's wait and 1.25 with the
// sleeping one, at the same 41.6-41.9 GB/s (profiles/r6/wait_poll/).
int wait_poll_us() {
    static const int v = [] {
        const char *e = getenv("JFSX_WAIT_POLL_US");
        return e ? atoi(e) : 20;
    }();
    return v;
}

hipError_t wait_event(hipEvent_t ev) {
    const int us = wait_poll_us();
    if (us <= 0) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        (void)hipGetLastError();  // hipErrorNotReady is not a failure
        std::this_thread::sleep_for(std::chrono::microseconds(us));
    }
}

// Collect the group in flight in slot s (s.mu held; called by the group's own
// caller, or by any caller that needs the slot next): wait for its D2H and
// write its per-block results into the owner's records.  Only results: the
// owner copies its bounced outputs out itself.
void pipe_collect(jfsx_ctx *c, PipeSlot &s) {
    PipeGroup *g = s.owner;
    if (!g) return;
    s.owner = nullptr;
    const hipError_t e = wait_event(s.ev_out);
    if (e != hipSuccess) {
        note_hip_error(e, __FILE__, __LINE__, "hipEventSynchronize(pipeline slot)");
        g->rc = JFSX_EIO;
        s.w.crc_back = false;
        s.w.n = 0;
        s.w.nt = 0;
        s.w.timed = false;
        return;
    }
    g->rc = finish_aead(c, s.w, s.ev_k0, s.ev_k1, g->open, g->dv);
}

// The host pipeline's metadata path: with it (the default) the compute stream
// pulls each group's descriptors out of the pinned mirror with a small kernel
// and finalize writes the per-block results (and GEN CRC words) straight into
// it, so the copy streams carry only block data -- small copies on them run as
// blit kernels between the SDMA transfers.  JFSX_PIPE_META=copy restores the
// metadata copies.
bool zero_copy_meta() {
    static const bool v = [] {
        const char *e = getenv("JFSX_PIPE_META");
        return !(e && !strcmp(e, "copy"));
    }();
    return v;
}

// The host pipeline's keysetup stream (JFSX_KS_STREAM, default on): each
// group's descriptor pull and keysetup kernel run on a fourth stream, so they
// overlap the previous group's main kernel instead of queueing behind it on
// the compute stream (the compute stream waits for them before the main
// kernel).  For a group of a few small blocks keysetup is most of the
// compute stream's time (54 us of 137 per group of 64 KiB blocks, rocprof).
bool ks_stream() {
    static const bool v = [] {
        const char *e = getenv("JFSX_KS_STREAM");
        return !(e && !strcmp(e, "0"));
    }();
    return v;
}

enum PipeOp { kPipeSeal, kPipeOpen, kPipeCrc };

// One group into an empty slot (s.mu and c->mu held): the blocks' data runs up
// on s_in into the slot's staging (coalesced where the blocks are adjacent in
// host memory -- a group's bounced blocks always are), then the transform on
// the compute stream (AEAD: keysetup / main / finalize; CRC: crc_segments /
// crc_finalize); the AEAD outputs run down on s_out, chained by the slot's
// events.  blks hold page-locked host addresses only (run_host substituted the
// bounce buffer for pageable ones); dv[i] (the call's copy of the caller's
// record) is pointed at the staging copy.  (A variant whose kernel wrote the
// outputs straight into engine-pinned caller memory over PCIe ran at 25 GB/s
// against 38.7 staged and was removed.)
int pipe_enqueue(jfsx_ctx *c, PipeSlot &s, PipeOp op, int algo, int nb, const jfsx_blk *blks, jfsx_blk *dv,
                 int crc_mode, const uintptr_t *in_id, const uintptr_t *out_id) {
    Workspace &w = s.w;
    size_t need = 0;
    for (int i = 0; i < nb; i++) need += host_need(blks[i], crc_mode);
    int rc;
    if ((rc = ensure_dev(c, &w.stage, &w.scap, std::max<size_t>(need, 256)))) return rc;
    size_t off = 0;
    // staging in the order of the source addresses: blocks that are
    // neighbours in host memory (pages of one pinned pool, or one bounce
    // buffer) then sit side by side in staging too, and their copies coalesce
    // both ways whatever order the callers submitted them in
    std::vector<int> ord(nb);
    for (int i = 0; i < nb; i++) ord[i] = i;
    if (nb > 1)
        std::stable_sort(ord.begin(), ord.end(),
                         [&](int a, int b) { return (uintptr_t)blks[a].src < (uintptr_t)blks[b].src; });
    const char *run_h = nullptr;
    char *run_d = nullptr;
    size_t run_n = 0;
    uintptr_t run_id = 0;
    auto flush_in = [&]() -> int {
        if (run_n) {
            HIP_OK(hipMemcpyAsync(run_d, run_h, run_n, hipMemcpyHostToDevice, c->s_in));
            c->ps_h2d++;
        }
        run_n = 0;
        return 0;
    };
    for (int k = 0; k < nb; k++) {
        const int i = ord[k];
        char *buf = w.stage + off;
        off += align256(blks[i].len);
        if (blks[i].len) {
            const char *hs = (const char *)blks[i].src;
            // one copy may only span one host allocation (a pinned pool, a
            // bounce buffer): in_id names the allocation, 0 = the block's own
            if (!(run_n && run_h + run_n == hs && run_d + run_n == buf && in_id[i] && in_id[i] == run_id) &&
                (rc = flush_in()))
                return rc;
            if (!run_n) {
                run_h = hs;
                run_d = buf;
                run_id = in_id[i];
            }
            run_n += blks[i].len;
            if (align256(blks[i].len) != blks[i].len && (rc = flush_in())) return rc;
        }
        dv[i].src = buf;
        dv[i].dst = op == kPipeCrc ? nullptr : buf;
    }
    if ((rc = flush_in())) return rc;
    // the transform on the compute stream.  (Moving keysetup onto s_in and
    // finalize onto s_out, to overlap them with neighbouring groups' main
    // kernels, measured 30-33 GB/s against 38-40 at 20 per-object callers:
    // the copy engines then wait behind those kernels.)  The CRC arrays pass
    // through the descriptor upload and the result download (host_crc).
    if (op == kPipeCrc)
        rc = enqueue_crc(c, w, c->stream, s.ev_k0, s.ev_k1, nb, dv, crc_mode, c->s_in, s.ev_in, false, true,
                         zero_copy_meta());
    else
        rc = enqueue_aead(c, w, c->stream, s.ev_k0, s.ev_k1, algo, op == kPipeOpen, nb, dv, crc_mode, c->s_in,
                          s.ev_in, false, nullptr, nullptr, true, zero_copy_meta(), ks_stream() ? c->s_ks : nullptr,
                          s.ev_ks);
    if (rc) return rc;
    HIP_OK(hipEventRecord(s.ev_comp, c->stream));
    HIP_OK(hipStreamWaitEvent(c->s_out, s.ev_comp, 0));
    char *oh = nullptr;
    const char *od = nullptr;
    size_t on = 0;
    uintptr_t oid = 0;
    auto flush_out = [&]() -> int {
        if (on) {
            HIP_OK(hipMemcpyAsync(oh, od, on, hipMemcpyDeviceToHost, c->s_out));
            c->ps_d2h++;
        }
        on = 0;
        return 0;
    };
    for (int k = 0; k < nb && op != kPipeCrc; k++) {
        const int i = ord[k];
        if (!blks[i].len) continue;
        char *hd = (char *)blks[i].dst;
        const char *dd = (const char *)dv[i].dst;
        if (!(on && oh + on == hd && od + on == dd && out_id[i] && out_id[i] == oid) && (rc = flush_out())) return rc;
        if (!on) {
            oh = hd;
            od = dd;
            oid = out_id[i];
        }
        on += blks[i].len;
        if (align256(blks[i].len) != blks[i].len && (rc = flush_out())) return rc;
    }
    if ((rc = flush_out())) return rc;
    if (w.down) HIP_OK(hipMemcpyAsync(w.h, w.dout, w.down, hipMemcpyDeviceToHost, c->s_out));
    HIP_OK(hipEventRecord(s.ev_out, c->s_out));
    return 0;
}

// A pipeline slot for the next group, locked.  Under c->mu only the choice is
// made: the first slot from the ring position on that is unlocked and whose
// group (if any) has finished its D2H, else the next slot in ring order.  The
// wait for a busy slot then happens under that slot's lock alone, so a caller
// waiting for another caller's group holds up nothing else on the context
// (device batches, CRC and codec calls, other callers' enqueues).
PipeSlot *claim_slot(jfsx_ctx *c) {
    PipeSlot *s = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        for (int k = 0; k < kPipe && !s; k++) {
            PipeSlot &q = c->pipe[(c->pipe_next + k) % kPipe];
            if (!q.mu.try_lock()) continue;
            bool idle = !q.owner;
            if (!idle) {
                idle = hipEventQuery(q.ev_out) == hipSuccess;
                (void)hipGetLastError();  // hipErrorNotReady is not a failure of this call
            }
            if (idle) {
                s = &q;
                c->pipe_next = (c->pipe_next + k + 1) % kPipe;
            } else {
                q.mu.unlock();
            }
        }
        if (s) return s;
        s = &c->pipe[c->pipe_next];
        c->pipe_next = (c->pipe_next + 1) % kPipe;
    }
    s->mu.lock();
    return s;
}

// bounce buffers: capacity classes of 1 MiB up to 16 MiB, then 16 MiB
size_t bounce_class(size_t need) {
    const size_t mib = (size_t)1 << 20, step = need <= 16 * mib ? mib : 16 * mib;
    return (std::max<size_t>(need, 1) + step - 1) / step * step;
}

// idle buffers kept per context (JFSX_BOUNCE_RETAIN_MB, default 1 GiB)
size_t bounce_retain() {
    static const size_t v = [] {
        const char *e = getenv("JFSX_BOUNCE_RETAIN_MB");
        return (e ? (size_t)atoll(e) : (size_t)1024) << 20;
    }();
    return v;
}

int alloc_pinned_on(int node, size_t bytes, void **p);

char *bounce_get(jfsx_ctx *c, size_t need, size_t *cap) {
    BouncePool &b = c->bounce;
    {
        std::lock_guard<std::mutex> g(b.mu);
        auto it = b.idle.lower_bound(need);
        if (it != b.idle.end() && it->first <= std::max(2 * need, need + ((size_t)1 << 20))) {
            char *p = it->second;
            *cap = it->first;
            b.idle_bytes -= it->first;
            b.idle.erase(it);
            return p;
        }
    }
    const size_t n = bounce_class(need);
    void *p = nullptr;
    if (alloc_pinned_on(c->numa_node, n, &p)) return nullptr;
    note_pinned(p, n);  // so host_pinned() knows a bounced block at once
    b.allocs++;
    *cap = n;
    return (char *)p;
}

// Back to the idle list.  Over the retention cap the largest idle buffers go
// first, so one big pageable host-ingest call's buffers do not crowd out the
// per-object ones (which would then be allocated and freed on every call).
void bounce_put(jfsx_ctx *c, char *p, size_t cap) {
    BouncePool &b = c->bounce;
    std::vector<char *> drop;
    {
        std::lock_guard<std::mutex> g(b.mu);
        b.idle.emplace(cap, p);
        b.idle_bytes += cap;
        while (b.idle_bytes > bounce_retain() && !b.idle.empty()) {
            auto it = std::prev(b.idle.end());
            b.idle_bytes -= it->first;
            drop.push_back(it->second);
            b.idle.erase(it);
        }
    }
    for (char *q : drop) {
        forget_pinned(q);
        (void)hipHostFree(q);
    }
}

}  // namespace

namespace jfsx {
// the aggregator stages pageable per-object requests on the calling thread
// with these (jfsx_agg.cpp)
char *bounce_acquire(jfsx_ctx *c, size_t need, size_t *cap) {
    CtxScope es_(c);
    (void)hipSetDevice(c->device);
    return bounce_get(c, need, cap);
}
void bounce_release(jfsx_ctx *c, char *p, size_t cap) { bounce_put(c, p, cap); }
void bounce_count(jfsx_ctx *c, uint64_t in, uint64_t out) {
    c->bounce.bytes_in += in;
    c->bounce.bytes_out += out;
}
}  // namespace jfsx

namespace {

// memcpy of a group's blocks into / out of its bounce buffer: on the calling
// thread (each per-object caller copies its own block, so max-uploads callers
// copy in parallel); one caller's big group (a host-ingest batch from pageable
// memory) is split over helper threads so the host copy keeps up with PCIe
int copy_threads() {  // JFSX_COPY_THREADS (default 8)
    static const int v = [] {
        const char *e = getenv("JFSX_COPY_THREADS");
        const int t = e ? atoi(e) : 8;
        return t >= 1 && t <= 64 ? t : 8;
    }();
    return v;
}

void par_copy(std::vector<std::pair<char *, const char *>> &ds, const std::vector<size_t> &lens) {
    size_t total = 0;
    for (size_t l : lens) total += l;
    const size_t mib = (size_t)1 << 20;
    const int nt = total >= 32 * mib ? (int)std::min<size_t>((size_t)copy_threads(), total / (8 * mib)) : 1;
    // bytes [lo, hi) of the concatenated items
    auto work = [&](size_t lo, size_t hi) {
        size_t base = 0;
        for (size_t k = 0; k < ds.size() && base < hi; base += lens[k], k++) {
            const size_t a = std::max(lo, base), b = std::min(hi, base + lens[k]);
            if (a < b) memcpy(ds[k].first + (a - base), ds[k].second + (a - base), b - a);
        }
    };
    if (nt <= 1) {
        work(0, total);
        return;
    }
    std::vector<std::thread> ts;
    for (int t = 1; t < nt; t++) ts.emplace_back(work, total * t / nt, total * (t + 1) / nt);
    work(0, total / nt);
    for (std::thread &t : ts) t.join();
}

// Host staging of the one-call paths (load, load_objects, store, store_objects,
// gather, and the upload of the ranged Open).  A caller's buffer that is
// page-locked is copied by DMA where it lies; a pageable one goes through one
// pinned bounce buffer that serves both directions: the stream has finished
// the uploads out of it before it reaches the downloads into it.  The rule of
// a direction: when every classified buffer of it is pageable the buffer is
// filled (or emptied) packed and crosses PCIe in one copy of the packed span;
// otherwise every non-empty item crosses in a copy of its own, from (to) its
// place in the bounce buffer or the caller's memory.
// A path classifies (mark) what it may transfer, takes the buffer (reserve)
// before its first enqueue, and names the items of a transfer when it
// enqueues it.  The object outlives the call's last stream wait: the buffer
// goes back to the pool when it dies.
struct StageItem {
    void *host;  // the caller's buffer
    char *dev;   // its place in device memory
    size_t off;  // its place in the bounce buffer (packed: dev is the span's start + off)
    size_t len;
    size_t idx;  // its index in the direction's classification
};

struct HostStage {
    struct Dir {
        std::vector<char> bounced;  // per index; an index never marked (an empty buffer) counts in neither flag
        bool all = true, any = false;
    };
    Dir in, out;

    HostStage() = default;
    HostStage(const HostStage &) = delete;
    HostStage &operator=(const HostStage &) = delete;
    ~HostStage() {
        if (pool_) bounce_put(pool_, buf_, cap_);
    }

    void resize(size_t n_in, size_t n_out) {
        in.bounced.assign(n_in, 0);
        out.bounced.assign(n_out, 0);
    }
    static void mark(Dir &d, size_t i, const void *p, size_t len) {
        const bool b = !host_pinned(p, len);
        d.bounced[i] = b;
        d.all = d.all && b;
        d.any = d.any || b;
    }
    size_t need(size_t up, size_t down) const { return std::max(in.any ? up : 0, out.any ? down : 0); }
    // the pool's buffer for the packed spans of both directions
    int reserve(jfsx_ctx *c, size_t up, size_t down) {
        const size_t n = need(up, down);
        if (!n) return 0;
        if (!(buf_ = bounce_get(c, n, &cap_))) return JFSX_ENOMEM;
        pool_ = c;
        return 0;
    }
    // a buffer of the caller's, of need() bytes, instead: it stays the caller's and no bounce bytes are counted
    void lend(char *buf) { buf_ = buf; }

    int upload(hipStream_t s, char *dev, size_t span, const std::vector<StageItem> &items) {
        copy(items, in, true);
        if (in.all && span) {
            HIP_OK(hipMemcpyAsync(dev, buf_, span, hipMemcpyHostToDevice, s));
            return 0;
        }
        for (const StageItem &it : items)
            if (it.len)
                HIP_OK(hipMemcpyAsync(it.dev, in.bounced[it.idx] ? buf_ + it.off : (const char *)it.host, it.len,
                                      hipMemcpyHostToDevice, s));
        return 0;
    }
    // span 0: the items do not lie packed in device memory, every one is copied by itself
    int download(hipStream_t s, const char *dev, size_t span, std::vector<StageItem> items) {
        down_ = std::move(items);
        if (out.all && span) {
            HIP_OK(hipMemcpyAsync(buf_, dev, span, hipMemcpyDeviceToHost, s));
            return 0;
        }
        for (const StageItem &it : down_)
            if (it.len)
                HIP_OK(hipMemcpyAsync(out.bounced[it.idx] ? buf_ + it.off : (char *)it.host, it.dev, it.len,
                                      hipMemcpyDeviceToHost, s));
        return 0;
    }
    // after the wait of a call that succeeded: the bounced items of download() to the caller
    void copy_out() { copy(down_, out, false); }

  private:
    void copy(const std::vector<StageItem> &items, const Dir &d, bool up) {
        std::vector<std::pair<char *, const char *>> cp;
        std::vector<size_t> cl;
        for (const StageItem &it : items) {
            if (!it.len || !d.bounced[it.idx]) continue;
            if (up) cp.push_back({buf_ + it.off, (const char *)it.host});
            else cp.push_back({(char *)it.host, buf_ + it.off});
            cl.push_back(it.len);
            if (pool_) (up ? pool_->bounce.bytes_in : pool_->bounce.bytes_out) += it.len;
        }
        par_copy(cp, cl);
    }
    char *buf_ = nullptr;
    size_t cap_ = 0;
    jfsx_ctx *pool_ = nullptr;  // the context whose pool buf_ goes back to
    std::vector<StageItem> down_;
};

// The wait that ends a phase of a call, whatever its enqueue returned, so that
// a failure leaves nothing in flight: a stream error becomes JFSX_EIO unless
// an earlier error stands.
int wait_stream(jfsx_ctx *c, int rc, const char *what) {
    const hipError_t se = hipStreamSynchronize(c->stream);
    if (!rc && se != hipSuccess) {
        note_hip_error(se, __FILE__, __LINE__, what);
        rc = JFSX_EIO;
    }
    return rc;
}

void add_elapsed_ms(jfsx_ctx *c, hipEvent_t ev0, hipEvent_t ev1) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) add_kernel_ms(c, ms);
    else (void)hipGetLastError();
}

// After a call's last wait: the main-kernel time of a stage that was timed
// (ok: the call succeeded), and its workspace free for the next call.
void settle_stage(jfsx_ctx *c, Workspace &w, hipEvent_t ev0, hipEvent_t ev1, bool ok) {
    if (ok && w.timed && w.nt) add_elapsed_ms(c, ev0, ev1);
    w.n = 0;
    w.nt = 0;
    w.timed = false;
    w.crc_back = false;
}

// Host-memory call (host ingest, the per-object shim, checksum() / ReadAt
// verify on host memory).  The call is cut into groups; for each group the
// calling thread (1) copies its pageable blocks into a bounce buffer, (2)
// claims a pipeline slot, collects whatever group still occupies it, (3)
// enqueues the group under c->mu and moves on.  It then waits for its own
// groups' D2H events only, copying each group's bounced outputs out as it
// completes (after at most a few groups in flight, when it holds bounce
// buffers, so one big pageable call pins no more than that).  So concurrent
// callers keep the H2D and D2H engines busy back to back instead of filling
// and draining the ring once per call.  Open releases no plaintext of a block
// whose tag failed: its destination is wiped before the call returns.  On an
// enqueue error the three streams are drained first, so an error return means
// nothing of the call is still copying into the caller's buffers.
int run_host(jfsx_ctx *c, PipeOp op, int algo, int n, jfsx_blk *blks, int crc_mode) {
    int rc = 0;
    const bool open = op == kPipeOpen;
    const std::vector<std::pair<int, int>> groups = host_groups(c, n, blks, crc_mode);
    std::vector<jfsx_blk> dv(blks, blks + n), hv(blks, blks + n);
    std::vector<char> out_b(n, 0);  // block i's output sits in the bounce buffer
    // the host allocation of each block's source / destination copy, for
    // coalescing (pinned_base; the bounce buffer; 0: copy the block alone)
    std::vector<uintptr_t> in_id(n, 0), out_id(n, 0);
    std::vector<PipeGroup> recs(groups.size());
    size_t issued = 0, done = 0, held = 0;  // groups enqueued / finished; bounce bytes held
    size_t pinned_held = 0;                 // caller ranges pinned by groups in flight
    using SClock = std::chrono::steady_clock;
    auto us = [](SClock::time_point a, SClock::time_point b) {
        return (uint64_t)std::chrono::duration_cast<std::chrono::microseconds>(b - a).count();
    };
    std::vector<std::pair<char *, const char *>> cp;
    std::vector<size_t> cl;
    // wait for group g, copy its bounced outputs out, release its bounce buffer
    auto finish = [&](size_t g) {
        PipeGroup &r = recs[g];
        const SClock::time_point f0 = SClock::now();
        {
            std::lock_guard<std::mutex> sl(r.slot->mu);
            if (r.slot->owner == &r) pipe_collect(c, *r.slot);
        }
        const SClock::time_point f1 = SClock::now();
        c->ps_wait_us += us(f0, f1);
        if (!r.rc) {
            cp.clear();
            cl.clear();
            for (int i = groups[g].first; i < groups[g].second; i++)
                if (out_b[i] && !(open && dv[i].status == JFSX_ETAG)) {
                    cp.push_back({(char *)blks[i].dst, (const char *)hv[i].dst});
                    cl.push_back(blks[i].len);
                    c->bounce.bytes_out += blks[i].len;
                }
            par_copy(cp, cl);
            c->ps_bout_us += us(f1, SClock::now());
        }
        if (r.bounce) {
            bounce_put(c, r.bounce, r.bcap);
            held -= r.bcap;
            r.bounce = nullptr;
        }
        for (const void *q : r.pins) host_unpin(q);
        r.pins.clear();
        if (r.rc && !rc) rc = r.rc;
    };
    for (size_t g = 0; g < groups.size() && !rc; g++) {
        const int b0 = groups[g].first, b1 = groups[g].second;
        PipeGroup &r = recs[g];
        // (1) bounce the group's pageable blocks: one region per block, used
        // by its input (copied in here) and / or its output (copied out by
        // finish); in place when src == dst
        const SClock::time_point p0 = SClock::now();
        size_t need = 0;
        std::vector<size_t> boff(b1 - b0, SIZE_MAX);
        std::vector<char> in_pg(b1 - b0, 0);
        for (int i = b0; i < b1; i++) {
            const jfsx_blk &b = blks[i];
            if (!b.len) continue;
            in_pg[i - b0] = !host_pinned(b.src, b.len);
            out_b[i] = op != kPipeCrc && (b.dst == b.src ? in_pg[i - b0] : !host_pinned(b.dst, b.len));
            // pin the caller's own pages for the call where the runtime
            // allows it; what stays unpinned is bounced
            if (in_pg[i - b0] && host_pin(b.src, b.len)) {
                r.pins.push_back(b.src);
                in_pg[i - b0] = 0;
                if (b.dst == b.src) out_b[i] = 0;
            }
            if (out_b[i] && host_pin(b.dst, b.len)) {
                r.pins.push_back(b.dst);
                out_b[i] = 0;
            }
            in_id[i] = pinned_base(b.src);
            out_id[i] = op == kPipeCrc ? 0 : pinned_base(b.dst);
            if (!in_pg[i - b0] && !out_b[i]) continue;
            boff[i - b0] = need;
            need += align256(b.len);
        }
        const SClock::time_point p1 = SClock::now();
        c->ps_pin_us += us(p0, p1);
        if (need) {
            if (!(r.bounce = bounce_get(c, need, &r.bcap))) {
                for (const void *q : r.pins) host_unpin(q);
                r.pins.clear();
                rc = JFSX_ENOMEM;
                break;
            }
            held += r.bcap;
            cp.clear();
            cl.clear();
            for (int i = b0; i < b1; i++) {
                if (boff[i - b0] == SIZE_MAX) continue;
                char *q = r.bounce + boff[i - b0];
                if (in_pg[i - b0]) {
                    cp.push_back({q, (const char *)blks[i].src});
                    cl.push_back(blks[i].len);
                    hv[i].src = q;
                    in_id[i] = (uintptr_t)r.bounce;
                    c->bounce.bytes_in += blks[i].len;
                }
                if (out_b[i]) {
                    hv[i].dst = q;
                    out_id[i] = (uintptr_t)r.bounce;
                }
            }
            par_copy(cp, cl);
            c->ps_bin_us += us(p1, SClock::now());
        }
        // (2) a slot, (3) the enqueue
        const SClock::time_point t0 = SClock::now();
        PipeSlot &s = *claim_slot(c);
        pipe_collect(c, s);
        const SClock::time_point t1 = SClock::now();
        {
            std::lock_guard<std::mutex> lk(c->mu);
            rc = pipe_enqueue(c, s, op, algo, b1 - b0, hv.data() + b0, dv.data() + b0, crc_mode, in_id.data() + b0,
                              out_id.data() + b0);
            if (rc) {
                (void)hipStreamSynchronize(c->s_in);
                (void)hipStreamSynchronize(c->stream);
                (void)hipStreamSynchronize(c->s_out);
                s.w.n = 0;
                s.w.nt = 0;
                s.w.timed = false;
                s.w.crc_back = false;
            }
        }
        c->ps_slot_us += us(t0, t1);
        c->ps_enq_us += us(t1, SClock::now());
        c->ps_groups++;
        c->ps_blocks += (uint64_t)(b1 - b0);
        if (rc) {
            s.mu.unlock();
            if (r.bounce) {
                bounce_put(c, r.bounce, r.bcap);
                held -= r.bcap;
                r.bounce = nullptr;
            }
            for (const void *q : r.pins) host_unpin(q);
            r.pins.clear();
            break;
        }
        r.slot = &s;
        r.dv = dv.data() + b0;
        r.open = open;
        s.owner = &r;
        s.mu.unlock();
        issued++;
        // a call holding bounce buffers or pinned caller pages keeps at most
        // 4 groups / 1 GiB of them in flight
        pinned_held += r.pins.size();
        while ((held || pinned_held) && (issued - done > 4 || held > ((size_t)1 << 30))) {
            pinned_held -= recs[done].pins.size();
            finish(done++);
        }
    }
    const SClock::time_point tw = SClock::now();
    while (done < issued) finish(done++);
    c->ps_own_us += us(tw, SClock::now());
    if (rc) return rc;
    for (int i = 0; i < n; i++) {
        blks[i].status = dv[i].status;
        blks[i].crc_bad_seg = dv[i].crc_bad_seg;
        blks[i].crc_got = dv[i].crc_got;
        blks[i].crc_expect = dv[i].crc_expect;
        if (op != kPipeOpen && op != kPipeCrc) memcpy(blks[i].tag, dv[i].tag, 16);
    }
    return open ? wipe_failed(c->stream, n, blks, crc_mode, false) : 0;
}

int run_aead_host(jfsx_ctx *c, int algo, bool open, int n, jfsx_blk *blks, int crc_mode) {
    int rc = check_aead_args(algo, n, blks, crc_mode, false);
    if (rc || n == 0) return rc;
    return run_host(c, open ? kPipeOpen : kPipeSeal, algo, n, blks, crc_mode);
}

int check_crc_args(int n, const jfsx_range *r, int mode, bool device) {
    if (n < 0 || (mode != JFSX_CRC_GEN && mode != JFSX_CRC_VERIFY)) return JFSX_EINVAL;
    for (int i = 0; i < n; i++) {
        if (r[i].len && (!r[i].data || (device && !aligned16(r[i].data)))) return JFSX_EINVAL;
        if (!r[i].crc) return JFSX_EINVAL;
    }
    return 0;
}

// ranges as the block records the pipeline and enqueue_crc take
std::vector<jfsx_blk> ranges_as_blocks(int n, const jfsx_range *r) {
    std::vector<jfsx_blk> b(n);
    for (int i = 0; i < n; i++) {
        memset(&b[i], 0, sizeof(jfsx_blk));
        b[i].src = r[i].data;
        b[i].len = r[i].len;
        b[i].crc = r[i].crc;
    }
    return b;
}

void blocks_to_ranges(int n, const jfsx_blk *b, jfsx_range *r) {
    for (int i = 0; i < n; i++) {
        r[i].status = b[i].status;
        r[i].bad_seg = b[i].crc_bad_seg;
        r[i].got = b[i].crc_got;
        r[i].expect = b[i].crc_expect;
    }
}

// Device-memory CRC batch: one enqueue, one sync (under c->mu).
int run_crc(jfsx_ctx *c, int n, jfsx_range *r, int mode) {
    int rc = check_crc_args(n, r, mode, true);
    if (rc || n == 0) return rc;
    std::vector<jfsx_blk> b = ranges_as_blocks(n, r);
    if ((rc = enqueue_crc(c, c->ws[0], c->stream, c->ev_k0[0], c->ev_k1[0], n, b.data(), mode))) {
        (void)hipStreamSynchronize(c->stream);
        c->ws[0].timed = false;
        return rc;
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    if ((rc = finish_aead(c, c->ws[0], c->ev_k0[0], c->ev_k1[0], true, b.data()))) return rc;
    blocks_to_ranges(n, b.data(), r);
    return 0;
}

// Host-memory CRC call: through the host pipeline, like a host AEAD call (no
// context lock held while it waits; pageable ranges bounced by the caller).
int run_crc_host(jfsx_ctx *c, int n, jfsx_range *r, int mode) {
    int rc = check_crc_args(n, r, mode, false);
    if (rc || n == 0) return rc;
    std::vector<jfsx_blk> b = ranges_as_blocks(n, r);
    if ((rc = run_host(c, kPipeCrc, 0, n, b.data(), mode))) return rc;
    blocks_to_ranges(n, b.data(), r);
    return 0;
}

constexpr uint64_t kLz4MaxInput = 0x7E000000ull;  // LZ4_MAX_INPUT_SIZE
uint64_t lz4_bound(uint64_t n) { return n > kLz4MaxInput ? 0 : n + n / 255 + 16; }
// ZSTD_compressBound
uint64_t zstd_bound(uint64_t n) { return n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0); }

enum CodecOp { kLz4Comp, kLz4Decomp, kZstdDecomp, kZstdComp };

// Waves of the zstd decoder for a batch of n objects (run_codec and run_load):
// block-parallel persistent waves unless JFSX_ZSTD_SERIAL=1 selects the
// one-wave-per-object serial kernel (A/B; 0 = serial).  The waves are capped by
// the context's arena budget (a 64-object batch needs 64 arenas, not 8 per CU).
int zstd_decode_waves(const jfsx_ctx *c, int n) {
    static const bool zd_serial = getenv("JFSX_ZSTD_SERIAL") && atoi(getenv("JFSX_ZSTD_SERIAL")) == 1;
    int waves = !zd_serial ? zstd_par_waves(n, c->ncu) : 0;
    if (waves) waves = (int)std::min<size_t>((size_t)waves, std::max<size_t>(c->zstd_arena_budget / kZstdArena, 1));
    return waves;
}

// Grow *buf to `base` bytes plus the zstd decoder's scratch for n objects:
// *waves arenas, or n x kZstdScratch (128 KiB per object) for the serial
// kernel.  If the buffer cannot grow to that many arenas, fewer waves are
// tried, then the serial kernel; *waves is what fitted.  A hipMalloc failure
// the fallback recovers from is not recorded as the batch's error.
int ensure_zstd_decode(jfsx_ctx *c, char **buf, size_t *cap, size_t base, int n, int *waves) {
    ErrRec before;
    {
        std::lock_guard<std::mutex> g(c->err_mu);
        before = c->err;
    }
    for (;;) {
        const size_t extra = *waves ? kZstdArena * (size_t)*waves : kZstdScratch * (size_t)n;
        const int rc = ensure_dev(c, buf, cap, base + extra);
        if (rc != JFSX_ENOMEM || *waves == 0) return rc;
        *waves = *waves > c->ncu ? std::max(*waves / 2, c->ncu) : 0;  // fewer waves, then serial
        (void)hipGetLastError();  // the failed hipMalloc is not this batch's error
        {
            std::lock_guard<std::mutex> g(c->err_mu);
            c->err = before;
        }
    }
}

// What a compressor launch needs besides its descriptors, for run_codec and
// run_store: `extra` bytes of device memory behind them -- LZ4's hash tables
// (16 KiB per block), or the zstd compressor's ticket word (256 bytes) and
// per-wave scratch -- and the zstd compressor's wave count.
struct CompSetup {
    bool zstd = false;
    int zc_waves = 0;
    bool zc_queue = false;
    size_t extra = 0;
};
CompSetup comp_setup(const jfsx_ctx *c, bool zstd, int n) {
    // zstd compression: persistent waves per CU (JFSX_ZC_WAVES overrides the
    // default for A/B; LDS and VGPRs allow 16)
    static const int zc_per_cu = getenv("JFSX_ZC_WAVES") ? std::max(1, std::min(16, atoi(getenv("JFSX_ZC_WAVES"))))
                                                         : kZcWavesPerCu;
    static const bool zc_queue = getenv("JFSX_ZC_QUEUE") && atoi(getenv("JFSX_ZC_QUEUE")) == 1;
    CompSetup cs;
    cs.zstd = zstd;
    if (zstd) {
        cs.zc_waves = std::min(n, c->ncu * zc_per_cu);
        cs.zc_queue = zc_queue;
        cs.extra = 256 + kZstdcScratch * (size_t)cs.zc_waves;  // per-wave scratch
    } else {
        cs.extra = kLz4TabBytes * (size_t)n;
    }
    return cs;
}
// tab: the cs.extra bytes
void launch_compress(const jfsx_ctx *c, hipStream_t s, const CompSetup &cs, int n, const ZDev *dz, ZOut *dout,
                     char *tab) {
    if (!cs.zstd) {
        launch_lz4_compress(s, n, c->ncu, dz, dout, (uint32_t *)tab);
        return;
    }
    // JFSX_ZC_QUEUE=1: ticket-queue object assignment (A/B; the word before
    // the scratch is the ticket counter)
    launch_zstd_compress(s, n, cs.zc_waves, dz, dout, (uint8_t *)(tab + 256), cs.zc_queue ? (uint32_t *)tab : nullptr);
}

// The codec stages (jfsx_lz4.hip, jfsx_zstd.hip, jfsx_zstdc.hip): one wave per
// object.  Host-memory batches are staged through the context's slot-0
// staging buffer (inputs up, the out_len bytes of each output down).
int run_codec(jfsx_ctx *c, int n, jfsx_zblk *z, int mem, CodecOp op) {
    if (n < 0 || (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST)) return JFSX_EINVAL;
    for (int i = 0; i < n; i++) {
        if ((z[i].src_len && !z[i].src) || (z[i].dst_cap && !z[i].dst) || z[i].src_len > kLz4MaxInput ||
            z[i].dst_cap >= ((uint64_t)1 << 32))
            return JFSX_EINVAL;
        if (op == kLz4Comp && z[i].dst_cap < lz4_bound(z[i].src_len)) return JFSX_EINVAL;
        if (op == kZstdComp && z[i].dst_cap < zstd_bound(z[i].src_len)) return JFSX_EINVAL;
        if (op == kZstdDecomp && z[i].dst_cap >= ((uint64_t)1 << 31)) return JFSX_EINVAL;  // 32-bit frame positions
    }
    if (n == 0) return 0;
    int rc;
    Workspace &w = c->ws[0];
    const bool comp = op == kLz4Comp || op == kZstdComp;
    const CompSetup cs = comp ? comp_setup(c, op == kZstdComp, n) : CompSetup{};
    // zstd decompression: the decoder's waves and arenas (zstd_decode_waves,
    // ensure_zstd_decode: fewer waves, then the serial kernel, under memory
    // pressure)
    int zd_waves = op == kZstdDecomp ? zstd_decode_waves(c, n) : 0;
    const size_t o_out = align256(sizeof(ZDev) * n), o_tab = o_out + align256(sizeof(ZOut) * n);
    if (op == kZstdDecomp) {
        rc = ensure_zstd_decode(c, &w.d, &w.dcap, o_tab, n, &zd_waves);
    } else {
        rc = ensure_dev(c, &w.d, &w.dcap, o_tab + cs.extra);
    }
    if (rc) return rc;
    if ((rc = ensure_host(&w.h, &w.hcap, o_tab))) return rc;  // descriptors and results only
    hipStream_t s = c->stream;
    ZDev *hz = (ZDev *)w.h;
    std::vector<char *> sdst(n, nullptr);
    if (mem == JFSX_MEM_HOST) {
        size_t need = 0;
        for (int i = 0; i < n; i++) need += align256(z[i].src_len) + align256(z[i].dst_cap);
        if ((rc = ensure_dev(c, &w.stage, &w.scap, std::max<size_t>(need, 256)))) return rc;
        size_t off = 0;
        for (int i = 0; i < n; i++) {
            char *in = w.stage + off;
            off += align256(z[i].src_len);
            sdst[i] = w.stage + off;
            off += align256(z[i].dst_cap);
            if (z[i].src_len) HIP_OK(hipMemcpyAsync(in, z[i].src, z[i].src_len, hipMemcpyHostToDevice, s));
            hz[i] = ZDev{(const uint8_t *)in, (uint8_t *)sdst[i], z[i].src_len, z[i].dst_cap};
        }
    } else {
        for (int i = 0; i < n; i++)
            hz[i] = ZDev{(const uint8_t *)z[i].src, (uint8_t *)z[i].dst, z[i].src_len, z[i].dst_cap};
    }
    HIP_OK(hipMemcpyAsync(w.d, w.h, sizeof(ZDev) * n, hipMemcpyHostToDevice, s));
    if (c->timing) HIP_OK(hipEventRecord(c->ev_k0[0], s));
    const ZDev *dz = (const ZDev *)w.d;
    ZOut *dout = (ZOut *)(w.d + o_out);
    launch_begin();
    switch (op) {
    case kLz4Comp:
    case kZstdComp:
        launch_compress(c, s, cs, n, dz, dout, w.d + o_tab);
        break;
    case kLz4Decomp:
        launch_lz4_decompress(s, n, dz, dout);
        break;
    case kZstdDecomp:
        launch_zstd_decompress(s, n, dz, dout, (uint8_t *)(w.d + o_tab), zd_waves);
        break;
    }
    if (c->timing) HIP_OK(hipEventRecord(c->ev_k1[0], s));
    HIP_OK(hipGetLastError());
    ZOut *ho = (ZOut *)(w.h + o_out);
    HIP_OK(hipMemcpyAsync(ho, dout, sizeof(ZOut) * n, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (c->timing) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, c->ev_k0[0], c->ev_k1[0]));
        add_kernel_ms(c, ms);
    }
    for (int i = 0; i < n; i++) {
        z[i].out_len = ho[i].out_len;
        z[i].status = ho[i].status;
        if (op == kZstdDecomp) {
            z[i].reserved = zd_waves ? ho[i].fallback : 0;
            if (zd_waves && ho[i].fallback) {
                std::lock_guard<std::mutex> g(c->stat_mu);
                c->met.zstd_serial++;
            }
        }
        if (mem == JFSX_MEM_HOST && ho[i].out_len)
            HIP_OK(hipMemcpyAsync(z[i].dst, sdst[i], ho[i].out_len, hipMemcpyDeviceToHost, s));
    }
    if (mem == JFSX_MEM_HOST) HIP_OK(hipStreamSynchronize(s));
    return 0;
}

// ---------------------------------------------------------------------------
// jfsx_load_batch: Open -> decompress -> checksum() of a batch of stored block
// images in one call (cachedStore.load, cached_store.go:673-748).  The stages
// are enqueued on the context's stream back to back (jfsx_load.hip has the
// order and the gate rule); the host plans everything from the lengths alone,
// so it waits once, at the end.
// ---------------------------------------------------------------------------
int check_load_args(int algo, int codec, int n, const jfsx_lblk *blks, int crc_mode, int mem) {
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305 && algo != JFSX_CIPHER_NONE) return JFSX_EINVAL;
    if (codec != JFSX_CODEC_LZ4 && codec != JFSX_CODEC_ZSTD) return JFSX_EINVAL;
    if (crc_mode != JFSX_CRC_NONE && crc_mode != JFSX_CRC_GEN) return JFSX_EINVAL;
    if (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST) return JFSX_EINVAL;
    if (n < 0) return JFSX_EINVAL;
    for (int i = 0; i < n; i++) {
        const jfsx_lblk &b = blks[i];
        if ((b.src_len && !b.src) || (b.len && !b.dst)) return JFSX_EINVAL;
        // run_codec's limits, then the ciphers' (check_aead_args)
        if (b.src_len > kLz4MaxInput || b.len >= ((uint64_t)1 << 32)) return JFSX_EINVAL;
        if (codec == JFSX_CODEC_ZSTD && b.len >= ((uint64_t)1 << 31)) return JFSX_EINVAL;  // 32-bit frame positions
        if (algo == JFSX_AES256GCM && b.src_len > kGcmMaxLen) return JFSX_EINVAL;
        if (algo == JFSX_CHACHA20P1305 && b.src_len > kCpMaxLen) return JFSX_EINVAL;
        if (crc_mode && !b.crc) return JFSX_EINVAL;
        if (mem == JFSX_MEM_DEVICE) {
            // jfsx_blk's rule where an AEAD or CRC kernel touches the buffer:
            // Open reads src, the CRC pass reads dst; the decoders and the
            // wipe take any alignment
            if (algo != JFSX_CIPHER_NONE && b.src_len && !aligned16(b.src)) return JFSX_EINVAL;
            if (crc_mode && b.len && !aligned16(b.dst)) return JFSX_EINVAL;
            if (b.dst && b.dst == b.src) return JFSX_EINVAL;  // the decoders do not run in place
        }
    }
    return 0;
}

struct LoadState {
    HostStage hs;               // host: the images up, the pages down
    std::vector<size_t> poff;   // host: page i at load_stage + img_bytes + poff[i]
    size_t h_res = 0;           // offset of the downloaded results in load_h
    size_t crc_off = 0;         // host CRC_GEN: offset of the CRC words behind the results
    int zd_waves = 0;           // zstd: waves of the block-parallel decoder (0: the serial kernel)
    bool aead = false, crc = false;
};

int load_enqueue(jfsx_ctx *c, int algo, int codec, int n, const jfsx_lblk *blks, int crc_mode, bool host,
                 LoadState &st) {
    hipStream_t s = c->stream;
    const bool aead = st.aead = algo != JFSX_CIPHER_NONE;
    const bool crc = st.crc = crc_mode == JFSX_CRC_GEN;
    const bool zstd = codec == JFSX_CODEC_ZSTD;
    // staging: the images, then (host) the pages
    std::vector<size_t> ioff(n);
    st.poff.assign(n, 0);
    size_t img_bytes = 0, page_bytes = 0;
    uint64_t crc_words = 0, max_len = 0;
    for (int i = 0; i < n; i++) {
        ioff[i] = img_bytes;
        img_bytes += align256(blks[i].src_len);
        st.poff[i] = page_bytes;
        page_bytes += align256(blks[i].len);
        crc_words += nseg_of(blks[i].len);
        max_len = std::max<uint64_t>(max_len, blks[i].len);
    }
    // device workspace of the load path
    size_t off = 0;
    const size_t o_lb = off; off = align256(off + sizeof(LoadBlk) * n);
    const size_t up = off;  // the block records are uploaded from the pinned mirror
    const size_t o_z = off; off = align256(off + sizeof(ZDev) * n);
    const size_t o_zo = off; off = align256(off + sizeof(ZOut) * n);
    const size_t o_res = off; off = align256(off + sizeof(LoadRes) * n);
    const size_t o_crc = off; if (host && crc) off = align256(off + 4 * crc_words);
    const size_t down = host && crc ? o_crc + 4 * crc_words - o_res : sizeof(LoadRes) * n;
    const size_t o_tab = off;
    st.h_res = up;
    st.crc_off = o_crc - o_res;
    int rc;
    // every buffer of the path before the first enqueue: growing one later
    // would free what a stage already in flight uses
    if (zstd) {
        st.zd_waves = zstd_decode_waves(c, n);
        rc = ensure_zstd_decode(c, &c->load_d, &c->load_dcap, o_tab, n, &st.zd_waves);
    } else {
        rc = ensure_dev(c, &c->load_d, &c->load_dcap, o_tab);
    }
    if (rc) return rc;
    if ((rc = ensure_host(&c->load_h, &c->load_hcap, up + down))) return rc;
    const size_t stage_need = host ? img_bytes + page_bytes : aead ? img_bytes : 0;
    if (stage_need && (rc = ensure_dev(c, &c->load_stage, &c->load_scap, stage_need))) return rc;
    char *d = c->load_d, *h = c->load_h, *stage = c->load_stage;
    // host: the images up and the pages down; an empty one is not classified
    std::vector<StageItem> up_items, down_items;
    if (host) {
        st.hs.resize(n, n);
        for (int i = 0; i < n; i++) {
            const jfsx_lblk &b = blks[i];
            if (b.src_len) HostStage::mark(st.hs.in, i, b.src, b.src_len);
            if (b.len) HostStage::mark(st.hs.out, i, b.dst, b.len);
            up_items.push_back({(void *)b.src, stage + ioff[i], ioff[i], b.src_len, (size_t)i});
            down_items.push_back({b.dst, stage + img_bytes + st.poff[i], st.poff[i], b.len, (size_t)i});
        }
        if ((rc = st.hs.reserve(c, img_bytes, page_bytes))) return rc;
    }
    // block records; the Open and CRC stages' blocks
    LoadBlk *hl = (LoadBlk *)(h + o_lb);
    std::vector<jfsx_blk> ab(aead ? n : 0), cb(crc ? n : 0);
    uint64_t cw = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_lblk &b = blks[i];
        uint8_t *img = host || aead ? (uint8_t *)(stage + ioff[i]) : (uint8_t *)b.src;
        if (!b.src_len) img = nullptr;
        hl[i].img = img;
        hl[i].dst = !b.len ? nullptr : host ? (uint8_t *)(stage + img_bytes + st.poff[i]) : (uint8_t *)b.dst;
        hl[i].crc = !crc ? nullptr : host ? (uint8_t *)(d + o_crc + 4 * cw) : b.crc;
        hl[i].src_len = b.src_len;
        hl[i].len = b.len;
        cw += nseg_of(b.len);
        if (aead) {
            jfsx_blk &a = ab[i];
            memset(&a, 0, sizeof(a));
            memcpy(a.key, b.key, 32);
            memcpy(a.nonce, b.nonce, 12);
            memcpy(a.tag, b.tag, 16);
            a.src = host ? img : b.src;  // host: the uploaded image is opened in place
            a.dst = img;
            a.len = b.src_len;
        }
        if (crc) {
            jfsx_blk &k = cb[i];
            memset(&k, 0, sizeof(k));
            k.src = hl[i].dst;
            k.len = b.len;
            k.crc = hl[i].crc;
        }
    }
    HIP_OK(hipMemcpyAsync(d + o_lb, h + o_lb, sizeof(LoadBlk) * n, hipMemcpyHostToDevice, s));
    if (host && (rc = st.hs.upload(s, stage, img_bytes, up_items))) return rc;
    const LoadBlk *dl = (const LoadBlk *)(d + o_lb);
    ZDev *dz = (ZDev *)(d + o_z);
    ZOut *dzo = (ZOut *)(d + o_zo);
    LoadRes *dres = (LoadRes *)(d + o_res);
    // 1. Open into the staging buffer; its BlkOut[n] stays on the device
    const BlkOut *opened = nullptr;
    if (aead) {
        if ((rc = enqueue_aead(c, c->load_aead, s, c->load_ev[0], c->load_ev[1], algo, true, n, ab.data(),
                               JFSX_CRC_NONE, nullptr, nullptr, false)))
            return rc;
        opened = (const BlkOut *)c->load_aead.dout;
    }
    // 2. the gate, 3. the decoder: it sees a block only through the gate's descriptor
    launch_begin();
    launch_load_gate(s, n, dl, opened, dz, dzo);
    if (zstd) launch_zstd_decompress(s, n, dz, dzo, (uint8_t *)(d + o_tab), st.zd_waves);
    else launch_lz4_decompress(s, n, dz, dzo);
    HIP_OK(hipGetLastError());
    // 4. checksum() of every page, planned from len
    if (crc && (rc = enqueue_crc(c, c->load_crc, s, c->load_ev[2], c->load_ev[3], n, cb.data(), JFSX_CRC_GEN, nullptr,
                                 nullptr, false)))
        return rc;
    // 5. verdicts; pages and CRC arrays of failed blocks zeroed
    launch_begin();
    const int groups = (int)std::min<uint64_t>(1024, std::max<uint64_t>(1, (max_len + 65535) / 65536));
    launch_load_finish(s, n, groups, dl, opened, dzo, zstd && st.zd_waves > 0, crc, dres);
    HIP_OK(hipGetLastError());
    // 6. results (and, host, the CRC words behind them) in one download; host: every page
    HIP_OK(hipMemcpyAsync(h + st.h_res, d + o_res, down, hipMemcpyDeviceToHost, s));
    if (host) return st.hs.download(s, stage + img_bytes, page_bytes, std::move(down_items));
    return 0;
}

// Under c->mu for the whole call, as device batches are.
int run_load(jfsx_ctx *c, int algo, int codec, int n, jfsx_lblk *blks, int crc_mode, int mem) {
    int rc = check_load_args(algo, codec, n, blks, crc_mode, mem);
    if (rc || n == 0) return rc;
    const bool host = mem == JFSX_MEM_HOST;
    LoadState st;
    rc = load_enqueue(c, algo, codec, n, blks, crc_mode, host, st);
    rc = wait_stream(c, rc, "hipStreamSynchronize(load)");  // the one wait of the call
    settle_stage(c, c->load_aead, c->load_ev[0], c->load_ev[1], !rc);
    settle_stage(c, c->load_crc, c->load_ev[2], c->load_ev[3], !rc);
    if (!rc) {
        const LoadRes *hr = (const LoadRes *)(c->load_h + st.h_res);
        const char *hw = c->load_h + st.h_res + st.crc_off;
        for (int i = 0; i < n; i++) {
            jfsx_lblk &b = blks[i];
            b.status = hr[i].status;
            b.out_len = hr[i].out_len;
            b.codec_info = hr[i].codec_info;
            if (host && st.crc) {
                memcpy(b.crc, hw, 4 * nseg_of(b.len));
                hw += 4 * nseg_of(b.len);
            }
        }
        st.hs.copy_out();
    }
    if (rc) return rc;
    // jfsx_ctx_metrics: what the separate calls would have counted
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &m = c->met;
    const bool zstd = codec == JFSX_CODEC_ZSTD;
    uint64_t &d_blocks = zstd ? m.zstdd_blocks : m.lz4d_blocks, &d_in = zstd ? m.zstdd_in : m.lz4d_in;
    uint64_t &d_out = zstd ? m.zstdd_out : m.lz4d_out, &d_fail = zstd ? m.zstdd_fail : m.lz4d_fail;
    if (st.aead) m.open_batches++;
    if (st.crc) m.crc_batches++;
    for (int i = 0; i < n; i++) {
        const jfsx_lblk &b = blks[i];
        if (st.aead) {
            m.open_blocks++;
            m.open_bytes += b.src_len;
            m.open_fail += b.status == JFSX_ETAG;
        }
        if (b.status != JFSX_ETAG) {  // the block reached the decoder
            d_blocks++;
            d_in += b.src_len;
            d_out += b.out_len;
            d_fail += b.status == JFSX_EFORMAT || b.status == JFSX_EDSTSIZE;
            if (zstd && b.codec_info) m.zstd_serial++;
        }
        if (st.crc) {
            m.crc_ranges++;
            m.crc_bytes += b.len;
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// jfsx_store_batch: verify / checksum() -> compress -> Seal -> object checksum
// of a batch of pages in one call (uploadStagingFile, cachedStore.upload,
// store.put; cached_store.go:944-999, :371-413).  Two phases on the context's
// stream (jfsx_store.hip has the order and the gate rule): the Seal's plan
// needs the compressed lengths, so the per-block verdicts come back in the
// middle (wait #1) and the host plans phase B from them.
// ---------------------------------------------------------------------------
int check_store_args(int algo, int codec, int n, const jfsx_sblk *blks, int crc_mode, int mem) {
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305 && algo != JFSX_CIPHER_NONE) return JFSX_EINVAL;
    if (codec != JFSX_CODEC_LZ4 && codec != JFSX_CODEC_ZSTD) return JFSX_EINVAL;
    // NONE, GEN, VERIFY, each with or without CT
    if (crc_mode < 0 || (crc_mode & ~(3 | JFSX_CRC_CT)) || (crc_mode & 3) == 3) return JFSX_EINVAL;
    if (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST) return JFSX_EINVAL;
    if (n < 0) return JFSX_EINVAL;
    const bool aead = algo != JFSX_CIPHER_NONE, page_crc = (crc_mode & 3) != 0, ct = (crc_mode & JFSX_CRC_CT) != 0;
    for (int i = 0; i < n; i++) {
        const jfsx_sblk &b = blks[i];
        if (b.reserved) return JFSX_EINVAL;
        if ((b.len && !b.src) || !b.dst) return JFSX_EINVAL;  // an image is never empty
        // run_codec's limits, then the ciphers' on the longest image (check_aead_args)
        if (b.len > kLz4MaxInput) return JFSX_EINVAL;
        const uint64_t bound = codec == JFSX_CODEC_ZSTD ? zstd_bound(b.len) : lz4_bound(b.len);
        if (b.dst_cap < bound) return JFSX_EINVAL;
        if (algo == JFSX_AES256GCM && bound > kGcmMaxLen) return JFSX_EINVAL;
        if (algo == JFSX_CHACHA20P1305 && bound > kCpMaxLen) return JFSX_EINVAL;
        if (page_crc && !b.crc) return JFSX_EINVAL;
        if (ct && b.hdr_len && !b.hdr) return JFSX_EINVAL;
        if (mem == JFSX_MEM_DEVICE) {
            // jfsx_blk's rule where an AEAD or CRC kernel touches the buffer:
            // the page CRC reads src, the Seal writes dst and the image CRC
            // reads it; the compressors take any alignment
            if (page_crc && b.len && !aligned16(b.src)) return JFSX_EINVAL;
            if ((aead || ct) && !aligned16(b.dst)) return JFSX_EINVAL;
            if (b.dst == b.src) return JFSX_EINVAL;  // the compressors do not run in place
        }
    }
    return 0;
}

inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct StoreState {
    bool host = false, aead = false, ct = false, zstd = false;
    bool plain = false;      // jfsx_store_objects with JFSX_CODEC_NONE: no compressor, the Seal reads the pages
    size_t obj_extra = 0;    // jfsx_store_objects: bytes of an object's slot beyond its image (frame, alignment)
    int page_mode = 0;       // JFSX_CRC_NONE / GEN / VERIFY of the pages
    HostStage hs;            // host: the pages up, the images (objects) down
    CompSetup cs;
    std::vector<uint64_t> cap;   // the codec's bound of every page length: the compressor's capacity
    std::vector<size_t> poff;    // host: page i at store_stage + poff[i]
    std::vector<size_t> zoff;    // the compressor's output slot of block i at slots + zoff[i]
    std::vector<size_t> ooff;    // host, phase B: image i at store_img + ooff[i], and there in the bounce buffer
    char *slots = nullptr;       // null: the compressor writes to the callers' dst (device, no cipher)
    size_t page_bytes = 0;
    std::vector<jfsx_blk> pb;    // the page CRC stage's blocks
    std::vector<jfsx_blk> sb;    // phase B: the Seal's / the image CRC stage's blocks, OK blocks only
    std::vector<int> okidx;      // their indices in the batch
    std::vector<uint8_t> ctcrc;  // their ciphertext segment CRCs (JFSX_CRC_CT)
    size_t h_res = 0;            // offset of the downloaded StoreRes[n] in store_h
};

// Phase A: pages up, page CRCs, gate, compressor, verdicts down.  st.plain:
// pages up and the VERIFY stage alone (its BlkOut[n] comes down instead of the
// verdicts); a GEN is left to the Seal's fused pass.
int store_phase_a(jfsx_ctx *c, int n, const jfsx_sblk *blks, StoreState &st) {
    hipStream_t s = c->stream;
    const bool host = st.host;
    const int page_mode = st.plain && st.page_mode == JFSX_CRC_GEN ? JFSX_CRC_NONE : st.page_mode;
    st.cap.assign(n, 0);
    st.poff.assign(n, 0);
    st.zoff.assign(n, 0);
    size_t page_bytes = 0, slot_bytes = 0, out_max = 0;
    for (int i = 0; i < n; i++) {
        st.cap[i] = st.plain ? blks[i].len : st.zstd ? zstd_bound(blks[i].len) : lz4_bound(blks[i].len);
        st.poff[i] = page_bytes;
        page_bytes += align256(blks[i].len);
        st.zoff[i] = slot_bytes;
        slot_bytes += align256(st.cap[i]);
        out_max += align16(st.cap[i] + st.obj_extra);
    }
    st.page_bytes = page_bytes;
    const bool use_slots = !st.plain && (host || st.aead);  // else the compressor writes the callers' dst
    if (!st.plain) st.cs = comp_setup(c, st.zstd, n);
    // device workspace of the store path
    size_t off = 0;
    const size_t o_sb = off; off = align256(off + sizeof(StoreBlk) * n);
    const size_t up = off;  // the block records are uploaded from the pinned mirror
    const size_t o_z = off; off = align256(off + sizeof(ZDev) * n);
    const size_t o_zo = off; off = align256(off + sizeof(ZOut) * n);
    const size_t o_res = off; off = align256(off + sizeof(StoreRes) * n);
    const size_t o_sink = off; off = align256(off + kStoreSink * (size_t)n);
    const size_t o_tab = off;
    st.h_res = up;
    int rc;
    // every buffer of the phase before its first enqueue: growing one later
    // would free what a stage already in flight uses
    if ((rc = ensure_dev(c, &c->store_d, &c->store_dcap, o_tab + st.cs.extra))) return rc;
    if ((rc = ensure_host(&c->store_h, &c->store_hcap, up + sizeof(StoreRes) * n))) return rc;
    const size_t stage_need = (host ? page_bytes : 0) + (use_slots ? slot_bytes : 0);
    if (stage_need && (rc = ensure_dev(c, &c->store_stage, &c->store_scap, stage_need))) return rc;
    char *d = c->store_d, *h = c->store_h, *stage = c->store_stage;
    st.slots = use_slots ? stage + (host ? page_bytes : 0) : nullptr;
    // host: the pages up.  Every destination is classified here, by its
    // capacity, because the buffer of both directions is taken now; which
    // images come down, and how long they are, only phase B knows
    std::vector<StageItem> up_items;
    if (host) {
        st.hs.resize(n, n);
        for (int i = 0; i < n; i++) {
            if (blks[i].len) HostStage::mark(st.hs.in, i, blks[i].src, blks[i].len);
            HostStage::mark(st.hs.out, i, blks[i].dst, st.cap[i] + st.obj_extra);
            up_items.push_back({(void *)blks[i].src, stage + st.poff[i], st.poff[i], blks[i].len, (size_t)i});
        }
        if ((rc = st.hs.reserve(c, page_bytes, out_max))) return rc;
    }
    // block records; the page CRC stage's blocks
    StoreBlk *hs = (StoreBlk *)(h + o_sb);
    st.pb.assign(page_mode ? n : 0, jfsx_blk{});
    for (int i = 0; i < n; i++) {
        const jfsx_sblk &b = blks[i];
        hs[i].src = !b.len ? nullptr : host ? (const uint8_t *)(stage + st.poff[i]) : (const uint8_t *)b.src;
        hs[i].dst = use_slots ? (uint8_t *)(st.slots + st.zoff[i]) : (uint8_t *)b.dst;
        hs[i].sink = (uint8_t *)(d + o_sink + kStoreSink * (size_t)i);
        hs[i].len = b.len;
        hs[i].cap = st.cap[i];
        if (page_mode) {
            jfsx_blk &k = st.pb[i];
            memset(&k, 0, sizeof(k));
            k.src = hs[i].src;
            k.len = b.len;
            k.crc = b.crc;  // host: rides the stage's descriptor upload (VERIFY) / result download (GEN)
        }
    }
    // 1. upload: the records, and every page once
    if (!st.plain) HIP_OK(hipMemcpyAsync(d + o_sb, h + o_sb, sizeof(StoreBlk) * n, hipMemcpyHostToDevice, s));
    if (host && (rc = st.hs.upload(s, stage, page_bytes, up_items))) return rc;
    // 2. checksum() of every page, or its verify; the BlkOut[n] stays on the device
    const BlkOut *verified = nullptr;
    if (page_mode) {
        if ((rc = enqueue_crc(c, c->store_crc, s, c->store_ev[0], c->store_ev[1], n, st.pb.data(), page_mode, nullptr,
                              nullptr, st.plain, host)))
            return rc;
        if (page_mode == JFSX_CRC_VERIFY) verified = (const BlkOut *)c->store_crc.dout;
    }
    if (st.plain) return 0;
    // 3. the gate, 4. the compressor: it sees a block only through the gate's descriptor
    const StoreBlk *ds = (const StoreBlk *)(d + o_sb);
    ZDev *dz = (ZDev *)(d + o_z);
    ZOut *dzo = (ZOut *)(d + o_zo);
    launch_begin();
    launch_store_gate(s, n, ds, verified, dz, dzo);
    launch_compress(c, s, st.cs, n, dz, dzo, d + o_tab);
    // 5. verdicts, and their download
    launch_store_verdict(s, n, ds, verified, dzo, (StoreRes *)(d + o_res));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h + st.h_res, d + o_res, sizeof(StoreRes) * n, hipMemcpyDeviceToHost, s));
    return 0;
}

// Phase B, after wait #1: the Seal (or, without a cipher, the image CRCs)
// planned from out_len over the OK blocks, then every download.
int store_phase_b(jfsx_ctx *c, int algo, int n, const jfsx_sblk *blks, StoreState &st) {
    hipStream_t s = c->stream;
    const bool host = st.host;
    const StoreRes *hr = (const StoreRes *)(c->store_h + st.h_res);
    st.ooff.assign(n, 0);
    size_t out_bytes = 0;
    uint64_t ct_words = 0;
    for (int i = 0; i < n; i++) {
        if (hr[i].status == jfsx_store::kBroken) return JFSX_EIO;  // no Seal is planned from such a length
        if (hr[i].status != JFSX_OK) continue;
        st.okidx.push_back(i);
        st.ooff[i] = out_bytes;
        out_bytes += align16(hr[i].out_len);
        ct_words += nseg_of(hr[i].out_len);
    }
    const int m = (int)st.okidx.size();
    int rc;
    if (host && st.aead && out_bytes && (rc = ensure_dev(c, &c->store_img, &c->store_icap, out_bytes))) return rc;
    if (st.ct) st.ctcrc.assign(4 * ct_words, 0);
    // 6. the Seal out of the compressor's slots, or the image CRCs where they lie
    if (m && (st.aead || st.ct)) {
        st.sb.assign(m, jfsx_blk{});
        uint64_t cw = 0;
        for (int k = 0; k < m; k++) {
            const int i = st.okidx[k];
            jfsx_blk &a = st.sb[k];
            memset(&a, 0, sizeof(a));
            const void *img = st.slots ? (const void *)(st.slots + st.zoff[i]) : blks[i].dst;
            a.src = img;
            a.len = hr[i].out_len;
            if (st.aead) {
                memcpy(a.key, blks[i].key, 32);
                memcpy(a.nonce, blks[i].nonce, 12);
                a.dst = host ? (void *)(c->store_img + st.ooff[i]) : blks[i].dst;
            }
            if (st.ct) a.crc = st.ctcrc.data() + 4 * cw;  // host arrays: they ride the result download
            cw += nseg_of(a.len);
        }
        if (st.aead)
            rc = enqueue_aead(c, c->store_aead, s, c->store_ev[2], c->store_ev[3], algo, false, m, st.sb.data(),
                              st.ct ? (JFSX_CRC_GEN | JFSX_CRC_CT) : JFSX_CRC_NONE, nullptr, nullptr, true, nullptr,
                              nullptr, st.ct);
        else
            rc = enqueue_crc(c, c->store_ct, s, c->store_ev[4], c->store_ev[5], m, st.sb.data(), JFSX_CRC_GEN, nullptr,
                             nullptr, true, true);
        if (rc) return rc;
    }
    // 7. downloads: the page CRC stage's results (host GEN: the CRC words behind them), the images
    if (st.page_mode) {
        Workspace &w = c->store_crc;
        HIP_OK(hipMemcpyAsync(w.h + w.res_off, w.dout, w.down, hipMemcpyDeviceToHost, s));
    }
    if (host && m) {
        // the sealed images lie packed in store_img; without a cipher they stay in the compressor's slots
        std::vector<StageItem> items;
        for (int i : st.okidx)
            items.push_back({blks[i].dst, st.aead ? c->store_img + st.ooff[i] : st.slots + st.zoff[i], st.ooff[i],
                             hr[i].out_len, (size_t)i});
        return st.hs.download(s, c->store_img, st.aead ? out_bytes : 0, std::move(items));
    }
    return 0;
}

// Under c->mu for the whole call, as device batches are; the arguments have
// passed check_store_args and n > 0.
int run_store(jfsx_ctx *c, int algo, int codec, int n, jfsx_sblk *blks, int crc_mode, int mem) {
    int rc = 0;
    StoreState st;
    st.host = mem == JFSX_MEM_HOST;
    st.aead = algo != JFSX_CIPHER_NONE;
    st.ct = (crc_mode & JFSX_CRC_CT) != 0;
    st.zstd = codec == JFSX_CODEC_ZSTD;
    st.page_mode = crc_mode & 3;
    rc = wait_stream(c, store_phase_a(c, n, blks, st), "hipStreamSynchronize(store, wait #1)");
    if (!rc) rc = wait_stream(c, store_phase_b(c, algo, n, blks, st), "hipStreamSynchronize(store, wait #2)");
    // the stages' results (tags, ciphertext CRC words, page CRC words) and main-kernel times
    Workspace *ws[3] = {&c->store_crc, &c->store_aead, &c->store_ct};
    jfsx_blk *wb[3] = {st.pb.data(), st.sb.data(), st.sb.data()};
    for (int k = 0; k < 3; k++) {
        Workspace &w = *ws[k];
        if (!rc && w.n) rc = finish_aead(c, w, c->store_ev[2 * k], c->store_ev[2 * k + 1], k != 1, wb[k]);
        else settle_stage(c, w, c->store_ev[2 * k], c->store_ev[2 * k + 1], false);
    }
    if (!rc) {
        const StoreRes *hr = (const StoreRes *)(c->store_h + st.h_res);
        for (int i = 0; i < n; i++) {
            jfsx_sblk &b = blks[i];
            b.status = hr[i].status;
            b.out_len = hr[i].out_len;
            b.crc_bad_seg = hr[i].bad_seg;
            b.crc_got = hr[i].got;
            b.crc_expect = hr[i].expect;
            b.obj_crc = 0;
            memset(b.tag, 0, 16);
        }
        uint64_t cw = 0;
        for (size_t k = 0; k < st.okidx.size(); k++) {
            jfsx_sblk &b = blks[st.okidx[k]];
            if (st.aead) memcpy(b.tag, st.sb[k].tag, 16);
            if (st.ct) {
                // 8. generateChecksum(hdr || image || tag) from the segment CRCs
                const uint8_t *seg = st.ctcrc.data() + 4 * cw;
                if (st.aead) {
                    (void)jfsx_object_crc32c(b.hdr, b.hdr_len, seg, b.out_len, b.tag, &b.obj_crc);
                } else {
                    uint32_t crc = jfsx_crc32c_update(0, b.hdr, b.hdr_len);
                    for (uint64_t j = 0; j < nseg_of(b.out_len); j++) {
                        const uint8_t *p = seg + 4 * j;
                        const uint32_t cj = (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
                        crc = jfsx_crc32c_combine(crc, cj, std::min<uint64_t>(kSeg, b.out_len - j * kSeg));
                    }
                    b.obj_crc = crc;
                }
                cw += nseg_of(b.out_len);
            }
        }
        st.hs.copy_out();
    }
    if (rc) return rc;
    // jfsx_ctx_metrics: what the separate calls would have counted
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &m = c->met;
    uint64_t &c_blocks = st.zstd ? m.zstdc_blocks : m.lz4c_blocks, &c_in = st.zstd ? m.zstdc_in : m.lz4c_in;
    uint64_t &c_out = st.zstd ? m.zstdc_out : m.lz4c_out;
    const bool ct_launch = st.ct && !st.aead && !st.okidx.empty();  // the image CRC stage: a CRC call of its own
    if (st.page_mode) m.crc_batches++;
    if (ct_launch) m.crc_batches++;
    if (st.aead && !st.okidx.empty()) m.seal_batches++;
    for (int i = 0; i < n; i++) {
        const jfsx_sblk &b = blks[i];
        if (st.page_mode) {
            m.crc_ranges++;
            m.crc_bytes += b.len;
            m.crc_fail += b.status == JFSX_ECRC;
        }
        if (b.status != JFSX_OK) continue;  // the block passed the gate
        c_blocks++;
        c_in += b.len;
        c_out += b.out_len;
        if (st.aead) {
            m.seal_blocks++;
            m.seal_bytes += b.out_len;
        }
        if (ct_launch) {
            m.crc_ranges++;
            m.crc_bytes += b.out_len;
        }
    }
    return 0;
}

}  // namespace

namespace jfsx {
// The device that owns p, with the bounds [lo, hi) of the allocation it lies
// in (so a caller can skip lookups for neighbouring pointers); -1 when p is
// not device memory.  jfsx_alloc_device allocations are found in the
// registry (an allocation must then be released with jfsx_free_device, which
// drops its entry; one released with hipFree leaves a stale range behind);
// other pointers are asked of the HIP runtime, which also reports the
// allocation's bounds, so the caller's range cache covers their neighbours.
int device_of(const void *p, uintptr_t *lo, uintptr_t *hi) {
    const uintptr_t a = (uintptr_t)p;
    {
        std::shared_lock<std::shared_mutex> g(g_alloc_mu);
        auto it = g_allocs.upper_bound(a);
        if (it != g_allocs.begin()) {
            --it;
            if (a < it->second.first) {
                *lo = it->first;
                *hi = it->second.first;
                return it->second.second;
            }
        }
    }
    *lo = a;
    *hi = a + 1;
    hipPointerAttribute_t at;
    if (p && hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice) {
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) == hipSuccess && base && size &&
            (uintptr_t)base <= a && a < (uintptr_t)base + size) {
            *lo = (uintptr_t)base;
            *hi = (uintptr_t)base + size;
        }
        (void)hipGetLastError();
        return at.device;
    }
    (void)hipGetLastError();
    return -1;
}
}  // namespace jfsx

// ===========================================================================
// exported C-ABI
// ===========================================================================
extern "C" {

int jfsx_abi_version(void) { return JFSX_ABI_VERSION; }

int jfsx_last_error(jfsx_ctx *c, int *hip_error, char *msg, size_t cap) {
    ErrRec e;
    if (c) {
        std::lock_guard<std::mutex> g(c->err_mu);
        e = c->err;
    } else {
        e = tl_err;
    }
    if (hip_error) *hip_error = e.hip;
    if (msg && cap) {
        strncpy(msg, e.msg, cap - 1);
        msg[cap - 1] = 0;
    }
    return 0;
}

int jfsx_device_count(int *n) {
    if (!n) return JFSX_EINVAL;
    if (hipGetDeviceCount(n) != hipSuccess) {
        *n = 0;
        return JFSX_ENODEV;
    }
    return 0;
}

// Where the GCM kernel's fused CRC takes its data-only slice lookups: the one
// place that decides, once per context.  The context flags win, then the
// environment (JFSX_CRC_L1=0 / 1), then the build's default.
static bool crc_l1_choice(uint32_t flags) {
    if (flags & JFSX_CTX_CRC_LDS) return false;
    if (flags & JFSX_CTX_CRC_L1) return JFSX_CRC_L1K > 0;
    const char *e = getenv("JFSX_CRC_L1");
    const bool on = e && *e ? atoi(e) != 0 : JFSX_CRC_L1_DEFAULT != 0;
    return on && JFSX_CRC_L1K > 0;
}

int jfsx_ctx_open(int device, uint32_t flags, jfsx_ctx **out) {
    constexpr uint32_t known = JFSX_CTX_BITSLICE | JFSX_CTX_CRC_LDS | JFSX_CTX_CRC_L1;
    if (!out || (flags & ~known) || (flags & (JFSX_CTX_CRC_LDS | JFSX_CTX_CRC_L1)) == (JFSX_CTX_CRC_LDS | JFSX_CTX_CRC_L1))
        return JFSX_EINVAL;
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return JFSX_ENODEV;
    HIP_OK(hipSetDevice(device));
    jfsx_ctx *c = new jfsx_ctx();
    c->device = device;
    c->bitslice = (flags & JFSX_CTX_BITSLICE) != 0;
    c->crc_l1 = crc_l1_choice(flags);
    (void)jfsx_device_numa_node(device, &c->numa_node);
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
        c->ncu = ncu;
    {
        // the block-parallel zstd decoder's arenas (kZstdArena per wave) may
        // take at most an eighth of the device's memory (JFSX_ZSTD_ARENA_MB
        // overrides): 8 waves per CU on a 256-CU, 288 GB part fit (28 GiB)
        size_t total = 0;
        (void)hipDeviceTotalMem(&total, device);
        c->zstd_arena_budget = total ? total / 8 : (size_t)4 << 30;
        if (const char *e = getenv("JFSX_ZSTD_ARENA_MB")) c->zstd_arena_budget = (size_t)atoll(e) << 20;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&c->s_ks, hipStreamNonBlocking) != hipSuccess) {
        jfsx_ctx_close(c);
        return JFSX_EIO;
    }
    std::vector<uint32_t> aes, crc, crcx, crcb;
    make_aes_table(aes);
    make_crc_tables(crc, crcx, &crcb);
    std::vector<uint32_t> cmul;
    make_crc_chunk_mul(cmul, &c->k512);
    const size_t nbytes = 4 * (aes.size() + crc.size() + crcx.size() + cmul.size() + crcb.size());
    if (hipMalloc((void **)&c->d_tab, nbytes) != hipSuccess) {
        c->d_tab = nullptr;
        jfsx_ctx_close(c);  // the streams made above
        return JFSX_ENOMEM;
    }
    std::vector<uint32_t> all;
    all.insert(all.end(), aes.begin(), aes.end());
    all.insert(all.end(), crc.begin(), crc.end());
    all.insert(all.end(), crcx.begin(), crcx.end());
    all.insert(all.end(), crcb.begin(), crcb.end());  // right behind crcx: the kernels reach it from tabs.crcx
    all.insert(all.end(), cmul.begin(), cmul.end());
    if (hipMemcpy(c->d_tab, all.data(), nbytes, hipMemcpyHostToDevice) != hipSuccess) {
        jfsx_ctx_close(c);
        return JFSX_EIO;
    }
    c->tabs.aes = c->d_tab;
    c->tabs.crc = c->d_tab + aes.size();
    c->tabs.crcx = c->d_tab + aes.size() + crc.size();
    c->d_chunk_mul = c->tabs.crcx + crcx.size() + crcb.size();
    for (int k = 0; k < kRing; k++) {
        if (hipEventCreate(&c->ev_k0[k]) != hipSuccess || hipEventCreate(&c->ev_k1[k]) != hipSuccess) {
            jfsx_ctx_close(c);
            return JFSX_EIO;
        }
    }
    for (hipEvent_t &e : c->load_ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            jfsx_ctx_close(c);
            return JFSX_EIO;
        }
    }
    for (hipEvent_t &e : c->store_ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            jfsx_ctx_close(c);
            return JFSX_EIO;
        }
    }
    for (hipEvent_t &e : c->obj_ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            e = nullptr;
            jfsx_ctx_close(c);
            return JFSX_EIO;
        }
    }
    for (PipeSlot &p : c->pipe) {
        if (hipEventCreateWithFlags(&p.ev_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&p.ev_comp, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&p.ev_out, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&p.ev_ks, hipEventDisableTiming) != hipSuccess ||
            hipEventCreate(&p.ev_k0) != hipSuccess || hipEventCreate(&p.ev_k1) != hipSuccess) {
            jfsx_ctx_close(c);
            return JFSX_EIO;
        }
    }
    *out = c;
    return 0;
}

int jfsx_ctx_close(jfsx_ctx *c) {
    if (!c) return JFSX_EINVAL;
    if (getenv("JFSX_PIPE_STATS") && c->ps_groups)
        fprintf(stderr, "jfsx pipe stats (device %d): %llu groups, %llu blocks, %llu H2D / %llu D2H data copies, "
                "enqueue %.1f us/group, slot wait %.1f us/group, own wait %.1f us/group\n", c->device,
                (unsigned long long)c->ps_groups.load(), (unsigned long long)c->ps_blocks.load(),
                (unsigned long long)c->ps_h2d.load(), (unsigned long long)c->ps_d2h.load(),
                c->ps_enq_us.load() / (double)c->ps_groups, c->ps_slot_us.load() / (double)c->ps_groups,
                c->ps_own_us.load() / (double)c->ps_groups);
    if (getenv("JFSX_PIPE_STATS") && c->ps_groups)
        fprintf(stderr, "jfsx pipe stats (device %d): per group: host-memory checks %.1f us, bounce in %.1f us, "
                "bounce out %.1f us, own-group wait %.1f us; bounce: %llu allocations, %.1f MB in, %.1f MB out\n",
                c->device, c->ps_pin_us.load() / (double)c->ps_groups, c->ps_bin_us.load() / (double)c->ps_groups,
                c->ps_bout_us.load() / (double)c->ps_groups, c->ps_wait_us.load() / (double)c->ps_groups,
                (unsigned long long)c->bounce.allocs.load(), c->bounce.bytes_in.load() / 1e6,
                c->bounce.bytes_out.load() / 1e6);
    async_detach(c);  // queued _async batches run first (jfsx_agg.cpp)
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    if (c->d_tab) (void)hipFree(c->d_tab);
    if (c->rsa_d) (void)hipFree(c->rsa_d);
    if (c->rsa_h) (void)hipHostFree(c->rsa_h);
    for (Workspace *w : {&c->load_aead, &c->load_crc, &c->obj_ct}) {
        if (w->d) (void)hipFree(w->d);
        if (w->h) (void)hipHostFree(w->h);
    }
    for (hipEvent_t e : c->obj_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->load_d) (void)hipFree(c->load_d);
    if (c->load_stage) (void)hipFree(c->load_stage);
    if (c->load_h) (void)hipHostFree(c->load_h);
    for (hipEvent_t e : c->load_ev)
        if (e) (void)hipEventDestroy(e);
    for (Workspace *w : {&c->store_crc, &c->store_aead, &c->store_ct}) {
        if (w->d) (void)hipFree(w->d);
        if (w->h) (void)hipHostFree(w->h);
    }
    if (c->store_d) (void)hipFree(c->store_d);
    if (c->store_stage) (void)hipFree(c->store_stage);
    if (c->store_img) (void)hipFree(c->store_img);
    if (c->store_h) (void)hipHostFree(c->store_h);
    for (hipEvent_t e : c->store_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->gat_d) (void)hipFree(c->gat_d);
    if (c->gat_stage) (void)hipFree(c->gat_stage);
    if (c->cmp_d) (void)hipFree(c->cmp_d);
    if (c->gat_h) (void)hipHostFree(c->gat_h);
    if (c->rng_h) (void)hipHostFree(c->rng_h);
    for (auto &kv : c->bounce.idle) {
        forget_pinned(kv.second);
        (void)hipHostFree(kv.second);
    }
    c->bounce.idle.clear();
    for (int k = 0; k < kRing; k++) {
        Workspace &w = c->ws[k];
        if (w.d) (void)hipFree(w.d);
        if (w.stage) (void)hipFree(w.stage);
        if (w.h) (void)hipHostFree(w.h);
        hipEvent_t evs[2] = {c->ev_k0[k], c->ev_k1[k]};
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
    }
    for (PipeSlot &p : c->pipe) {
        if (p.w.d) (void)hipFree(p.w.d);
        if (p.w.stage) (void)hipFree(p.w.stage);
        if (p.w.h) (void)hipHostFree(p.w.h);
        hipEvent_t evs[6] = {p.ev_in, p.ev_comp, p.ev_out, p.ev_k0, p.ev_k1, p.ev_ks};
        for (hipEvent_t e : evs)
            if (e) (void)hipEventDestroy(e);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    if (c->s_in) (void)hipStreamDestroy(c->s_in);
    if (c->s_ks) (void)hipStreamDestroy(c->s_ks);
    if (c->s_out) (void)hipStreamDestroy(c->s_out);
    delete c;
    return 0;
}

int jfsx_ctx_sync(jfsx_ctx *c) {
    if (!c) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    HIP_OK(hipStreamSynchronize(c->s_in));
    HIP_OK(hipStreamSynchronize(c->s_out));
    return 0;
}

int jfsx_ctx_set_slot_bytes(jfsx_ctx *c, uint64_t bytes) {
    if (!c || bytes < (1u << 20)) return JFSX_EINVAL;
    c->slot_bytes = (size_t)bytes;
    return 0;
}

void *jfsx_ctx_stream(jfsx_ctx *c) { return c ? (void *)c->stream : nullptr; }

int jfsx_ctx_set_timing(jfsx_ctx *c, int enable) {
    if (!c) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    c->timing = enable != 0;
    return 0;
}

int jfsx_ctx_kernel_time(jfsx_ctx *c, double *ms_total, uint64_t *launches, int reset) {
    if (!c) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->stat_mu);
    if (ms_total) *ms_total = c->ms_total;
    if (launches) *launches = c->launches;
    if (reset) {
        c->ms_total = 0;
        c->launches = 0;
    }
    return 0;
}

int jfsx_pcie_probe(jfsx_ctx *c, uint64_t bytes, double out[4]) {
    if (!c || !out || bytes < 8 * 4096) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const int chunks = 8;
    const size_t ch = (bytes / chunks) & ~(size_t)4095, tot = ch * chunks;
    char *hA = nullptr, *hB = nullptr, *dA = nullptr, *dB = nullptr;
    int rc = 0;
    auto fail = [&](hipError_t e, int line, const char *what) {
        note_hip_error(e, __FILE__, line, what);
        rc = JFSX_EIO;
    };
    hipError_t e;
    // host buffers exactly as jfsx_alloc_pinned makes the ring's staging
    if ((e = hipHostMalloc((void **)&hA, tot, hipHostMallocPortable)) != hipSuccess ||
        (e = hipHostMalloc((void **)&hB, tot, hipHostMallocPortable)) != hipSuccess ||
        (e = hipMalloc((void **)&dA, tot)) != hipSuccess || (e = hipMalloc((void **)&dB, tot)) != hipSuccess) {
        fail(e, __LINE__, "pcie probe buffers");
    } else {
        memset(hA, 1, tot);
        memset(hB, 2, tot);
        hipEvent_t ea, eb;
        (void)hipEventCreate(&ea);
        (void)hipEventCreate(&eb);
        for (int mode = 0; mode < 3 && !rc; mode++) {  // 0 H2D, 1 D2H, 2 both
            float best_a = 1e30f, best_b = 1e30f;
            for (int it = 0; it < 4 && !rc; it++) {
                // the ring's own two streams only: other contexts' work on the
                // device is not waited for (a diagnostic for an idle context)
                if ((e = hipStreamSynchronize(c->s_in)) != hipSuccess || (e = hipStreamSynchronize(c->s_out)) != hipSuccess) {
                    fail(e, __LINE__, "pcie probe sync");
                    break;
                }
                const auto t0 = std::chrono::steady_clock::now();
                for (int k = 0; k < chunks; k++) {
                    if (mode != 1) (void)hipMemcpyAsync(dA + k * ch, hA + k * ch, ch, hipMemcpyHostToDevice, c->s_in);
                    if (mode != 0) (void)hipMemcpyAsync(hB + k * ch, dB + k * ch, ch, hipMemcpyDeviceToHost, c->s_out);
                }
                if (mode != 1) (void)hipEventRecord(ea, c->s_in);
                if (mode != 0) (void)hipEventRecord(eb, c->s_out);
                if (mode != 1) (void)hipEventSynchronize(ea);
                const float ta = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
                if (mode != 0) (void)hipEventSynchronize(eb);
                const float tb = std::chrono::duration<float>(std::chrono::steady_clock::now() - t0).count();
                if ((e = hipGetLastError()) != hipSuccess) { fail(e, __LINE__, "pcie probe copies"); break; }
                if (it == 0) continue;  // warm-up
                if (ta < best_a) best_a = ta;
                if (tb < best_b) best_b = tb;
            }
            if (mode == 0) out[0] = tot / (double)best_a / 1e9;
            if (mode == 1) out[1] = tot / (double)best_b / 1e9;
            if (mode == 2) {
                out[2] = tot / (double)best_a / 1e9;
                out[3] = tot / (double)best_b / 1e9;
            }
        }
        (void)hipEventDestroy(ea);
        (void)hipEventDestroy(eb);
    }
    if (hA) (void)hipHostFree(hA);
    if (hB) (void)hipHostFree(hB);
    if (dA) (void)hipFree(dA);
    if (dB) (void)hipFree(dB);
    return rc;
}

int jfsx_ctx_metrics(jfsx_ctx *c, jfsx_metrics *out, int reset) {
    if (!c || !out) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->stat_mu);
    *out = c->met;
    out->kernel_ms = c->ms_total;
    out->kernel_launches = c->launches;
    if (reset) {
        c->met = jfsx_metrics{};
        c->ms_total = 0;
        c->launches = 0;
    }
    return 0;
}

int jfsx_alloc_pinned(jfsx_ctx *c, size_t bytes, void **p) {
    if (!c || !p) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    // portable: the multi-device context's other GPUs DMA from it as well
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocPortable);
    if (e == hipSuccess) {
        note_pinned(*p, bytes);
        return 0;
    }
    note_hip_error(e, __FILE__, __LINE__, "hipHostMalloc(pinned)");
    return JFSX_ENOMEM;
}
int jfsx_device_numa_node(int device, int *node) {
    if (!node) return JFSX_EINVAL;
    *node = -1;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return JFSX_ENODEV;
    int v = -1;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeHostNumaId, device) == hipSuccess && v >= 0) {
        *node = v;
        return 0;
    }
    (void)hipGetLastError();
    // the PCI function's node, as the kernel reports it
    char bus[64] = {0}, path[160];
    if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return 0;
    for (char *q = bus; *q; q++) *q = (char)tolower(*q);
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    if (FILE *f = fopen(path, "r")) {
        if (fscanf(f, "%d", &v) == 1 && v >= 0) *node = v;
        fclose(f);
    }
    return 0;
}

namespace {
// set_mempolicy / get_mempolicy (numaif.h modes), called directly so the
// library needs no libnuma
constexpr int kMpolDefault = 0, kMpolBind = 2, kMpolFNode = 1, kMpolFAddr = 2;
constexpr unsigned long kMaxNodes = 1024;
}  // namespace

namespace {
// pinned portable host memory whose pages are bound to `node` (-1: default
// placement).  Binds this thread's allocations to the node while the runtime
// allocates and pins the pages (hipHostMallocNumaUser: they follow the
// caller's policy), then restores the thread's own policy.  Where the node
// cannot be bound (a cpuset without it), the default placement is used.
int alloc_pinned_on(int node, size_t bytes, void **p) {
    unsigned long old_mask[kMaxNodes / 64] = {0}, mask[kMaxNodes / 64] = {0};
    int old_mode = kMpolDefault;
    bool bound = false;
    if (node >= 0 && node < (int)kMaxNodes && syscall(SYS_get_mempolicy, &old_mode, old_mask, kMaxNodes, nullptr, 0) == 0) {
        mask[node / 64] = 1ul << (node % 64);
        bound = syscall(SYS_set_mempolicy, kMpolBind, mask, kMaxNodes) == 0;
    }
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocPortable | (bound ? hipHostMallocNumaUser : 0));
    if (bound) (void)syscall(SYS_set_mempolicy, old_mode, old_mode == kMpolDefault ? nullptr : old_mask, kMaxNodes);
    if (e == hipSuccess) return 0;
    note_hip_error(e, __FILE__, __LINE__, "hipHostMalloc(pinned, NUMA node)");
    return JFSX_ENOMEM;
}
}  // namespace

int jfsx_alloc_pinned_node(jfsx_ctx *c, size_t bytes, int node, void **p) {
    if (!c || !p || node < -1 || node >= (int)kMaxNodes) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    if (node < 0 && jfsx_device_numa_node(c->device, &node)) node = -1;
    const int rc = alloc_pinned_on(node, bytes, p);
    if (rc == 0) note_pinned(*p, bytes);
    return rc;
}

int jfsx_host_numa_node(const void *p, size_t bytes, int *node) {
    if (!p || !node) return JFSX_EINVAL;
    *node = -1;
    const size_t page = 4096, step = (size_t)64 << 20;
    for (size_t o = 0; o < std::max<size_t>(bytes, 1); o += step) {
        int nd = -1;
        void *a = (void *)(((uintptr_t)p + o) & ~(uintptr_t)(page - 1));
        if (syscall(SYS_get_mempolicy, &nd, nullptr, 0, a, kMpolFNode | kMpolFAddr) != 0) return 0;
        if (*node == -1) *node = nd;
        else if (*node != nd) {
            *node = -2;
            return 0;
        }
    }
    return 0;
}

int jfsx_free_pinned(jfsx_ctx *c, void *p) {
    if (!c) return JFSX_EINVAL;
    forget_pinned(p);
    HIP_OK(hipHostFree(p));
    return 0;
}
int jfsx_alloc_device(jfsx_ctx *c, size_t bytes, void **p) {
    if (!c || !p) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) {
        note_alloc(*p, bytes, c->device);
        return 0;
    }
    note_hip_error(e, __FILE__, __LINE__, "hipMalloc(device buffer)");
    return JFSX_ENOMEM;
}
int jfsx_free_device(jfsx_ctx *c, void *p) {
    if (!c) return JFSX_EINVAL;
    forget_alloc(p);
    HIP_OK(hipFree(p));
    return 0;
}
int jfsx_memcpy_h2d(jfsx_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}
int jfsx_memcpy_d2h(jfsx_ctx *c, void *dst, const void *src, size_t bytes) {
    if (!c) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

namespace {
// host batches lock per group inside the pipeline (the call waits unlocked);
// device batches hold the context for the whole call
int aead_entry(jfsx_ctx *c, int algo, bool open, int n, jfsx_blk *blks, int crc_mode, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    if (mem != JFSX_MEM_HOST && mem != JFSX_MEM_DEVICE) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    int rc;
    if (mem == JFSX_MEM_HOST) {
        rc = run_aead_host(c, algo, open, n, blks, crc_mode);
    } else {
        std::lock_guard<std::mutex> g(c->mu);
        rc = run_aead(c, algo, open, n, blks, crc_mode);
    }
    if (rc == 0) tally_aead(c, open, n, blks);
    return rc;
}
}  // namespace

int jfsx_seal_batch(jfsx_ctx *c, int algo, int n, jfsx_blk *blks, int crc_mode, int mem) {
    return aead_entry(c, algo, false, n, blks, crc_mode, mem);
}

int jfsx_open_batch(jfsx_ctx *c, int algo, int n, jfsx_blk *blks, int crc_mode, int mem) {
    return aead_entry(c, algo, true, n, blks, crc_mode, mem);
}

int jfsx_crc32c_segments(jfsx_ctx *c, int n, jfsx_range *ranges, int mode, int mem) {
    if (!c || (n > 0 && !ranges)) return JFSX_EINVAL;
    if (mem != JFSX_MEM_HOST && mem != JFSX_MEM_DEVICE) return JFSX_EINVAL;
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    int rc;
    if (mem == JFSX_MEM_HOST) {
        rc = run_crc_host(c, n, ranges, mode);  // the host pipeline locks per group
    } else {
        std::lock_guard<std::mutex> g(c->mu);
        rc = run_crc(c, n, ranges, mode);
    }
    if (rc == 0) tally_crc(c, n, ranges);
    return rc;
}

uint64_t jfsx_lz4_bound(uint64_t n) { return lz4_bound(n); }

int jfsx_lz4_compress_batch(jfsx_ctx *c, int n, jfsx_zblk *blks, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const int rc = run_codec(c, n, blks, mem, kLz4Comp);
    if (rc == 0) tally_codec(c, c->met.lz4c_blocks, c->met.lz4c_in, c->met.lz4c_out, nullptr, n, blks);
    return rc;
}

int jfsx_lz4_decompress_batch(jfsx_ctx *c, int n, jfsx_zblk *blks, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const int rc = run_codec(c, n, blks, mem, kLz4Decomp);
    if (rc == 0) tally_codec(c, c->met.lz4d_blocks, c->met.lz4d_in, c->met.lz4d_out, &c->met.lz4d_fail, n, blks);
    return rc;
}

int jfsx_zstd_decompress_batch(jfsx_ctx *c, int n, jfsx_zblk *blks, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const int rc = run_codec(c, n, blks, mem, kZstdDecomp);
    if (rc == 0) tally_codec(c, c->met.zstdd_blocks, c->met.zstdd_in, c->met.zstdd_out, &c->met.zstdd_fail, n, blks);
    return rc;
}

uint64_t jfsx_zstd_bound(uint64_t n) { return zstd_bound(n); }

int jfsx_zstd_compress_batch(jfsx_ctx *c, int n, jfsx_zblk *blks, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    const int rc = run_codec(c, n, blks, mem, kZstdComp);
    if (rc == 0) tally_codec(c, c->met.zstdc_blocks, c->met.zstdc_in, c->met.zstdc_out, nullptr, n, blks);
    return rc;
}

int jfsx_load_batch(jfsx_ctx *c, int algo, int codec, int n, jfsx_lblk *blks, int crc_mode, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_load(c, algo, codec, n, blks, crc_mode, mem);
}

int jfsx_store_batch(jfsx_ctx *c, int algo, int codec, int n, jfsx_sblk *blks, int crc_mode, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    // argument errors before the context's device is touched
    const int rc = check_store_args(algo, codec, n, blks, crc_mode, mem);
    if (rc || n == 0) return rc;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_store(c, algo, codec, n, blks, crc_mode, mem);
}

int jfsx_checksum(jfsx_ctx *c, const void *data, uint64_t len, uint8_t *out) {
    if (!c || !out || (len && !data)) return JFSX_EINVAL;
    jfsx_range r;
    memset(&r, 0, sizeof(r));
    r.data = data;
    r.len = len;
    r.crc = out;
    if (len == 0) {
        memset(out, 0, 4);  // disk_cache.go:1221: (0-1)/csBlock+1 = 1 entry, loop body never runs
        return 0;
    }
    return jfsx_crc32c_segments(c, 1, &r, JFSX_CRC_GEN, JFSX_MEM_HOST);
}

// ---------------------------------------------------------------------------
// Hadoop file checksum, MD5-of-MD5-of-CRC32C (getFileChecksum,
// sdk/java/src/main/java/io/juicefs/JuiceFileSystemImpl.java:1286-1343)
// ---------------------------------------------------------------------------
namespace {
constexpr uint32_t kFsumBpc = 512;                // bytesPerCRC: Hadoop's default, the only value the reference pins
constexpr size_t kFsumStage = (size_t)16 << 20;  // host data: bytes staged per round

// The file MD5 over the k block digests: Hadoop hashes DataOutputBuffer
// .getData(), the whole backing array (32 bytes at first, grown to
// max(2 * cap, needed) by the 16-byte appends), so the 16 k digest bytes
// zero-padded to the smallest 32 * 2^j that holds them.
void fsum_finish(const uint8_t *digests, uint64_t k, uint64_t span_len, uint64_t block_bytes, jfsx_fsum *f) {
    uint64_t cap = 32;
    while (cap < 16 * k) cap *= 2;
    static const uint8_t zeros[256] = {0};
    jfsx_md5::Ctx m;
    jfsx_md5::init(&m);
    if (k) jfsx_md5::update(&m, digests, 16 * k);
    for (uint64_t pad = cap - 16 * k; pad;) {
        const uint64_t t = std::min<uint64_t>(pad, sizeof(zeros));
        jfsx_md5::update(&m, zeros, t);
        pad -= t;
    }
    jfsx_md5::final(&m, f->md5);
    f->bytes_per_crc = k ? kFsumBpc : 0;
    f->crc32c = k ? 1 : 0;
    f->crc_per_block = k && span_len > block_bytes ? block_bytes / kFsumBpc : 0;
}

struct FsumPiece {
    int file;
    uint64_t off, len;  // of the file; off % 4096 == 0
    size_t soff;        // host data: offset in the staging buffers
};

// The batch under c->mu.  The data is cut into rounds of pieces: device
// memory is one round with every file a piece; host memory goes through the
// pinned bounce buffer and the device staging buffer in rounds of up to
// kFsumStage bytes, pieces of whole 4 KiB spans (but a file's last), which the
// chunk-CRC kernel hashes independently into the files' chunk-CRC arrays.
int run_file_checksum(jfsx_ctx *c, int n, jfsx_fsum *f, uint64_t block_bytes, bool device, char *bounce,
                      size_t stage_cap) {
    const uint64_t per = block_bytes / kFsumBpc;
    std::vector<uint64_t> w0(n + 1, 0), b0(n + 1, 0);  // first chunk-CRC word / DFS block of file i
    for (int i = 0; i < n; i++) {
        const uint64_t nch = (f[i].len + kFsumBpc - 1) / kFsumBpc;
        w0[i + 1] = w0[i] + nch;
        b0[i + 1] = b0[i] + (nch + per - 1) / per;
    }
    const uint64_t W = w0[n], B = b0[n];
    if (B > 0xffffffffull) return JFSX_EINVAL;
    if (W == 0) {
        for (int i = 0; i < n; i++) fsum_finish(nullptr, 0, 0, block_bytes, &f[i]);
        return 0;
    }
    std::vector<std::vector<FsumPiece>> rounds(1);
    if (device) {
        for (int i = 0; i < n; i++)
            if (f[i].len) rounds[0].push_back(FsumPiece{i, 0, f[i].len, 0});
    } else {
        size_t used = 0;
        for (int i = 0; i < n; i++)
            for (uint64_t off = 0; off < f[i].len;) {
                const uint64_t room = (stage_cap - used) & ~(uint64_t)4095;
                const uint64_t take = std::min<uint64_t>(f[i].len - off, room);
                if (!take) {
                    rounds.emplace_back();
                    used = 0;
                    continue;
                }
                rounds.back().push_back(FsumPiece{i, off, take, used});
                used += (take + 4095) & ~(size_t)4095;
                off += take;
            }
    }
    // tasks of every round, cut as enqueue_crc cuts them
    std::vector<std::vector<Task>> rtasks(rounds.size());
    size_t max_tasks = 1, max_pieces = 1;
    for (size_t r = 0; r < rounds.size(); r++) {
        std::vector<uint64_t> lens;
        for (const FsumPiece &p : rounds[r]) lens.push_back(p.len);
        rtasks[r] = plan_batch(kPlanCrc, lens).tasks;
        max_tasks = std::max(max_tasks, rtasks[r].size());
        max_pieces = std::max(max_pieces, rounds[r].size());
    }
    Workspace &w = c->ws[0];
    size_t off = 0;
    const size_t o_blk = off; off = align256(off + sizeof(BlkDev) * max_pieces);
    const size_t o_task = off; off = align256(off + sizeof(Task) * max_tasks);
    const size_t o_job = off; off = align256(off + sizeof(Md5Job) * B);
    const size_t h_bytes = off;
    const size_t o_dig = off; off = align256(off + 16 * B);
    const size_t o_words = off; off = align256(off + 4 * W);
    int rc;
    if ((rc = ensure_dev(c, &w.d, &w.dcap, off))) return rc;
    if ((rc = ensure_host(&w.h, &w.hcap, h_bytes + 16 * B))) return rc;
    if (!device && (rc = ensure_dev(c, &w.stage, &w.scap, stage_cap))) return rc;
    char *h = w.h, *d = w.d;
    uint32_t *words = (uint32_t *)(d + o_words);
    Md5Job *jobs = (Md5Job *)(h + o_job);
    for (int i = 0; i < n; i++) {
        const uint64_t nch = w0[i + 1] - w0[i];
        for (uint64_t b = 0; b < b0[i + 1] - b0[i]; b++)
            jobs[b0[i] + b] = Md5Job{w0[i] + b * per, std::min(per, nch - b * per)};
    }
    const hipStream_t s = c->stream;
    launch_begin();
    HIP_OK(hipMemcpyAsync(d + o_job, h + o_job, sizeof(Md5Job) * B, hipMemcpyHostToDevice, s));
    bool timed = false;
    // wait for the stream; then the CRC kernel's time of the round just run
    auto settle = [&]() -> int {
        HIP_OK(hipStreamSynchronize(s));
        if (timed) {
            float ms = 0;
            timed = false;
            HIP_OK(hipEventElapsedTime(&ms, c->ev_k0[0], c->ev_k1[0]));
            add_kernel_ms(c, ms);
        }
        return 0;
    };
    for (size_t r = 0; r < rounds.size(); r++) {
        const std::vector<FsumPiece> &ps = rounds[r];
        if (ps.empty()) continue;
        BlkDev *hb = (BlkDev *)(h + o_blk);
        size_t extent = 0;
        for (size_t k = 0; k < ps.size(); k++) {
            const FsumPiece &p = ps[k];
            memset(&hb[k], 0, sizeof(BlkDev));
            hb[k].len = p.len;
            hb[k].crc_calc = words + w0[p.file] + p.off / kFsumBpc;
            if (device) {
                hb[k].src = (const uint8_t *)f[p.file].data + p.off;
            } else {
                memcpy(bounce + p.soff, (const char *)f[p.file].data + p.off, p.len);
                hb[k].src = (const uint8_t *)w.stage + p.soff;
                extent = p.soff + p.len;
            }
        }
        memcpy(h + o_task, rtasks[r].data(), sizeof(Task) * rtasks[r].size());
        HIP_OK(hipMemcpyAsync(d, h, o_job, hipMemcpyHostToDevice, s));
        if (extent) {
            HIP_OK(hipMemcpyAsync(w.stage, bounce, extent, hipMemcpyHostToDevice, s));
            bounce_count(c, extent, 0);
        }
        if (c->timing) HIP_OK(hipEventRecord(c->ev_k0[0], s));
        launch_crc_chunks(s, (int)rtasks[r].size(), (const Task *)(d + o_task), (const BlkDev *)(d + o_blk), c->tabs,
                          c->d_chunk_mul, c->k512);
        if (c->timing) HIP_OK(hipEventRecord(c->ev_k1[0], s));
        timed = c->timing;
        HIP_OK(hipGetLastError());
        // the descriptors' mirror and the staging buffers are rewritten by the next round
        if (r + 1 < rounds.size() && (rc = settle())) return rc;
    }
    launch_md5_blocks(s, (uint32_t)B, (const Md5Job *)(d + o_job), words, (uint32_t *)(d + o_dig));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h + h_bytes, d + o_dig, 16 * B, hipMemcpyDeviceToHost, s));
    if ((rc = settle())) return rc;
    for (int i = 0; i < n; i++)
        fsum_finish((const uint8_t *)h + h_bytes + 16 * b0[i], b0[i + 1] - b0[i], f[i].len, block_bytes, &f[i]);
    return 0;
}
}  // namespace

uint64_t jfsx_file_checksum_span(uint64_t file_size, uint64_t length, uint32_t bytes_per_crc) {
    if (!bytes_per_crc) return 0;
    if (length < bytes_per_crc) return std::min(file_size, length);
    const uint64_t chunks = length / bytes_per_crc + (length % bytes_per_crc ? 1 : 0);
    if (chunks > UINT64_MAX / bytes_per_crc) return file_size;
    return std::min(file_size, chunks * bytes_per_crc);
}

int jfsx_file_checksum_batch(jfsx_ctx *c, int n, jfsx_fsum *files, uint32_t bytes_per_crc, uint64_t block_bytes,
                             int mem) {
    if (!c || n < 0 || (n > 0 && !files)) return JFSX_EINVAL;
    if (mem != JFSX_MEM_HOST && mem != JFSX_MEM_DEVICE) return JFSX_EINVAL;
    if (bytes_per_crc != kFsumBpc || !block_bytes || block_bytes % kFsumBpc) return JFSX_EINVAL;
    const bool device = mem == JFSX_MEM_DEVICE;
    uint64_t total = 0, staged = 0;
    for (int i = 0; i < n; i++) {
        if (files[i].len && (!files[i].data || (device && !aligned16(files[i].data)))) return JFSX_EINVAL;
        total += files[i].len;
        staged += (files[i].len + 4095) & ~(uint64_t)4095;
    }
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    char *bounce = nullptr;
    size_t bcap = 0;
    const size_t stage_cap = (size_t)std::min<uint64_t>(kFsumStage, std::max<uint64_t>(staged, 4096));
    if (!device && total && !(bounce = bounce_get(c, stage_cap, &bcap))) return JFSX_ENOMEM;
    const int rc = run_file_checksum(c, n, files, block_bytes, device, bounce, stage_cap);
    if (rc) (void)hipStreamSynchronize(c->stream);  // nothing in flight reads the buffers once the call returns
    if (bounce) bounce_put(c, bounce, bcap);
    if (rc == 0) {
        std::lock_guard<std::mutex> sg(c->stat_mu);
        c->met.crc_batches++;
        c->met.crc_ranges += n;
        c->met.crc_bytes += total;
    }
    return rc;
}

int jfsx_file_checksum_fold(const uint8_t *chunk_crcs, uint64_t nchunks, uint64_t span_len, uint32_t bytes_per_crc,
                            uint64_t block_bytes, jfsx_fsum *out) {
    if (!out || bytes_per_crc != kFsumBpc || !block_bytes || block_bytes % kFsumBpc) return JFSX_EINVAL;
    if ((nchunks && !chunk_crcs) || nchunks != span_len / kFsumBpc + (span_len % kFsumBpc ? 1 : 0)) return JFSX_EINVAL;
    const uint64_t per = block_bytes / kFsumBpc, k = (nchunks + per - 1) / per;
    std::vector<uint8_t> digests(16 * k);
    for (uint64_t b = 0; b < k; b++)
        jfsx_md5::digest(chunk_crcs + 4 * per * b, 4 * std::min(per, nchunks - per * b), digests.data() + 16 * b);
    fsum_finish(digests.data(), k, span_len, block_bytes, out);
    return 0;
}

int jfsx_cache_verify(jfsx_ctx *c, const void *file, uint64_t file_size, uint64_t length, int level, uint64_t off,
                      uint64_t size, void *out, uint64_t *n_out, uint32_t *got, uint32_t *expect,
                      int64_t *bad_seg) {
    // cacheFile.ReadAt, disk_cache.go:1255-1329 -- range logic on the host,
    // the CRC work on the GPU.
    if (!c || !file || !n_out || level < 0 || level > 3) return JFSX_EINVAL;
    const uint8_t *f = (const uint8_t *)file;
    *n_out = 0;
    *bad_seg = -1;
    auto pread = [&](uint8_t *dst, uint64_t sz, uint64_t o, bool *eof) -> uint64_t {
        uint64_t nn = 0;
        *eof = false;
        if (o < file_size) {
            nn = std::min(sz, file_size - o);
            if (nn) memcpy(dst, f + o, nn);
        }
        if (nn < sz) *eof = true;
        return nn;
    };
    bool eof = false;
    if (level == 0 || (level == 1 && (off != 0 || size != length))) {
        *n_out = pread((uint8_t *)out, size, off, &eof);
        return eof ? JFSX_EOF : 0;
    }
    std::vector<uint8_t> tmp;
    uint8_t *rb = (uint8_t *)out;
    uint64_t rbsize = size, roff = off;
    if (level == 3) {
        roff = off / kSeg * kSeg;
        uint64_t rend = off + size;
        if (rend % kSeg != 0) {
            rend = (rend / kSeg + 1) * kSeg;
            if (rend > length) rend = length;
        }
        if (rend - roff != size) {
            rbsize = rend - roff;
            tmp.resize(std::max<uint64_t>(rbsize, 1));
            rb = tmp.data();
        }
    }
    const uint64_t nread = pread(rb, rbsize, roff, &eof);
    int rc = 0;
    if (eof) {
        rc = JFSX_EOF;
    } else {
        uint64_t ioff = roff / kSeg, cstart = 0, clen = rbsize;
        bool check = true;
        if (level == 2) {
            if (roff % kSeg != 0) {
                const uint64_t o = kSeg - roff % kSeg;
                if (clen <= o) check = false;
                else {
                    cstart += o;
                    clen -= o;
                    ioff += 1;
                }
            }
            const uint64_t end = roff + nread;
            if (check && end != length && end % kSeg != 0) {
                if (clen <= end % kSeg) check = false;
                else clen -= end % kSeg;
            }
        }
        if (check) {
            const uint64_t nexp = clen ? (clen - 1) / kSeg + 1 : 1;
            std::vector<uint8_t> ebuf(4 * nexp);
            bool eof2 = false;
            pread(ebuf.data(), 4 * nexp, length + ioff * 4, &eof2);
            if (eof2) {
                rc = JFSX_EOF;
            } else if (clen) {
                // the window goes to the host pipeline as it is: a pageable
                // window (the caller's buffer, or the widened read of the
                // extend level) is bounced by this thread, a pinned one
                // streams directly; concurrent readers share the pipeline
                int e;
                jfsx_range r;
                memset(&r, 0, sizeof(r));
                r.data = rb + cstart;
                r.len = clen;
                r.crc = ebuf.data();
                e = jfsx_crc32c_segments(c, 1, &r, JFSX_CRC_VERIFY, JFSX_MEM_HOST);
                if (e) return e;
                if (r.status == JFSX_ECRC) {
                    rc = JFSX_ECRC;
                    if (got) *got = r.got;
                    if (expect) *expect = r.expect;
                    *bad_seg = (int64_t)ioff + r.bad_seg;
                }
            }
        }
    }
    if (!tmp.empty() || (level == 3 && rb != (uint8_t *)out)) {
        if (rc == 0) {
            const uint64_t avail = rbsize - (off - roff);
            const uint64_t cpy = std::min(avail, size);
            if (cpy) memcpy(out, rb + (off - roff), cpy);
            *n_out = cpy;
        } else {
            *n_out = 0;
        }
    } else {
        *n_out = nread;
    }
    return rc;
}

int jfsx_parse_header(const void *obj, uint64_t olen, int *klen, int *nlen) {
    const uint8_t *o = (const uint8_t *)obj;
    if (!o || olen < 3) return JFSX_EMISFORMED;
    const int kl = ((int)o[0] << 8) + o[1], nl = o[2];
    if (klen) *klen = kl;
    if (nlen) *nlen = nl;
    if ((uint64_t)(3 + kl + nl) >= olen) return JFSX_EMISFORMED;  // encrypt.go:199-201
    return 0;
}

// ---------------------------------------------------------------------------
// host CRC32C helpers for the object checksum (pkg/object/checksum.go)
// ---------------------------------------------------------------------------
namespace {
const uint32_t *crc_table1() {
    static uint32_t t[256];
    static std::once_flag once;
    std::call_once(once, [] {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t v = i;
            for (int k = 0; k < 8; k++) v = v & 1 ? (v >> 1) ^ kCrcPoly : v >> 1;
            t[i] = v;
        }
    });
    return t;
}
uint32_t h_xpow8(uint64_t n) {  // x^(8n) mod P
    uint32_t r = 1u << 31, p = 1u << 23;
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mulmod_h(p, r);
        p = crc_mulmod_h(p, p);
    }
    return r;
}
uint32_t be32(const uint8_t *p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
}  // namespace

uint32_t jfsx_crc32c_update(uint32_t crc, const void *data, uint64_t n) {
    // hash/crc32.Update(crc, MakeTable(Castagnoli), p): pre/post-inverted
    const uint32_t *t = crc_table1();
    const uint8_t *p = (const uint8_t *)data;
    crc = ~crc;
    for (uint64_t i = 0; i < n; i++) crc = t[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}

uint32_t jfsx_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) {
    return len_b ? crc_mulmod_h(h_xpow8(len_b), crc_a) ^ crc_b : crc_a;
}

int jfsx_object_crc32c(const void *hdr, uint64_t hlen, const uint8_t *seg_crcs, uint64_t clen, const uint8_t *tag,
                       uint32_t *out) {
    // generateChecksum(header || C || tag) (checksum.go:31-53) from the
    // engine's big-endian 32 KiB segment CRCs of C (crc_mode GEN|CT)
    if (!out || (hlen && !hdr) || (clen && !seg_crcs) || !tag) return JFSX_EINVAL;
    uint32_t crc = jfsx_crc32c_update(0, hdr, hlen);
    const uint64_t ns = clen ? (clen - 1) / kSeg + 1 : 0;
    for (uint64_t j = 0; j < ns; j++) {
        const uint64_t lj = std::min<uint64_t>(kSeg, clen - j * kSeg);
        crc = jfsx_crc32c_combine(crc, be32(seg_crcs + 4 * j), lj);
    }
    *out = jfsx_crc32c_update(crc, tag, 16);
    return 0;
}

}  // extern "C"

namespace {
// dataEncryptor.Encrypt / Decrypt around one Seal / Open, issued either as a
// one-block batch on a context or through the aggregator (jfsx_agg_data_*)
using AeadFn = std::function<int(jfsx_blk *, int crc_mode)>;

int data_encrypt(const AeadFn &seal, int algo, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *wrapped,
                 int wlen, const void *plaintext, uint64_t len, void *out, uint64_t out_cap, uint64_t *out_len,
                 uint32_t *obj_crc, uint8_t *seg_crc) {
    // encrypt.go:182-193: [BE16 klen][nlen][wrapped key][nonce][Seal(plaintext)]
    if (!key || !nonce || wlen < 0 || wlen > 65535 || (wlen && !wrapped) || !out) return JFSX_EINVAL;
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;
    const uint64_t hdr = 3 + (uint64_t)wlen + 12;
    if (out_cap < hdr + len + 16) return JFSX_EINVAL;
    uint8_t *o = (uint8_t *)out;
    o[0] = (uint8_t)(wlen >> 8);
    o[1] = (uint8_t)(wlen & 0xff);
    o[2] = 12;
    if (wlen) memcpy(o + 3, wrapped, wlen);
    memcpy(o + 3 + wlen, nonce, 12);
    jfsx_blk b;
    memset(&b, 0, sizeof(b));
    memcpy(b.key, key, 32);
    memcpy(b.nonce, nonce, 12);
    b.src = plaintext;
    b.dst = o + hdr;
    b.len = len;
    // the checksums the call asks for, in one pass: checksum() of the
    // plaintext (seg_crc, straight into the caller's array), the ciphertext
    // segment CRCs the object checksum is folded from (obj_crc), or both
    const uint64_t ns = nseg_of(len);
    std::vector<uint8_t> segs;
    int mode = JFSX_CRC_NONE;
    if (obj_crc && seg_crc) {
        segs.resize(8 * ns);
        b.crc = segs.data();
        mode = JFSX_CRC_GEN | JFSX_CRC_BOTH;
    } else if (obj_crc) {
        segs.resize(4 * ns);
        b.crc = segs.data();
        mode = JFSX_CRC_GEN | JFSX_CRC_CT;
    } else if (seg_crc) {
        b.crc = seg_crc;
        mode = JFSX_CRC_GEN;
    }
    int rc = seal(&b, mode);
    if (rc) return rc;
    memcpy(o + hdr + len, b.tag, 16);
    const uint8_t *ct_segs = obj_crc && seg_crc ? segs.data() + 4 * ns : segs.data();
    if (obj_crc && seg_crc) memcpy(seg_crc, segs.data(), 4 * ns);
    if (obj_crc && (rc = jfsx_object_crc32c(o, hdr, ct_segs, len, b.tag, obj_crc))) return rc;
    if (out_len) *out_len = hdr + len + 16;
    return 0;
}

int data_decrypt(const AeadFn &open, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                 uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc,
                 uint8_t *seg_crc) {
    // encrypt.go:196-216; with expect_crc, the object checksum the store kept
    // (checksum.go:55-82) is verified in the same pass over C; with seg_crc,
    // checksum() of the plaintext for the cache file the load path writes next
    // (cached_store.go:745 -> disk_cache.go:469) comes out of the same pass
    if (!key || !obj || !out) return JFSX_EINVAL;
    int kl = 0, nl = 0;
    int rc = jfsx_parse_header(obj, olen, &kl, &nl);
    if (rc) return rc;
    const uint8_t *o = (const uint8_t *)obj;
    if (expect_crc && !got_crc) return JFSX_EINVAL;
    if (nl != 12) return JFSX_ETAG;  // aead.Open rejects a wrong nonce size (recovered as an error upstream)
    const uint64_t hdr = 3 + (uint64_t)kl + nl;
    if (olen - hdr < 16) return JFSX_ETAG;  // shorter than the tag: cipher: message authentication failed
    const uint64_t len = olen - hdr - 16;
    if (out_cap < len) return JFSX_EINVAL;
    jfsx_blk b;
    memset(&b, 0, sizeof(b));
    memcpy(b.key, key, 32);
    memcpy(b.nonce, o + 3 + kl, 12);
    b.src = o + hdr;
    b.dst = out;
    b.len = len;
    memcpy(b.tag, o + hdr + len, 16);
    const uint64_t ns = nseg_of(len);
    std::vector<uint8_t> segs;
    int mode = JFSX_CRC_NONE;
    if (expect_crc && seg_crc) {
        segs.resize(8 * ns);
        b.crc = segs.data();
        mode = JFSX_CRC_GEN | JFSX_CRC_BOTH;
    } else if (expect_crc) {
        segs.resize(4 * ns);
        b.crc = segs.data();
        mode = JFSX_CRC_GEN | JFSX_CRC_CT;
    } else if (seg_crc) {
        b.crc = seg_crc;
        mode = JFSX_CRC_GEN;
    }
    rc = open(&b, mode);
    if (rc) return rc;
    if (expect_crc) {
        // the store's read fails first ("verify checksum failed"), before Decrypt sees the bytes
        const uint8_t *ct_segs = seg_crc ? segs.data() + 4 * ns : segs.data();
        if ((rc = jfsx_object_crc32c(o, hdr, ct_segs, len, o + hdr + len, got_crc))) return rc;
        if (*got_crc != *expect_crc) {
            if (len) memset(out, 0, len);
            if (seg_crc) memset(seg_crc, 0, 4 * ns);
            return JFSX_ECRC;
        }
        if (seg_crc) memcpy(seg_crc, segs.data(), 4 * ns);  // zeros when the tag failed
    }
    if (b.status == JFSX_ETAG) return JFSX_ETAG;
    if (out_len) *out_len = len;
    return 0;
}
}  // namespace

extern "C" {

int jfsx_data_encrypt_ex(jfsx_ctx *c, int algo, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *wrapped,
                         int wlen, const void *plaintext, uint64_t len, void *out, uint64_t out_cap, uint64_t *out_len,
                         uint32_t *obj_crc, uint8_t *seg_crc) {
    if (!c) return JFSX_EINVAL;
    return data_encrypt([&](jfsx_blk *b, int m) { return jfsx_seal_batch(c, algo, 1, b, m, JFSX_MEM_HOST); }, algo,
                        key, nonce, wrapped, wlen, plaintext, len, out, out_cap, out_len, obj_crc, seg_crc);
}

int jfsx_data_decrypt_ex(jfsx_ctx *c, int algo, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                         uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc,
                         uint8_t *seg_crc) {
    if (!c || (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305)) return JFSX_EINVAL;
    return data_decrypt([&](jfsx_blk *b, int m) { return jfsx_open_batch(c, algo, 1, b, m, JFSX_MEM_HOST); }, key,
                        obj, olen, out, out_cap, out_len, expect_crc, got_crc, seg_crc);
}

int jfsx_data_encrypt(jfsx_ctx *c, int algo, const uint8_t key[32], const uint8_t nonce[12], const uint8_t *wrapped,
                      int wlen, const void *plaintext, uint64_t len, void *out, uint64_t out_cap, uint64_t *out_len,
                      uint32_t *obj_crc) {
    return jfsx_data_encrypt_ex(c, algo, key, nonce, wrapped, wlen, plaintext, len, out, out_cap, out_len, obj_crc,
                                nullptr);
}

int jfsx_data_decrypt(jfsx_ctx *c, int algo, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                      uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc) {
    return jfsx_data_decrypt_ex(c, algo, key, obj, olen, out, out_cap, out_len, expect_crc, got_crc, nullptr);
}

int jfsx_agg_data_encrypt_ex(jfsx_agg *a, int algo, const uint8_t key[32], const uint8_t nonce[12],
                             const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                             uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc, uint8_t *seg_crc) {
    if (!a) return JFSX_EINVAL;
    return data_encrypt([&](jfsx_blk *b, int m) { return jfsx_agg_seal(a, algo, b, m, JFSX_MEM_HOST); }, algo, key,
                        nonce, wrapped, wlen, plaintext, len, out, out_cap, out_len, obj_crc, seg_crc);
}

int jfsx_agg_data_decrypt_ex(jfsx_agg *a, int algo, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                             uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc,
                             uint8_t *seg_crc) {
    if (!a || (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305)) return JFSX_EINVAL;
    return data_decrypt([&](jfsx_blk *b, int m) { return jfsx_agg_open(a, algo, b, m, JFSX_MEM_HOST); }, key, obj,
                        olen, out, out_cap, out_len, expect_crc, got_crc, seg_crc);
}

int jfsx_agg_data_encrypt(jfsx_agg *a, int algo, const uint8_t key[32], const uint8_t nonce[12],
                          const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                          uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc) {
    return jfsx_agg_data_encrypt_ex(a, algo, key, nonce, wrapped, wlen, plaintext, len, out, out_cap, out_len,
                                    obj_crc, nullptr);
}

int jfsx_agg_data_decrypt(jfsx_agg *a, int algo, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                          uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc) {
    return jfsx_agg_data_decrypt_ex(a, algo, key, obj, olen, out, out_cap, out_len, expect_crc, got_crc, nullptr);
}

int jfsx_gen_synthetic(jfsx_ctx *c, void *dst, uint64_t len, uint64_t seed, uint64_t block) {
    if (!c || (len && !dst) || !aligned16(dst)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    launch_begin();
    if (len) launch_gen_synthetic(c->stream, (uint8_t *)dst, len, seed, block);
    HIP_OK(hipGetLastError());
    return 0;
}

int jfsx_gen_synthetic_batch(jfsx_ctx *c, void *dst, uint64_t stride, int n, const uint64_t *lens, uint64_t seed,
                             uint64_t block0) {
    if (!c || n < 0 || (n && (!dst || !lens)) || !aligned16(dst) || (n > 1 && (stride & 15))) return JFSX_EINVAL;
    for (int i = 0; i < n; i++)
        if (lens[i] > stride && n > 1) return JFSX_EINVAL;
    if (n == 0) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    Workspace &w = c->ws[0];
    int rc;
    if ((rc = ensure_dev(c, &w.d, &w.dcap, 8 * (size_t)n))) return rc;
    if ((rc = ensure_host(&w.h, &w.hcap, 8 * (size_t)n))) return rc;
    memcpy(w.h, lens, 8 * (size_t)n);
    HIP_OK(hipMemcpyAsync(w.d, w.h, 8 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    launch_begin();
    launch_gen_synthetic_batch(c->stream, (uint8_t *)dst, stride, n, (const uint64_t *)w.d, seed, block0);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(c->stream));  // w.h/w.d are reused by the next batch
    return 0;
}

void jfsx_gen_key(uint64_t seed, uint64_t b, uint8_t key[32], uint8_t nonce[12]) {
    auto mix64 = [](uint64_t z) {
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
        return z ^ (z >> 31);
    };
    const uint64_t G = 0x9E3779B97F4A7C15ULL;
    for (int i = 0; i < 4; i++) {
        uint64_t w = mix64((seed ^ 0x4B4559ULL) + G * ((b << 8) + i + 1));
        memcpy(key + 8 * i, &w, 8);
    }
    uint64_t w0 = mix64((seed ^ 0x4E4F4E4345ULL) + G * ((b << 8) + 1));
    uint64_t w1 = mix64((seed ^ 0x4E4F4E4345ULL) + G * ((b << 8) + 2));
    memcpy(nonce, &w0, 8);
    memcpy(nonce + 8, &w1, 4);
}

#ifdef JFSX_KS_PHASES
// The last plain device-resident batch's step outside the main kernel, in
// microseconds.  out[0..8]: the host's intervals between EdgeHost::t's ten
// stamps; out[9..14]: on the stream, the upload, keysetup, keysetup's end to
// the main kernel's start, the main kernel, finalize, the copy-back.
int jfsx_debug_edge_host(double *out) {
    if (!g_edge.ok) return -1;
    for (int i = 0; i < 9; i++) out[i] = (g_edge.t[i + 1] - g_edge.t[i]) * 1e6;
    for (int i = 0; i < 6; i++) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, g_edge.ev[i], g_edge.ev[i + 1]) != hipSuccess) return -1;
        out[9 + i] = ms * 1e3;
    }
    return 0;
}
#endif

// Host-only view of plan_batch (no device, no context), for tests: kind 0 GCM,
// 1 ChaCha20-Poly1305, 2 CRC-only; tasks (nullable): up to cap triples
// (blk, c0, c1) in dispatch order.  Not part of the ABI (undeclared in jfsx.h).
int jfsx_debug_plan(int kind, int n, const uint64_t *lens, uint64_t *task_bytes, uint64_t *ntasks, uint64_t *nslots,
                    uint64_t *tasks, uint64_t cap) {
    if (kind < kPlanGcm || kind > kPlanCrc || n < 0 || (n && !lens)) return JFSX_EINVAL;
    // the per-algorithm length limits of the batch validation (check_aead_args)
    for (int i = 0; i < n; i++)
        if ((kind == kPlanGcm && lens[i] > kGcmMaxLen) || (kind == kPlanCp && lens[i] > kCpMaxLen)) return JFSX_EINVAL;
    const Plan p = plan_batch(kind, std::vector<uint64_t>(lens, lens + n));
    if (task_bytes) *task_bytes = p.task_bytes;
    if (ntasks) *ntasks = p.tasks.size();
    if (nslots) *nslots = p.nslots;
    if (tasks && cap) {
        std::vector<Task> t(std::max<size_t>(p.tasks.size(), 1));
        p.dispatch(t.data());
        for (size_t i = 0; i < std::min<uint64_t>(cap, p.tasks.size()); i++) {
            tasks[3 * i] = t[i].blk;
            tasks[3 * i + 1] = t[i].c0;
            tasks[3 * i + 2] = t[i].c1;
        }
    }
    return 0;
}

int jfsx_debug_tables(uint32_t *aes, uint32_t *crc, uint32_t *crcx) {
    std::vector<uint32_t> a, c, x;
    make_aes_table(a);  // 16384 / 8192 / 192 dwords
    make_crc_tables(c, x);
    if (aes) memcpy(aes, a.data(), 4 * a.size());
    if (crc) memcpy(crc, c.data(), 4 * c.size());
    if (crcx) memcpy(crcx, x.data(), 4 * x.size());
    return 0;
}

// The composed CRC tables of gcm_main's two-row loop (make_crc_tables): tt
// 4096 dwords (TT_0..15), xlb 64.  Not part of the ABI (undeclared in jfsx.h).
int jfsx_debug_crc_composed(uint32_t *tt, uint32_t *xlb) {
    std::vector<uint32_t> c, x, b;
    make_crc_tables(c, x, &b);
    if (tt) memcpy(tt, b.data(), 4 * 4096);
    if (xlb) memcpy(xlb, b.data() + 4096, 4 * 64);
    return 0;
}

// ---------------------------------------------------------------------------
// batched RSA-OAEP key unwrap (rsaEncryptor.Decrypt,
// pkg/object/encrypt.go:124-134 and :207-210)
// ---------------------------------------------------------------------------
struct jfsx_rsa_key {
    int device = 0;
    int kbytes = 0;         // modulus length k: 256 (d_key is a jfsx_rsa::Key) or 512 (a jfsx_rsa::KeyW)
    void *d_key = nullptr;
};

int jfsx_rsa_key_new(jfsx_ctx *c, const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq,
                     const uint8_t *qinv, int prime_bytes, const uint8_t *label, int label_len, jfsx_rsa_key **out) {
    if (!c || !out || !p || !q || !dp || !dq || !qinv || label_len < 0 || (label_len && !label)) return JFSX_EINVAL;
    *out = nullptr;
    // RSA-2048 (1024-bit primes) or RSA-4096 (2048-bit primes); no other size
    const bool wide = prime_bytes == 4 * jfsx_rsa::kLimbsW;
    if (!wide && prime_bytes != 4 * jfsx_rsa::kLimbs) return JFSX_EINVAL;
    // one record of either width, on the heap (KeyW is 5 KiB)
    std::unique_ptr<jfsx_rsa::Key> k2(wide ? nullptr : new jfsx_rsa::Key());
    std::unique_ptr<jfsx_rsa::KeyW> kw(wide ? new jfsx_rsa::KeyW() : nullptr);
    const uint8_t empty = 0;
    const uint8_t *lab = label_len ? label : &empty;
    if (wide ? !jfsx_rsa::key_setup_w(*kw, p, q, dp, dq, qinv, lab, label_len)
             : !jfsx_rsa::key_setup(*k2, p, q, dp, dq, qinv, lab, label_len))
        return JFSX_EINVAL;
    const void *rec = wide ? (const void *)kw.get() : (const void *)k2.get();
    const size_t rec_bytes = wide ? sizeof(jfsx_rsa::KeyW) : sizeof(jfsx_rsa::Key);
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    jfsx_rsa_key *rk = new jfsx_rsa_key();
    rk->device = c->device;
    rk->kbytes = wide ? jfsx_rsa::kModBytesW : jfsx_rsa::kModBytes;
    if (hipMalloc((void **)&rk->d_key, rec_bytes) != hipSuccess) {
        delete rk;
        return JFSX_ENOMEM;
    }
    if (hipMemcpy(rk->d_key, rec, rec_bytes, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(rk->d_key);
        delete rk;
        return JFSX_EIO;
    }
    *out = rk;
    return 0;
}

int jfsx_rsa_key_free(jfsx_rsa_key *k) {
    if (!k) return JFSX_EINVAL;
    (void)hipSetDevice(k->device);
    if (k->d_key) (void)hipFree(k->d_key);
    delete k;
    return 0;
}

int jfsx_rsa_key_bytes(const jfsx_rsa_key *k) { return k ? k->kbytes : JFSX_EINVAL; }

int jfsx_rsa_oaep_decrypt_batch(jfsx_ctx *c, const jfsx_rsa_key *k, int n, const uint8_t *ct, uint64_t ct_stride,
                                const uint32_t *ct_len, uint8_t *msg, uint64_t msg_stride, int32_t *msg_len) {
    if (!c || !k || n < 0 || (n && (!ct || !ct_len || !msg_len || (msg_stride && !msg)))) return JFSX_EINVAL;
    if (n == 0) return 0;
    if (k->device != c->device) return JFSX_EINVAL;
    const size_t K = (size_t)k->kbytes;
    const size_t o_ct = 0, o_mh = align256(K * n), o_em = o_mh + align256(4 * rsa_mh_words(k->kbytes) * (size_t)n),
                 o_len = o_em + align256(K * n), dbytes = o_len + align256(4 * (size_t)n);
    const size_t hbytes = align256(K * n) + align256(4 * (size_t)n);
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_dev(c, &c->rsa_d, &c->rsa_dcap, dbytes))) return rc;
    if ((rc = ensure_host(&c->rsa_h, &c->rsa_hcap, hbytes))) return rc;
    // Go's decrypt rejects a ciphertext longer than the modulus; shorter ones
    // are big-endian integers (left-padded here)
    for (int i = 0; i < n; i++) {
        uint8_t *d = (uint8_t *)c->rsa_h + K * i;
        const uint32_t l = ct_len[i] <= K ? ct_len[i] : 0;
        memset(d, 0, K - l);
        if (l) memcpy(d + K - l, ct + ct_stride * i, l);
    }
    char *d = c->rsa_d;
    HIP_OK(hipMemcpyAsync(d + o_ct, c->rsa_h, K * n, hipMemcpyHostToDevice, c->stream));
    launch_begin();
    launch_rsa_unwrap(c->stream, k->d_key, k->kbytes, n, (const uint8_t *)(d + o_ct), (uint32_t *)(d + o_mh),
                      (uint8_t *)(d + o_em), (int32_t *)(d + o_len));
    HIP_OK(hipGetLastError());
    char *hl = c->rsa_h + align256(K * n);
    HIP_OK(hipMemcpyAsync(c->rsa_h, d + o_em, K * n, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipMemcpyAsync(hl, d + o_len, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) {
        int32_t l = ((const int32_t *)hl)[i];
        if (ct_len[i] > K) l = -1;
        msg_len[i] = l;
        if (l > 0 && msg_stride) memcpy(msg + msg_stride * i, c->rsa_h + K * i, std::min<uint64_t>(l, msg_stride));
    }
    return 0;
}

// batched RSA-OAEP key wrap (rsaEncryptor.Encrypt, encrypt.go:128-130, called
// per object at :169), on the unwrap's stream and grow-only workspace
int jfsx_rsa_oaep_encrypt_batch(jfsx_ctx *c, const jfsx_rsa_key *k, uint32_t e, int n, const uint8_t *msg,
                                uint64_t msg_stride, const uint32_t *msg_len, const uint8_t *seed, uint8_t *ct,
                                uint64_t ct_stride, int32_t *status) {
    constexpr size_t H = jfsx_rsa::kHash;
    if (!c || !k || n < 0 || e < jfsx_rsa::kMinE || e > jfsx_rsa::kMaxE) return JFSX_EINVAL;  // e: Go's checkPub
    const size_t K = (size_t)k->kbytes, S = (size_t)rsa_wrap_slot(k->kbytes);
    if (n == 0) return 0;
    if (!msg_len || !seed || !ct || !status || ct_stride < K) return JFSX_EINVAL;
    for (int i = 0; i < n; i++)
        if (msg_len[i] > msg_stride || (msg_len[i] && !msg)) return JFSX_EINVAL;
    if (k->device != c->device) return JFSX_EINVAL;
    // device: msg slots | seeds | lengths (one copy in) | EM limbs | ct (one copy out)
    const size_t o_msg = 0, o_seed = align256(S * n), o_len = o_seed + align256(H * n),
                 inbytes = o_len + align256(4 * (size_t)n), o_em = inbytes,
                 o_ct = o_em + align256(4 * rsa_em_words(k->kbytes) * (size_t)n), dbytes = o_ct + align256(K * n);
    const size_t hbytes = std::max(inbytes, K * n);
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    int rc;
    if ((rc = ensure_dev(c, &c->rsa_d, &c->rsa_dcap, dbytes))) return rc;
    if ((rc = ensure_host(&c->rsa_h, &c->rsa_hcap, hbytes))) return rc;
    char *h = c->rsa_h;
    memset(h, 0, inbytes);
    for (int i = 0; i < n; i++) {
        // Go: "message too long for RSA key size"; the kernels give such an item k zero bytes
        status[i] = msg_len[i] > (uint32_t)(K - 2 * H - 2) ? -1 : 0;
        if (status[i] == 0 && msg_len[i]) memcpy(h + o_msg + S * i, msg + msg_stride * i, msg_len[i]);
        memcpy(h + o_seed + H * i, seed + H * i, H);
        ((uint32_t *)(h + o_len))[i] = msg_len[i];
    }
    char *d = c->rsa_d;
    HIP_OK(hipMemcpyAsync(d, h, inbytes, hipMemcpyHostToDevice, c->stream));
    launch_begin();
    launch_rsa_wrap(c->stream, k->d_key, k->kbytes, e, n, (const uint8_t *)(d + o_msg), (const uint32_t *)(d + o_len),
                    (const uint8_t *)(d + o_seed), (uint32_t *)(d + o_em), (uint8_t *)(d + o_ct));
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h, d + o_ct, K * n, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int i = 0; i < n; i++) memcpy(ct + ct_stride * i, h + K * i, K);
    return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------
// jfsx_load_objects: checksum verify -> key unwrap -> Open -> decompress ->
// checksum() of a batch of stored objects in one call (checksumReader,
// checksum.go:55-82; dataEncryptor.Decrypt, encrypt.go:196-216;
// cachedStore.load, cached_store.go:673-748).  jfsx_load_batch's chain
// (load_enqueue) with the two stages a reader ran around it in front, on the
// same stream and in the same grow-only buffers; jfsx_objload.hip has the order
// and the gate rule.  The host still plans everything from the lengths alone
// and waits once.
// ---------------------------------------------------------------------------
namespace {

int check_objects_args(const jfsx_rsa_key *key, int algo, int codec, int n, const jfsx_oblk *blks, int crc_mode,
                       int mem) {
    const bool cipher = algo != JFSX_CIPHER_NONE, coded = codec != JFSX_CODEC_NONE;
    if (cipher && algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;
    if (coded && codec != JFSX_CODEC_LZ4 && codec != JFSX_CODEC_ZSTD) return JFSX_EINVAL;
    if (!cipher && !coded) return JFSX_EINVAL;  // jfsx_crc32c_segments serves that volume
    if (crc_mode < 0 || (crc_mode & ~(JFSX_CRC_GEN | JFSX_CRC_CT))) return JFSX_EINVAL;
    if (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST) return JFSX_EINVAL;
    if (n < 0 || cipher != (key != nullptr)) return JFSX_EINVAL;
    const bool crc = (crc_mode & JFSX_CRC_GEN) != 0, ct = (crc_mode & JFSX_CRC_CT) != 0;
    for (int i = 0; i < n; i++) {
        const jfsx_oblk &b = blks[i];
        if (b.reserved || (b.hdr_len && (!b.hdr || !cipher))) return JFSX_EINVAL;
        if ((b.src_len && !b.src) || (b.len && !b.dst)) return JFSX_EINVAL;
        if (!coded && b.src_len != b.len) return JFSX_EINVAL;
        // check_load_args' limits
        if (b.src_len > kLz4MaxInput || b.len >= ((uint64_t)1 << 32)) return JFSX_EINVAL;
        if (codec == JFSX_CODEC_ZSTD && b.len >= ((uint64_t)1 << 31)) return JFSX_EINVAL;
        if (crc && !b.crc) return JFSX_EINVAL;
        if (mem == JFSX_MEM_DEVICE) {
            // Open and the image CRC pass read src, Open (no codec) writes dst, the page CRC pass reads dst
            if ((cipher || ct) && b.src_len && !aligned16(b.src)) return JFSX_EINVAL;
            if ((crc || !coded) && b.len && !aligned16(b.dst)) return JFSX_EINVAL;
            if (b.dst && b.dst == b.src) return JFSX_EINVAL;
        }
    }
    return 0;
}

struct ObjLoadState {
    HostStage hs;
    std::vector<size_t> poff;
    size_t h_res = 0, st_off = 0, crc_off = 0;  // the download in load_h; ObjState[n] and CRC words behind LoadRes[n]
    int zd_waves = 0;
    bool aead = false, crc = false, ct = false, coded = false;
};

int objects_enqueue(jfsx_ctx *c, const jfsx_rsa_key *key, int algo, int codec, int n, const jfsx_oblk *blks,
                    int crc_mode, bool host, ObjLoadState &st) {
    hipStream_t s = c->stream;
    const bool aead = st.aead = algo != JFSX_CIPHER_NONE;
    const bool crc = st.crc = (crc_mode & JFSX_CRC_GEN) != 0;
    const bool ct = st.ct = (crc_mode & JFSX_CRC_CT) != 0;
    const bool coded = st.coded = codec != JFSX_CODEC_NONE;
    const bool zstd = codec == JFSX_CODEC_ZSTD;
    const int kbytes = key ? key->kbytes : jfsx_rsa::kModBytes;  // the modulus length k of the volume's key
    const size_t K = (size_t)kbytes;
    std::vector<size_t> ioff(n);
    st.poff.assign(n, 0);
    size_t img_bytes = 0, page_bytes = 0;
    uint64_t crc_words = 0, ct_words = 0, max_len = 0;
    for (int i = 0; i < n; i++) {
        ioff[i] = img_bytes;
        img_bytes += align256(blks[i].src_len);
        st.poff[i] = page_bytes;
        page_bytes += align256(blks[i].len);
        crc_words += nseg_of(blks[i].len);
        ct_words += nseg_of(blks[i].src_len);
        max_len = std::max<uint64_t>(max_len, blks[i].len);
    }
    // device workspace: load_enqueue's, with ObjBlk behind LoadBlk (one upload)
    // and ObjState behind LoadRes (one download)
    size_t off = 0;
    const size_t o_lb = off; off = align256(off + sizeof(LoadBlk) * n);
    const size_t o_ob = off; off = align256(off + sizeof(ObjBlk) * n);
    const size_t up = off;
    const size_t o_z = off; off = align256(off + sizeof(ZDev) * n);
    const size_t o_zo = off; off = align256(off + sizeof(ZOut) * n);
    const size_t o_res = off; off = align256(off + sizeof(LoadRes) * n);
    const size_t o_st = off; off = align256(off + sizeof(ObjState) * n);
    const size_t o_crc = off; if (host && crc) off = align256(off + 4 * crc_words);
    const size_t down = off - o_res;
    const size_t o_ct = off; if (ct) off = align256(off + 4 * ct_words);
    const size_t o_tab = off;
    st.h_res = up;
    st.st_off = o_st - o_res;
    st.crc_off = o_crc - o_res;
    // the unwrap's workspace, as jfsx_rsa_oaep_decrypt_batch lays it out
    const size_t r_ct = 0, r_mh = align256(K * n), r_em = r_mh + align256(4 * rsa_mh_words(kbytes) * (size_t)n),
                 r_len = r_em + align256(K * n), r_bytes = r_len + align256(4 * (size_t)n);
    int rc;
    // every buffer of the path before the first enqueue
    if (zstd) {
        st.zd_waves = zstd_decode_waves(c, n);
        rc = ensure_zstd_decode(c, &c->load_d, &c->load_dcap, o_tab, n, &st.zd_waves);
    } else {
        rc = ensure_dev(c, &c->load_d, &c->load_dcap, o_tab);
    }
    if (rc) return rc;
    if ((rc = ensure_host(&c->load_h, &c->load_hcap, up + down))) return rc;
    // device memory without a codec: Open reads src and writes the page itself
    const size_t stage_need = host ? img_bytes + page_bytes : (aead && coded) ? img_bytes : 0;
    if (stage_need && (rc = ensure_dev(c, &c->load_stage, &c->load_scap, stage_need))) return rc;
    if (aead) {
        if ((rc = ensure_dev(c, &c->rsa_d, &c->rsa_dcap, r_bytes))) return rc;
        if ((rc = ensure_host(&c->rsa_h, &c->rsa_hcap, align256(K * n)))) return rc;
    }
    char *d = c->load_d, *h = c->load_h, *stage = c->load_stage;
    // host: the stored bytes up and the pages down, as load_enqueue stages them
    std::vector<StageItem> up_items, down_items;
    if (host) {
        st.hs.resize(n, n);
        for (int i = 0; i < n; i++) {
            const jfsx_oblk &b = blks[i];
            if (b.src_len) HostStage::mark(st.hs.in, i, b.src, b.src_len);
            if (b.len) HostStage::mark(st.hs.out, i, b.dst, b.len);
            up_items.push_back({(void *)b.src, stage + ioff[i], ioff[i], b.src_len, (size_t)i});
            down_items.push_back({b.dst, stage + img_bytes + st.poff[i], st.poff[i], b.len, (size_t)i});
        }
        if ((rc = st.hs.reserve(c, img_bytes, page_bytes))) return rc;
    }
    // block records; the blocks of the image CRC, Open and page CRC stages; the wrapped keys
    LoadBlk *hl = (LoadBlk *)(h + o_lb);
    ObjBlk *ho = (ObjBlk *)(h + o_ob);
    std::vector<jfsx_blk> ab(aead ? n : 0), cb(crc && coded ? n : 0), tb(ct ? n : 0);
    uint64_t cw = 0, tw = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_oblk &b = blks[i];
        // raw: the stored bytes in device memory; img: what the decoder reads
        uint8_t *raw = host ? (uint8_t *)(stage + ioff[i]) : (uint8_t *)b.src;
        uint8_t *img = host || (aead && coded) ? (uint8_t *)(stage + ioff[i]) : (uint8_t *)b.src;
        if (!b.src_len) raw = img = nullptr;
        hl[i].img = img;
        hl[i].dst = !b.len ? nullptr : host ? (uint8_t *)(stage + img_bytes + st.poff[i]) : (uint8_t *)b.dst;
        hl[i].crc = !crc ? nullptr : host ? (uint8_t *)(d + o_crc + 4 * cw) : b.crc;
        hl[i].src_len = b.src_len;
        hl[i].len = b.len;
        cw += nseg_of(b.len);
        ObjBlk &o = ho[i];
        memset(&o, 0, sizeof(o));
        o.segs = ct ? (const uint8_t *)(d + o_ct + 4 * tw) : nullptr;
        o.clen = b.src_len;
        o.expect = b.expect_crc;
        tw += nseg_of(b.src_len);
        if (ct) {
            jfsx_blk &k = tb[i];
            memset(&k, 0, sizeof(k));
            k.src = raw;
            k.len = b.src_len;
            k.crc = (uint8_t *)o.segs;
        }
        if (aead) {
            // dataEncryptor.Decrypt's header parse (encrypt.go:197-205); the
            // sizes that make the unwrap or Open fail without running are flags
            const uint8_t *hd = (const uint8_t *)b.hdr;
            uint8_t *w = (uint8_t *)c->rsa_h + K * i;
            memset(w, 0, K);
            jfsx_blk &a = ab[i];
            memset(&a, 0, sizeof(a));
            const uint32_t kl = b.hdr_len >= 3 ? ((uint32_t)hd[0] << 8) + hd[1] : 0, nl = b.hdr_len >= 3 ? hd[2] : 0;
            if (b.hdr_len < 3 || b.hdr_len != 3 + kl + nl) {
                o.flags |= jfsx_obj::kHdrBad;
            } else {
                if (kl == 0 || kl > K) o.flags |= jfsx_obj::kKeyBad;
                else memcpy(w + K - kl, hd + 3, kl);  // a big-endian integer, left-padded
                if (nl != 12) o.flags |= jfsx_obj::kNonceBad;
                else memcpy(a.nonce, hd + 3 + kl, 12);
            }
            o.crc_hdr = jfsx_crc32c_update(0, hd, b.hdr_len);
            o.crc_tag = jfsx_crc32c_update(0, b.tag, 16);
            memcpy(a.tag, b.tag, 16);
            a.src = raw;
            a.dst = coded ? img : hl[i].dst;
            a.len = b.src_len;
            a.crc = coded ? nullptr : hl[i].crc;
        }
        if (crc && coded) {
            jfsx_blk &k = cb[i];
            memset(&k, 0, sizeof(k));
            k.src = hl[i].dst;
            k.len = b.len;
            k.crc = hl[i].crc;
        }
    }
    // 1. records, images (host) and wrapped keys up
    HIP_OK(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemsetAsync(d + o_st, 0, sizeof(ObjState) * n, s));
    if (host && (rc = st.hs.upload(s, stage, img_bytes, up_items))) return rc;
    char *r = c->rsa_d;
    if (aead) HIP_OK(hipMemcpyAsync(r + r_ct, c->rsa_h, K * n, hipMemcpyHostToDevice, s));
    const LoadBlk *dl = (const LoadBlk *)(d + o_lb);
    const ObjBlk *dob = (const ObjBlk *)(d + o_ob);
    ObjState *dst = (ObjState *)(d + o_st);
    ZDev *dz = (ZDev *)(d + o_z);
    ZOut *dzo = (ZOut *)(d + o_zo);
    LoadRes *dres = (LoadRes *)(d + o_res);
    // 2. segment CRCs of every image, before Open overwrites a host batch's in place
    if (ct && (rc = enqueue_crc(c, c->obj_ct, s, c->obj_ev[0], c->obj_ev[1], n, tb.data(), JFSX_CRC_GEN, nullptr,
                                nullptr, false)))
        return rc;
    // 3. the unwrap, 4. the fold
    launch_begin();
    if (aead)
        launch_rsa_unwrap(s, key->d_key, kbytes, n, (const uint8_t *)(r + r_ct), (uint32_t *)(r + r_mh),
                          (uint8_t *)(r + r_em), (int32_t *)(r + r_len));
    if (ct) launch_obj_fold(s, n, dob, aead ? 16 : 0, c->tabs.crcx + 64, dst);
    HIP_OK(hipGetLastError());
    // 5. the keys into Open's KeyIn[n], 6. Open: into the staging buffer for
    // the decoder, or into the page with the fused CRC_GEN
    const BlkOut *opened = nullptr;
    if (aead) {
        const KeyHook hook = [&](hipStream_t ks, KeyIn *dk) {
            launch_obj_keys(ks, n, dob, dst, (uint8_t *)(r + r_em), kbytes, (const int32_t *)(r + r_len), dk);
        };
        if ((rc = enqueue_aead(c, c->load_aead, s, c->load_ev[0], c->load_ev[1], algo, true, n, ab.data(),
                               !coded && crc ? JFSX_CRC_GEN : JFSX_CRC_NONE, nullptr, nullptr, false, nullptr, nullptr,
                               false, false, nullptr, nullptr, &hook)))
            return rc;
        opened = (const BlkOut *)c->load_aead.dout;
    }
    // 7. the gate and the decoder, then checksum() of every page
    if (coded) {
        launch_begin();
        launch_obj_gate(s, n, dl, dob, dst, opened, ct, dz, dzo);
        if (zstd) launch_zstd_decompress(s, n, dz, dzo, (uint8_t *)(d + o_tab), st.zd_waves);
        else launch_lz4_decompress(s, n, dz, dzo);
        HIP_OK(hipGetLastError());
        if (crc && (rc = enqueue_crc(c, c->load_crc, s, c->load_ev[2], c->load_ev[3], n, cb.data(), JFSX_CRC_GEN,
                                     nullptr, nullptr, false)))
            return rc;
    }
    // 8. verdicts; pages and CRC arrays of failed blocks zeroed; one download
    launch_begin();
    const int groups = (int)std::min<uint64_t>(1024, std::max<uint64_t>(1, (max_len + 65535) / 65536));
    launch_obj_verdict(s, n, dl, dob, dst, opened, coded ? dzo : nullptr, ct, zstd && st.zd_waves > 0, dres);
    launch_load_wipe(s, n, groups, dl, dres, crc);
    HIP_OK(hipGetLastError());
    HIP_OK(hipMemcpyAsync(h + st.h_res, d + o_res, down, hipMemcpyDeviceToHost, s));
    if (host) return st.hs.download(s, stage + img_bytes, page_bytes, std::move(down_items));
    return 0;
}

// Under c->mu for the whole call, as run_load.
int run_objects(jfsx_ctx *c, const jfsx_rsa_key *key, int algo, int codec, int n, jfsx_oblk *blks, int crc_mode,
                int mem) {
    const bool host = mem == JFSX_MEM_HOST;
    ObjLoadState st;
    int rc = objects_enqueue(c, key, algo, codec, n, blks, crc_mode, host, st);
    rc = wait_stream(c, rc, "hipStreamSynchronize(load_objects)");
    settle_stage(c, c->load_aead, c->load_ev[0], c->load_ev[1], !rc);
    settle_stage(c, c->load_crc, c->load_ev[2], c->load_ev[3], !rc);
    settle_stage(c, c->obj_ct, c->obj_ev[0], c->obj_ev[1], !rc);
    if (!rc) {
        const LoadRes *hr = (const LoadRes *)(c->load_h + st.h_res);
        const ObjState *hs = (const ObjState *)(c->load_h + st.h_res + st.st_off);
        const char *hw = c->load_h + st.h_res + st.crc_off;
        for (int i = 0; i < n; i++) {
            jfsx_oblk &b = blks[i];
            b.status = hr[i].status;
            b.out_len = hr[i].out_len;
            b.codec_info = hr[i].codec_info;
            b.key_len = st.aead ? hs[i].key_len : 0;
            if (st.ct) b.obj_crc = hs[i].obj_crc;
            if (host && st.crc) {
                memcpy(b.crc, hw, 4 * nseg_of(b.len));
                hw += 4 * nseg_of(b.len);
            }
        }
        st.hs.copy_out();
    }
    if (rc) return rc;
    // jfsx_ctx_metrics: what the separate calls would have counted
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &m = c->met;
    const bool zstd = codec == JFSX_CODEC_ZSTD;
    uint64_t &d_blocks = zstd ? m.zstdd_blocks : m.lz4d_blocks, &d_in = zstd ? m.zstdd_in : m.lz4d_in;
    uint64_t &d_out = zstd ? m.zstdd_out : m.lz4d_out, &d_fail = zstd ? m.zstdd_fail : m.lz4d_fail;
    if (st.aead) m.open_batches++;
    m.crc_batches += (st.crc ? 1 : 0) + (st.ct ? 1 : 0);
    for (int i = 0; i < n; i++) {
        const jfsx_oblk &b = blks[i];
        const bool keyed = b.status != JFSX_ECRC && b.status != JFSX_EHEADER && b.status != JFSX_EKEY;
        if (st.aead && keyed) {
            m.open_blocks++;
            m.open_bytes += b.src_len;
            m.open_fail += b.status == JFSX_ETAG;
        }
        if (st.coded && keyed && b.status != JFSX_ETAG) {  // the block reached the decoder
            d_blocks++;
            d_in += b.src_len;
            d_out += b.out_len;
            d_fail += b.status == JFSX_EFORMAT || b.status == JFSX_EDSTSIZE;
            if (zstd && b.codec_info) m.zstd_serial++;
        }
        if (st.crc) {
            m.crc_ranges++;
            m.crc_bytes += b.len;
        }
        if (st.ct) {
            m.crc_ranges++;
            m.crc_bytes += b.src_len;
            m.crc_fail += b.status == JFSX_ECRC;
        }
    }
    return 0;
}

}  // namespace

extern "C" int jfsx_load_objects(jfsx_ctx *c, const jfsx_rsa_key *key, int algo, int codec, int n, jfsx_oblk *blks,
                                 int crc_mode, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    // argument errors before the context or its device is touched
    const int rc = check_objects_args(key, algo, codec, n, blks, crc_mode, mem);
    if (rc || n == 0) return rc;
    if (key && key->device != c->device) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_objects(c, key, algo, codec, n, blks, crc_mode, mem);
}

// ---------------------------------------------------------------------------
// jfsx_store_objects: key wrap -> verify / checksum() -> compress -> Seal ->
// header and tag -> object checksum of a batch of pages in one call
// (dataEncryptor.Encrypt, encrypt.go:164-194; generateChecksum,
// checksum.go:31-53).  jfsx_store_batch's chain (store_phase_a) with the wrap
// in front, on the same stream and in the same grow-only buffers, and a phase
// B of its own: the Seal writes C where the object has it, and sobj_frame_k
// puts the header and the tag around it and folds obj_crc, so the host
// assembles and folds nothing.  jfsx_objstore.hip has the order.
// ---------------------------------------------------------------------------
namespace {

// header and tag around C for a key whose modulus is kbytes long: 287, or 543
// with a 4096-bit key.  15 + kbytes is 15 mod 16 for both, so the rule "obj is
// 1 mod 16" puts C on 16 bytes at either width.
constexpr uint64_t obj_hdr(int kbytes) { return 3 + (uint64_t)kbytes + 12; }
constexpr uint64_t obj_frame(int kbytes) { return obj_hdr(kbytes) + JFSX_OBJ_TAG_BYTES; }
static_assert(obj_hdr(jfsx_rsa::kModBytes) == JFSX_OBJ_HDR_BYTES, "the public header's RSA-2048 figure");
static_assert(obj_hdr(jfsx_rsa::kModBytes) % 16 == 15 && obj_hdr(jfsx_rsa::kModBytesW) % 16 == 15, "C's alignment");
// a host batch's object in the packed device image and in the bounce buffer:
// one byte into a 16-byte aligned slot, so that C is 16-byte aligned
constexpr size_t kObjLead = 1;
inline size_t obj_slot(int kbytes, uint64_t img_len) { return align16(kObjLead + obj_frame(kbytes) + img_len); }

uint64_t object_bound(int kbytes, int codec, uint64_t len) {
    if (codec != JFSX_CODEC_NONE && codec != JFSX_CODEC_LZ4 && codec != JFSX_CODEC_ZSTD) return 0;
    const uint64_t img = codec == JFSX_CODEC_ZSTD ? zstd_bound(len) : codec == JFSX_CODEC_LZ4 ? lz4_bound(len) : len;
    if (codec == JFSX_CODEC_LZ4 && !img) return 0;  // past jfsx_lz4_bound's domain
    return obj_frame(kbytes) + img;
}

int check_sobj_args(const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n, const jfsx_soblk *blks,
                    int crc_mode, int mem) {
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;  // no cipher: jfsx_store_batch
    if (codec != JFSX_CODEC_NONE && codec != JFSX_CODEC_LZ4 && codec != JFSX_CODEC_ZSTD) return JFSX_EINVAL;
    if (crc_mode < 0 || (crc_mode & ~(3 | JFSX_CRC_CT)) || (crc_mode & 3) == 3) return JFSX_EINVAL;
    if (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST) return JFSX_EINVAL;
    if (n < 0 || !key || e < jfsx_rsa::kMinE || e > jfsx_rsa::kMaxE) return JFSX_EINVAL;
    const bool coded = codec != JFSX_CODEC_NONE, page_crc = (crc_mode & 3) != 0;
    for (int i = 0; i < n; i++) {
        const jfsx_soblk &b = blks[i];
        if (b.reserved || b.reserved2) return JFSX_EINVAL;
        if ((b.len && !b.src) || !b.obj) return JFSX_EINVAL;
        if (coded && b.len > kLz4MaxInput) return JFSX_EINVAL;
        const uint64_t img = codec == JFSX_CODEC_ZSTD ? zstd_bound(b.len) : coded ? lz4_bound(b.len) : b.len;
        if (algo == JFSX_AES256GCM && img > kGcmMaxLen) return JFSX_EINVAL;
        if (algo == JFSX_CHACHA20P1305 && img > kCpMaxLen) return JFSX_EINVAL;
        // the smallest bound of any key: the key itself is not looked at here
        // (check_sobj_caps has its bound, once the key is known to be one)
        if (b.obj_cap < obj_frame(jfsx_rsa::kModBytes) + img) return JFSX_EINVAL;
        if (page_crc && !b.crc) return JFSX_EINVAL;
        if (mem == JFSX_MEM_DEVICE) {
            if (((uintptr_t)b.obj & 15) != 1) return JFSX_EINVAL;
            // the page CRC and, without a codec, the Seal read src where it lies
            if ((page_crc || !coded) && b.len && !aligned16(b.src)) return JFSX_EINVAL;
            if (b.obj == b.src) return JFSX_EINVAL;
        }
    }
    return 0;
}

// obj_cap against the key's own bound (543 + the image bound at 4096 bits);
// the blocks have passed check_sobj_args
int check_sobj_caps(const jfsx_rsa_key *key, int codec, int n, const jfsx_soblk *blks) {
    for (int i = 0; i < n; i++)
        if (blks[i].obj_cap < object_bound(key->kbytes, codec, blks[i].len)) return JFSX_EINVAL;
    return 0;
}

struct SobjState {
    StoreState st;
    std::vector<StoreRes> res;     // per block: what phase A found (wait #1), or OK / len without one
    std::vector<size_t> seg_word;  // per sealed block: its first word in the Seal's CRC words
    bool seal_pages = false;       // JFSX_CODEC_NONE with GEN: the Seal's fused pass writes the page CRCs
    int seal_mult = 1;
    size_t out_bytes = 0;
    size_t o_msg = 0, o_ct = 0, msg_bytes = 0;  // the wrap's workspace
    int kbytes = 0;                             // the key's modulus length: the wrapped key in every header
    size_t h_sres = 0;                          // the downloaded SobjRes[m] in store_h
};
// jfsx_compact_objects: more downloads behind phase B's, in front of its wait
using SobjTail = std::function<int(const SobjState &)>;

// The wrap, in jfsx_rsa_oaep_encrypt_batch's layout: msg | seed | len up in
// one copy, the k-byte results left at o_ct.
int sobj_wrap(jfsx_ctx *c, const jfsx_rsa_key *key, uint32_t e, int n, const jfsx_soblk *blks, SobjState &so) {
    constexpr size_t H = jfsx_rsa::kHash;
    const size_t K = (size_t)key->kbytes, S = (size_t)rsa_wrap_slot(key->kbytes);
    const size_t o_msg = 0, o_seed = align256(S * n), o_len = o_seed + align256(H * n),
                 inbytes = o_len + align256(4 * (size_t)n), o_em = inbytes,
                 o_ct = o_em + align256(4 * rsa_em_words(key->kbytes) * (size_t)n), dbytes = o_ct + align256(K * n);
    so.kbytes = key->kbytes;
    int rc;
    if ((rc = ensure_dev(c, &c->rsa_d, &c->rsa_dcap, dbytes))) return rc;
    if ((rc = ensure_host(&c->rsa_h, &c->rsa_hcap, std::max(inbytes, K * n)))) return rc;
    char *h = c->rsa_h, *d = c->rsa_d;
    memset(h, 0, inbytes);
    for (int i = 0; i < n; i++) {
        memcpy(h + o_msg + S * i, blks[i].key, 32);
        memcpy(h + o_seed + H * i, blks[i].seed, H);
        ((uint32_t *)(h + o_len))[i] = 32;
    }
    so.o_msg = o_msg;
    so.o_ct = o_ct;
    so.msg_bytes = S * n;
    HIP_OK(hipMemcpyAsync(d, h, inbytes, hipMemcpyHostToDevice, c->stream));
    launch_begin();
    launch_rsa_wrap(c->stream, key->d_key, key->kbytes, e, n, (const uint8_t *)(d + o_msg),
                    (const uint32_t *)(d + o_len), (const uint8_t *)(d + o_seed), (uint32_t *)(d + o_em),
                    (uint8_t *)(d + o_ct));
    HIP_OK(hipGetLastError());
    return 0;
}

// Phase B: the Seal over the OK blocks into the objects (device memory) or the
// packed device image (host memory), the frame, and every download.
int sobj_phase_b(jfsx_ctx *c, int algo, int n, const jfsx_soblk *blks, SobjState &so, const SobjTail *tail) {
    StoreState &st = so.st;
    hipStream_t s = c->stream;
    const bool host = st.host;
    st.ooff.assign(n, 0);
    size_t out_bytes = 0;
    for (int i = 0; i < n; i++) {
        if (so.res[i].status == jfsx_store::kBroken) return JFSX_EIO;
        if (so.res[i].status != JFSX_OK) continue;
        st.okidx.push_back(i);
        st.ooff[i] = out_bytes;
        out_bytes += obj_slot(so.kbytes, so.res[i].out_len);
    }
    so.out_bytes = out_bytes;
    const int m = (int)st.okidx.size();
    if (!m) return 0;
    so.seal_pages = st.plain && st.page_mode == JFSX_CRC_GEN;
    const int seal_mode = so.seal_pages ? (st.ct ? (JFSX_CRC_GEN | JFSX_CRC_BOTH) : JFSX_CRC_GEN)
                          : st.ct      ? (JFSX_CRC_GEN | JFSX_CRC_CT)
                                       : JFSX_CRC_NONE;
    so.seal_mult = so.seal_pages && st.ct ? 2 : 1;
    // workspace: SobjBlk[m] up, SobjRes[m] down, behind phase A's records
    const size_t o_sb = align256(st.h_res + sizeof(StoreRes) * n), o_res = align256(o_sb + sizeof(SobjBlk) * m),
                 total = align256(o_res + sizeof(SobjRes) * m);
    int rc;
    if ((rc = ensure_host(&c->store_h, &c->store_hcap, total))) return rc;
    if (host && (rc = ensure_dev(c, &c->store_img, &c->store_icap, out_bytes))) return rc;
    // store_d is free again: phase A's kernels have finished (wait #1), or none of them ran
    if ((rc = ensure_dev(c, &c->store_d, &c->store_dcap, total))) return rc;
    so.h_sres = o_res;
    SobjBlk *hb = (SobjBlk *)(c->store_h + o_sb);
    st.sb.assign(m, jfsx_blk{});
    so.seg_word.assign(m, 0);
    static uint8_t crc_unused[8];  // never written: the CRC words stay in the Seal's workspace (host_crc)
    size_t cw = 0;
    for (int k = 0; k < m; k++) {
        const int i = st.okidx[k];
        const jfsx_soblk &b = blks[i];
        const uint64_t img_len = so.res[i].out_len;
        uint8_t *obj = host ? (uint8_t *)(c->store_img + st.ooff[i] + kObjLead) : (uint8_t *)b.obj;
        jfsx_blk &a = st.sb[k];
        memset(&a, 0, sizeof(a));
        a.src = st.plain ? (!b.len ? nullptr : host ? (const void *)(c->store_stage + st.poff[i]) : b.src)
                         : (const void *)(st.slots + st.zoff[i]);
        a.dst = obj + obj_hdr(so.kbytes);
        a.len = img_len;
        memcpy(a.nonce, b.nonce, 12);  // the key comes from the wrap's message slot (sobj_keys_k)
        a.crc = seal_mode ? crc_unused : nullptr;
        so.seg_word[k] = cw;
        memset(&hb[k], 0, sizeof(SobjBlk));
        hb[k].obj = obj;
        hb[k].img_len = img_len;
        memcpy(hb[k].nonce, b.nonce, 12);
        hb[k].idx = (uint32_t)i;
        hb[k].seg_off = (uint32_t)(cw + (so.seal_mult == 2 ? nseg_of(img_len) : 0));
        cw += so.seal_mult * nseg_of(img_len);
    }
    char *d = c->store_d;
    const SobjBlk *dsb = (const SobjBlk *)(d + o_sb);
    HIP_OK(hipMemcpyAsync(d + o_sb, c->store_h + o_sb, sizeof(SobjBlk) * m, hipMemcpyHostToDevice, s));
    const uint8_t *msg = (const uint8_t *)(c->rsa_d + so.o_msg);
    const KeyHook hook = [&](hipStream_t ks, KeyIn *dk) { launch_sobj_keys(ks, m, dsb, msg, so.kbytes, dk); };
    if ((rc = enqueue_aead(c, c->store_aead, s, c->store_ev[2], c->store_ev[3], algo, false, m, st.sb.data(),
                           seal_mode, nullptr, nullptr, false, nullptr, nullptr, seal_mode != 0, false, nullptr,
                           nullptr, &hook)))
        return rc;
    Workspace &w = c->store_aead;
    const uint8_t *words = (const uint8_t *)w.dout + w.crc_off;
    launch_begin();
    launch_sobj_frame(s, m, dsb, (const uint8_t *)(c->rsa_d + so.o_ct), so.kbytes, (const BlkOut *)w.dout, st.ct ? words : nullptr,
                      st.ct, c->tabs.crcx + 64, (SobjRes *)(d + o_res));
    HIP_OK(hipGetLastError());
    // the keys have reached the Seal's schedules: no copy stays in the wrap's workspace
    HIP_OK(hipMemsetAsync(c->rsa_d + so.o_msg, 0, so.msg_bytes, s));
    // downloads: the results, the page CRC words, the objects
    HIP_OK(hipMemcpyAsync(c->store_h + o_res, d + o_res, sizeof(SobjRes) * m, hipMemcpyDeviceToHost, s));
    if (st.page_mode && !st.plain) {
        Workspace &pw = c->store_crc;
        HIP_OK(hipMemcpyAsync(pw.h + pw.res_off, pw.dout, pw.down, hipMemcpyDeviceToHost, s));
    }
    if (so.seal_pages) {
        if (host) {
            HIP_OK(hipMemcpyAsync(w.h, w.dout, w.down, hipMemcpyDeviceToHost, s));
        } else {
            for (int k = 0; k < m; k++) {
                const jfsx_soblk &b = blks[st.okidx[k]];
                HIP_OK(hipMemcpyAsync(b.crc, words + 4 * so.seg_word[k], 4 * nseg_of(b.len), hipMemcpyDeviceToDevice,
                                      s));
            }
        }
    }
    if (host) {
        std::vector<StageItem> items;
        for (int i : st.okidx) {
            const size_t at = st.ooff[i] + kObjLead;
            items.push_back({blks[i].obj, c->store_img + at, at, obj_frame(so.kbytes) + so.res[i].out_len, (size_t)i});
        }
        if ((rc = st.hs.download(s, c->store_img, out_bytes, std::move(items)))) return rc;
    }
    return tail ? (*tail)(so) : 0;
}

// Under c->mu for the whole call; the arguments have passed check_sobj_args and n > 0.
int run_store_objects(jfsx_ctx *c, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n, jfsx_soblk *blks,
                      int crc_mode, int mem, const SobjTail *tail = nullptr) {
    int rc = 0;
    SobjState so;
    StoreState &st = so.st;
    st.host = mem == JFSX_MEM_HOST;
    st.aead = true;
    st.ct = (crc_mode & JFSX_CRC_CT) != 0;
    st.zstd = codec == JFSX_CODEC_ZSTD;
    st.plain = codec == JFSX_CODEC_NONE;
    st.page_mode = crc_mode & 3;
    st.obj_extra = kObjLead + obj_frame(key->kbytes) + 15;
    // the blocks as store_phase_a takes them; dst is looked at (pinned or not), never written
    std::vector<jfsx_sblk> sh(n);
    for (int i = 0; i < n; i++) {
        jfsx_sblk &b = sh[i];
        memset(&b, 0, sizeof(b));
        b.src = blks[i].src;
        b.len = blks[i].len;
        b.dst = blks[i].obj;
        b.dst_cap = blks[i].obj_cap - obj_frame(key->kbytes);
        b.crc = blks[i].crc;
    }
    const bool verify = st.page_mode == JFSX_CRC_VERIFY, wait1 = !st.plain || verify;
    rc = sobj_wrap(c, key, e, n, blks, so);
    if (!rc) rc = store_phase_a(c, n, sh.data(), st);
    if (wait1 || rc) rc = wait_stream(c, rc, "hipStreamSynchronize(store_objects, wait #1)");
    bool crc_done = false;  // the page CRC stage's results are in its mirror
    if (!rc) {
        so.res.assign(n, StoreRes{});
        if (!st.plain) {
            memcpy(so.res.data(), c->store_h + st.h_res, sizeof(StoreRes) * n);
        } else {
            if (verify) {
                rc = finish_aead(c, c->store_crc, c->store_ev[0], c->store_ev[1], true, st.pb.data());
                crc_done = true;
            }
            for (int i = 0; i < n && !rc; i++) {
                StoreRes &r = so.res[i];
                r.status = verify ? st.pb[i].status : JFSX_OK;
                r.out_len = r.status == JFSX_OK ? blks[i].len : 0;
                r.bad_seg = verify ? st.pb[i].crc_bad_seg : -1;
                r.got = verify ? st.pb[i].crc_got : 0;
                r.expect = verify ? st.pb[i].crc_expect : 0;
            }
        }
    }
    if (!rc) {
        rc = sobj_phase_b(c, algo, n, blks, so, tail);
        rc = wait_stream(c, rc, "hipStreamSynchronize(store_objects, wait #2)");
    }
    // the page CRC stage (GEN with a codec: the CRC words to the callers' host
    // arrays) and the Seal (JFSX_CODEC_NONE with GEN, host: the words of its fused pass)
    if (!rc && st.page_mode && !st.plain) {
        rc = finish_aead(c, c->store_crc, c->store_ev[0], c->store_ev[1], true, st.pb.data());
        crc_done = true;
    }
    Workspace &w = c->store_aead;
    if (!rc && w.n && so.seal_pages && st.host) {
        const char *hw = w.h + w.crc_off;
        for (size_t k = 0; k < st.okidx.size(); k++) {
            jfsx_soblk &b = blks[st.okidx[k]];
            memcpy(b.crc, hw + 4 * so.seg_word[k], 4 * nseg_of(b.len));
        }
    }
    settle_stage(c, w, c->store_ev[2], c->store_ev[3], !rc && w.n);
    if (!(crc_done && !rc)) settle_stage(c, c->store_crc, c->store_ev[0], c->store_ev[1], false);
    if (c->rsa_h) memset(c->rsa_h, 0, std::min(c->rsa_hcap, so.msg_bytes));  // the pinned copy of the data keys
    if (!rc) {
        const SobjRes *hr = (const SobjRes *)(c->store_h + so.h_sres);
        std::vector<std::pair<char *, const char *>> cp;
        std::vector<size_t> cl;
        for (int i = 0; i < n; i++) {
            jfsx_soblk &b = blks[i];
            b.status = so.res[i].status;
            b.crc_bad_seg = so.res[i].bad_seg;
            b.crc_got = so.res[i].got;
            b.crc_expect = so.res[i].expect;
            b.out_len = b.img_len = 0;
            b.obj_crc = 0;
        }
        for (size_t k = 0; k < st.okidx.size(); k++) {
            const int i = st.okidx[k];
            jfsx_soblk &b = blks[i];
            b.status = hr[k].status;
            b.out_len = hr[k].out_len;
            b.img_len = hr[k].img_len;
            b.obj_crc = hr[k].obj_crc;
        }
        st.hs.copy_out();
    }
    if (rc) return rc;
    // jfsx_ctx_metrics: what the separate calls would have counted
    std::lock_guard<std::mutex> g(c->stat_mu);
    jfsx_metrics &mt = c->met;
    uint64_t &c_blocks = st.zstd ? mt.zstdc_blocks : mt.lz4c_blocks, &c_in = st.zstd ? mt.zstdc_in : mt.lz4c_in;
    uint64_t &c_out = st.zstd ? mt.zstdc_out : mt.lz4c_out;
    if (st.page_mode) mt.crc_batches++;
    if (!st.okidx.empty()) mt.seal_batches++;
    for (int i = 0; i < n; i++) {
        const jfsx_soblk &b = blks[i];
        if (st.page_mode) {
            mt.crc_ranges++;
            mt.crc_bytes += b.len;
            mt.crc_fail += b.status == JFSX_ECRC;
        }
        if (b.status != JFSX_OK) continue;
        if (!st.plain) {
            c_blocks++;
            c_in += b.len;
            c_out += b.img_len;
        }
        mt.seal_blocks++;
        mt.seal_bytes += b.img_len;
    }
    return 0;
}

}  // namespace

extern "C" uint64_t jfsx_object_bound(int codec, uint64_t len) {
    return object_bound(jfsx_rsa::kModBytes, codec, len);  // an RSA-2048 volume's
}
extern "C" uint64_t jfsx_object_bound_key(const jfsx_rsa_key *key, int codec, uint64_t len) {
    return key ? object_bound(key->kbytes, codec, len) : 0;
}

extern "C" int jfsx_store_objects(jfsx_ctx *c, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n,
                                  jfsx_soblk *blks, int crc_mode, int mem) {
    if (!c || (n > 0 && !blks)) return JFSX_EINVAL;
    // argument errors before the context, the key or the device is touched
    const int rc = check_sobj_args(key, e, algo, codec, n, blks, crc_mode, mem);
    if (rc || n == 0) return rc;
    if (key->device != c->device || check_sobj_caps(key, codec, n, blks)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_store_objects(c, key, e, algo, codec, n, blks, crc_mode, mem);
}

// ---------------------------------------------------------------------------
// Slice compaction (vfs.Compact, pkg/vfs/compact.go:54-109): jfsx_compact_plan
// (jfsx_compact.h, host only), jfsx_gather_batch (gather_pages_k,
// jfsx_gather.hip) and jfsx_compact_objects, which chains run_objects, the
// gather and run_store_objects on the context's stream: stored objects in,
// stored objects out, the pages in device memory only.
// ---------------------------------------------------------------------------
extern "C" int jfsx_compact_plan(uint32_t block_size, int n, const jfsx_slice *slices, int src_cap, jfsx_csrc *srcs,
                                 int *n_src, int page_cap, jfsx_cpage *pages, uint64_t *page_len, int *n_page,
                                 int piece_cap, jfsx_piece *pieces, int *n_piece) {
    if (!n_src || !n_page || !n_piece || src_cap < 0 || page_cap < 0 || piece_cap < 0) return JFSX_EINVAL;
    if ((src_cap && !srcs) || (page_cap && (!pages || !page_len)) || (piece_cap && !pieces)) return JFSX_EINVAL;
    jfsx_compact::Plan p;
    constexpr size_t kMax = 0x7FFFFFFF;
    try {
        const int rc = jfsx_compact::plan(block_size, n, slices, p);
        if (rc) return rc;
    } catch (const std::bad_alloc &) {
        return JFSX_ENOMEM;  // nothing is thrown across the C ABI
    } catch (const std::length_error &) {
        return JFSX_ENOMEM;
    }
    if (p.srcs.size() > kMax || p.pages.size() > kMax || p.pieces.size() > kMax) return JFSX_ENOMEM;
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

namespace {

struct GatherRun {
    uint32_t first, count;
};

// the piece rules of jfsx_gather_batch over n_src source lengths and n_dst
// destinations (their lengths and piece runs)
int check_pieces(int n_src, const uint64_t *slen, int n_dst, const uint64_t *dlen, const GatherRun *runs, int n_piece,
                 const jfsx_piece *pieces) {
    for (int k = 0; k < n_piece; k++) {
        const jfsx_piece &p = pieces[k];
        if (p.reserved || p.len == 0 || p.src < -1 || p.src >= n_src) return JFSX_EINVAL;
        if (p.src >= 0 && (p.src_off > slen[p.src] || p.len > slen[p.src] - p.src_off)) return JFSX_EINVAL;
    }
    for (int j = 0; j < n_dst; j++) {
        if ((uint64_t)runs[j].first + runs[j].count > (uint64_t)n_piece) return JFSX_EINVAL;
        uint64_t sum = 0;
        for (uint32_t k = 0; k < runs[j].count; k++) {
            const uint64_t l = pieces[runs[j].first + k].len;
            if (l > dlen[j] - sum) return JFSX_EINVAL;
            sum += l;
        }
        if (sum != dlen[j]) return JFSX_EINVAL;
    }
    return 0;
}

// One gather launch on c->stream over the destinations with dp[j] != nullptr
// and dlen[j] > 0; sp / dp are device addresses.  The pieces have passed
// check_pieces.  timed: the launch lies between the events of the synchronous
// paths (jfsx_ctx_set_timing).
int gather_enqueue(jfsx_ctx *c, const uint8_t *const *sp, int n_dst, uint8_t *const *dp, const uint64_t *dlen,
                   const GatherRun *runs, const jfsx_piece *pieces, bool timed, bool *launched = nullptr) {
    using jfsx_gather::GPage;
    using jfsx_gather::GPiece;
    std::vector<GPage> pg;
    std::vector<GPiece> pc;
    uint64_t tiles = 0;
    for (int j = 0; j < n_dst; j++) {
        if (!dp[j] || !dlen[j]) continue;
        GPage g{};
        g.dst = dp[j];
        g.len = dlen[j];
        g.tile_first = tiles;
        g.piece_first = (uint32_t)pc.size();
        g.piece_count = runs[j].count;
        uint64_t off = 0;
        for (uint32_t k = 0; k < runs[j].count; k++) {
            const jfsx_piece &p = pieces[runs[j].first + k];
            pc.push_back(GPiece{p.src < 0 ? nullptr : sp[p.src] + p.src_off, off, p.len});
            off += p.len;
        }
        tiles += jfsx_gather::tiles_of(dlen[j]);
        pg.push_back(g);
        if (pc.size() > 0xFFFFFFFFull) return JFSX_EINVAL;
    }
    if (pg.empty()) return 0;
    const size_t o_pc = align256(sizeof(GPage) * pg.size()), total = o_pc + sizeof(GPiece) * pc.size();
    int rc;
    if ((rc = ensure_host(&c->gat_h, &c->gat_hcap, total))) return rc;
    if ((rc = ensure_dev(c, &c->gat_d, &c->gat_dcap, total))) return rc;
    memcpy(c->gat_h, pg.data(), sizeof(GPage) * pg.size());
    memcpy(c->gat_h + o_pc, pc.data(), sizeof(GPiece) * pc.size());
    HIP_OK(hipMemcpyAsync(c->gat_d, c->gat_h, total, hipMemcpyHostToDevice, c->stream));
    if (timed) HIP_OK(hipEventRecord(c->ev_k0[0], c->stream));
    launch_begin();
    launch_gather(c->stream, c->ncu, (uint32_t)pg.size(), tiles, c->gat_d, c->gat_d + o_pc);
    HIP_OK(hipGetLastError());
    if (timed) HIP_OK(hipEventRecord(c->ev_k1[0], c->stream));
    if (launched) *launched = true;
    return 0;
}

// Under c->mu.  Host memory: gat_stage holds the sources and, behind them, the
// destinations; an empty buffer is not classified.
int run_gather(jfsx_ctx *c, int n_src, const jfsx_gsrc *src, int n_dst, const jfsx_gdst *dst, const uint64_t *dlen,
               const GatherRun *runs, const jfsx_piece *pieces, bool host) {
    hipStream_t s = c->stream;
    std::vector<const uint8_t *> sp(n_src, nullptr);
    std::vector<uint8_t *> dp(n_dst, nullptr);
    HostStage hs;
    std::vector<StageItem> up_items, down_items;
    size_t src_bytes = 0, dst_bytes = 0;
    int rc = 0;
    if (host) {
        for (int i = 0; i < n_src; i++) src_bytes += align256(src[i].len);
        for (int j = 0; j < n_dst; j++) dst_bytes += align256(dst[j].len);
        if ((rc = ensure_dev(c, &c->gat_stage, &c->gat_scap, src_bytes + dst_bytes))) return rc;
        hs.resize(n_src, n_dst);
        size_t off = 0;
        for (int i = 0; i < n_src; off += align256(src[i].len), i++) {
            sp[i] = (const uint8_t *)c->gat_stage + off;
            if (src[i].len) HostStage::mark(hs.in, i, src[i].data, src[i].len);
            up_items.push_back({(void *)src[i].data, c->gat_stage + off, off, src[i].len, (size_t)i});
        }
        off = 0;
        for (int j = 0; j < n_dst; off += align256(dst[j].len), j++) {
            dp[j] = (uint8_t *)c->gat_stage + src_bytes + off;
            if (dst[j].len) HostStage::mark(hs.out, j, dst[j].data, dst[j].len);
            down_items.push_back({dst[j].data, (char *)dp[j], off, dst[j].len, (size_t)j});
        }
        if ((rc = hs.reserve(c, src_bytes, dst_bytes))) return rc;
    } else {
        for (int i = 0; i < n_src; i++) sp[i] = (const uint8_t *)src[i].data;
        for (int j = 0; j < n_dst; j++) dp[j] = (uint8_t *)dst[j].data;
    }
    // what is enqueued; the stream is waited for below whatever happens, so a failure does not return at once
    const bool timed = c->timing;
    bool launched = false;
    const auto enqueue = [&]() {
        int r;
        if (host && (r = hs.upload(s, c->gat_stage, src_bytes, up_items))) return r;
        if ((r = gather_enqueue(c, sp.data(), n_dst, dp.data(), dlen, runs, pieces, timed, &launched))) return r;
        return host ? hs.download(s, c->gat_stage + src_bytes, dst_bytes, std::move(down_items)) : 0;
    };
    rc = wait_stream(c, enqueue(), "hipStreamSynchronize(gather)");
    if (!rc && timed && launched) add_elapsed_ms(c, c->ev_k0[0], c->ev_k1[0]);
    if (!rc) hs.copy_out();
    return rc;
}

}  // namespace

extern "C" int jfsx_gather_batch(jfsx_ctx *c, int n_src, const jfsx_gsrc *src, int n_dst, jfsx_gdst *dst, int n_piece,
                                 const jfsx_piece *pieces, int mem) {
    if (!c || n_src < 0 || n_dst < 0 || n_piece < 0) return JFSX_EINVAL;
    if ((n_src && !src) || (n_dst && !dst) || (n_piece && !pieces)) return JFSX_EINVAL;
    if (mem != JFSX_MEM_DEVICE && mem != JFSX_MEM_HOST) return JFSX_EINVAL;
    // argument errors before the context or its device is touched
    std::vector<uint64_t> slen(n_src), dlen(n_dst);
    std::vector<GatherRun> runs(n_dst);
    for (int i = 0; i < n_src; i++) {
        if (src[i].len && !src[i].data) return JFSX_EINVAL;
        slen[i] = src[i].len;
    }
    for (int j = 0; j < n_dst; j++) {
        if (dst[j].len && !dst[j].data) return JFSX_EINVAL;
        dlen[j] = dst[j].len;
        runs[j] = GatherRun{dst[j].piece_first, dst[j].piece_count};
    }
    int rc = check_pieces(n_src, slen.data(), n_dst, dlen.data(), runs.data(), n_piece, pieces);
    if (rc) return rc;
    if (mem == JFSX_MEM_DEVICE) {
        // 16-byte aligned, and no destination range overlaps a source's or another destination's
        struct Iv {
            uintptr_t lo, hi;
            bool dst;
        };
        std::vector<Iv> iv;
        for (int i = 0; i < n_src; i++) {
            if (!src[i].len) continue;
            if (!aligned16(src[i].data)) return JFSX_EINVAL;
            iv.push_back(Iv{(uintptr_t)src[i].data, (uintptr_t)src[i].data + src[i].len, false});
        }
        for (int j = 0; j < n_dst; j++) {
            if (!dst[j].len) continue;
            if (!aligned16(dst[j].data)) return JFSX_EINVAL;
            iv.push_back(Iv{(uintptr_t)dst[j].data, (uintptr_t)dst[j].data + dst[j].len, true});
        }
        std::sort(iv.begin(), iv.end(), [](const Iv &a, const Iv &b) { return a.lo < b.lo; });
        uintptr_t end_any = 0, end_dst = 0;
        for (const Iv &v : iv) {
            if (v.lo < (v.dst ? end_any : end_dst)) return JFSX_EINVAL;
            end_any = std::max(end_any, v.hi);
            if (v.dst) end_dst = std::max(end_dst, v.hi);
        }
    }
    if (n_dst == 0) return 0;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_gather(c, n_src, src, n_dst, dst, dlen.data(), runs.data(), pieces, mem == JFSX_MEM_HOST);
}

namespace {

// Under c->mu for the whole call; every argument has been checked.
int run_compact(jfsx_ctx *c, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n_src, jfsx_oblk *src,
                int src_crc_mode, int n_dst, jfsx_soblk *dst, jfsx_cpage *pages, int dst_crc_mode,
                const jfsx_piece *pieces) {
    hipStream_t s = c->stream;
    const bool gen = (dst_crc_mode & 3) == JFSX_CRC_GEN, ct_in = (src_crc_mode & JFSX_CRC_CT) != 0;
    // cmp_d: images | source pages | new pages | objects (each 1 mod 16) | page CRC words
    std::vector<size_t> ioff(n_src), soff(n_src), doff(n_dst), ooff(n_dst), coff(n_dst);
    size_t off = 0;
    for (int i = 0; i < n_src; i++) ioff[i] = off, off += align256(src[i].src_len);
    const size_t img_bytes = off;
    for (int i = 0; i < n_src; i++) soff[i] = off, off += align256(src[i].len);
    for (int j = 0; j < n_dst; j++) doff[j] = off, off += align256(dst[j].len);
    const size_t o_obj = off;
    for (int j = 0; j < n_dst; j++) ooff[j] = off - o_obj, off += align256(kObjLead + object_bound(key->kbytes, codec, dst[j].len));
    const size_t obj_bytes = off - o_obj, o_crc = off;
    for (int j = 0; j < n_dst; j++) coff[j] = off - o_crc, off += gen ? 4 * nseg_of(dst[j].len) : 0;
    const size_t crc_bytes = off - o_crc;
    int rc;
    if ((rc = ensure_dev(c, &c->cmp_d, &c->cmp_dcap, off))) return rc;
    char *d = c->cmp_d;
    // one pinned buffer: the images on their way up, then the objects and CRC words on their way down
    size_t bcap = 0;
    char *bounce = bounce_get(c, std::max(img_bytes, align256(obj_bytes) + crc_bytes), &bcap);
    if (!bounce) return JFSX_ENOMEM;
    struct BounceHold {  // back to the pool on every way out; each of them has waited for the stream
        jfsx_ctx *c;
        char *p;
        size_t cap;
        ~BounceHold() { bounce_put(c, p, cap); }
    } hold{c, bounce, bcap};
    // 1. load: images up, jfsx_load_objects' chain in its device-memory form, wait
    {
        std::vector<std::pair<char *, const char *>> cp;
        std::vector<size_t> cl;
        for (int i = 0; i < n_src; i++)
            if (src[i].src_len) {
                cp.push_back({bounce + ioff[i], (const char *)src[i].src});
                cl.push_back(src[i].src_len);
                c->bounce.bytes_in += src[i].src_len;
            }
        par_copy(cp, cl);
    }
    if (img_bytes) HIP_OK(hipMemcpyAsync(d, bounce, img_bytes, hipMemcpyHostToDevice, s));
    std::vector<jfsx_oblk> lo(src, src + n_src);
    for (int i = 0; i < n_src; i++) {
        lo[i].src = src[i].src_len ? d + ioff[i] : nullptr;
        lo[i].dst = src[i].len ? d + soff[i] : nullptr;
        lo[i].crc = nullptr;
    }
    // an all-hole chunk has no source: its pages are zeros from the gather alone
    if (n_src && (rc = run_objects(c, key, algo, codec, n_src, lo.data(), src_crc_mode, JFSX_MEM_DEVICE))) return rc;
    for (int i = 0; i < n_src; i++) {
        src[i].status = lo[i].status;
        src[i].out_len = lo[i].out_len;
        src[i].codec_info = lo[i].codec_info;
        src[i].key_len = lo[i].key_len;
        if (ct_in) src[i].obj_crc = lo[i].obj_crc;
    }
    // 2. gate: a page is good when every source its pieces name is
    std::vector<int> good;
    for (int j = 0; j < n_dst; j++) {
        int32_t bad = -1;
        for (uint32_t k = 0; k < pages[j].piece_count && bad < 0; k++) {
            const int32_t sidx = pieces[pages[j].piece_first + k].src;
            if (sidx >= 0 && (src[sidx].status != JFSX_OK || src[sidx].out_len != src[sidx].len)) bad = sidx;
        }
        pages[j].src_bad = bad;
        jfsx_soblk &b = dst[j];
        b.status = bad < 0 ? JFSX_OK : JFSX_ESRC;
        b.out_len = b.img_len = 0;
        b.obj_crc = 0;
        b.crc_bad_seg = -1;
        b.crc_got = b.crc_expect = 0;
        if (bad < 0) good.push_back(j);
    }
    const int m = (int)good.size();
    if (!m) return 0;
    // 3. gather: one launch over the good pages
    std::vector<const uint8_t *> sp(n_src);
    std::vector<uint8_t *> dp(n_dst, nullptr);
    std::vector<uint64_t> dlen(n_dst);
    std::vector<GatherRun> runs(n_dst);
    for (int i = 0; i < n_src; i++) sp[i] = (const uint8_t *)d + soff[i];
    for (int j = 0; j < n_dst; j++) {
        dlen[j] = dst[j].len;
        runs[j] = GatherRun{pages[j].piece_first, pages[j].piece_count};
    }
    for (int j : good) dp[j] = (uint8_t *)d + doff[j];
    if ((rc = gather_enqueue(c, sp.data(), n_dst, dp.data(), dlen.data(), runs.data(), pieces, false))) {
        (void)hipStreamSynchronize(s);
        return rc;
    }
    // 4. store: jfsx_store_objects' chain in its device-memory form over the
    // good pages; the objects and CRC words come down behind its phase B
    std::vector<jfsx_soblk> so(m);
    for (int k = 0; k < m; k++) {
        const int j = good[k];
        so[k] = dst[j];
        so[k].src = dst[j].len ? d + doff[j] : nullptr;
        so[k].obj = d + o_obj + ooff[j] + kObjLead;
        so[k].obj_cap = object_bound(key->kbytes, codec, dst[j].len);
        so[k].crc = gen ? (uint8_t *)(d + o_crc + coff[j]) : nullptr;
    }
    const SobjTail tail = [&](const SobjState &ss) {
        for (int k : ss.st.okidx) {
            const size_t at = ooff[good[k]] + kObjLead;
            HIP_OK(hipMemcpyAsync(bounce + at, d + o_obj + at, obj_frame(key->kbytes) + ss.res[k].out_len,
                                  hipMemcpyDeviceToHost, s));
        }
        if (crc_bytes)
            HIP_OK(hipMemcpyAsync(bounce + align256(obj_bytes), d + o_crc, crc_bytes, hipMemcpyDeviceToHost, s));
        return 0;
    };
    if ((rc = run_store_objects(c, key, e, algo, codec, m, so.data(), dst_crc_mode, JFSX_MEM_DEVICE, &tail)))
        return rc;
    std::vector<std::pair<char *, const char *>> cp;
    std::vector<size_t> cl;
    for (int k = 0; k < m; k++) {
        const int j = good[k];
        jfsx_soblk &b = dst[j];
        b.status = so[k].status;
        b.out_len = so[k].out_len;
        b.img_len = so[k].img_len;
        b.obj_crc = so[k].obj_crc;
        b.crc_bad_seg = so[k].crc_bad_seg;
        b.crc_got = so[k].crc_got;
        b.crc_expect = so[k].crc_expect;
        if (b.status != JFSX_OK) continue;
        cp.push_back({(char *)b.obj, bounce + ooff[j] + kObjLead});
        cl.push_back(b.out_len);
        c->bounce.bytes_out += b.out_len;
        if (gen) memcpy(b.crc, bounce + align256(obj_bytes) + coff[j], 4 * nseg_of(b.len));
    }
    par_copy(cp, cl);
    return 0;
}

}  // namespace

extern "C" int jfsx_compact_objects(jfsx_ctx *c, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n_src,
                                    jfsx_oblk *src, int src_crc_mode, int n_dst, jfsx_soblk *dst, jfsx_cpage *pages,
                                    int dst_crc_mode, int n_piece, const jfsx_piece *pieces) {
    if (!c || n_src < 0 || n_dst < 0 || n_piece < 0) return JFSX_EINVAL;
    if ((n_src && !src) || (n_dst && (!dst || !pages)) || (n_piece && !pieces)) return JFSX_EINVAL;
    // argument errors before the context, the key or the device is touched:
    // the two calls' rules for host memory on copies that carry a page address
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;
    if (src_crc_mode & ~JFSX_CRC_CT) return JFSX_EINVAL;
    if (dst_crc_mode < 0 || (dst_crc_mode & 3) == JFSX_CRC_VERIFY) return JFSX_EINVAL;
    static const uint8_t page_stub[16] = {};
    std::vector<jfsx_oblk> lo(src, src + n_src);
    std::vector<uint64_t> slen(n_src), dlen(n_dst);
    for (int i = 0; i < n_src; i++) {
        if (src[i].dst || src[i].crc) return JFSX_EINVAL;  // the page stays on the device
        lo[i].dst = (void *)page_stub;
        slen[i] = src[i].len;
    }
    int rc = check_objects_args(key, algo, codec, n_src, lo.data(), src_crc_mode, JFSX_MEM_HOST);
    if (rc) return rc;
    std::vector<jfsx_soblk> so(dst, dst + n_dst);
    std::vector<GatherRun> runs(n_dst);
    for (int j = 0; j < n_dst; j++) {
        if (dst[j].src || pages[j].reserved) return JFSX_EINVAL;  // the page is assembled
        so[j].src = page_stub;
        dlen[j] = dst[j].len;
        runs[j] = GatherRun{pages[j].piece_first, pages[j].piece_count};
    }
    if ((rc = check_sobj_args(key, e, algo, codec, n_dst, so.data(), dst_crc_mode, JFSX_MEM_HOST))) return rc;
    if ((rc = check_pieces(n_src, slen.data(), n_dst, dlen.data(), runs.data(), n_piece, pieces))) return rc;
    if (n_dst == 0) return 0;
    if (key->device != c->device || check_sobj_caps(key, codec, n_dst, dst)) return JFSX_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    CtxScope es_(c);
    HIP_OK(hipSetDevice(c->device));
    return run_compact(c, key, e, algo, codec, n_src, src, src_crc_mode, n_dst, dst, pages, dst_crc_mode, pieces);
}

// ---------------------------------------------------------------------------
// Ranged Open: jfsx_open_range_batch, jfsx_data_decrypt_range
// ---------------------------------------------------------------------------
namespace {

// Go's slice rule (encrypt.go:246-253) and the window widened to whole
// segments: [w0, w1) is empty when n == 0
struct RangeWin {
    uint64_t o, n, w0, w1;
};
RangeWin range_window(uint64_t len, uint64_t off, int64_t limit) {
    RangeWin r;
    r.o = std::min(off, len);
    r.n = (limit == -1 || (uint64_t)limit > len - r.o) ? len - r.o : (uint64_t)limit;
    r.w0 = r.w1 = 0;
    if (r.n) {
        r.w0 = r.o / kSeg * kSeg;
        r.w1 = std::min(len, (r.o + r.n + kSeg - 1) / kSeg * kSeg);
    }
    return r;
}

// The task lists of a ranged batch.  The widened windows go to the main
// kernel as ordinary Open tasks, cut by plan_batch as a batch of blocks of the
// windows' lengths would be; every other segment goes to the auth kernel in
// tasks of auth_bytes.  A block's slots are contiguous: its main tasks' first,
// then its auth tasks'.
//   auth_bytes: a power of two of segments, the largest up to the kernel's
//   maximum that still leaves `want` tasks in the batch, else its minimum
//     GCM     64 KiB .. 1 MiB, 512 tasks (one 16-wave workgroup per CU: 4 to 64
//             rows per wave, and the task's GHASH table built once per task)
//     ChaCha  32 KiB .. 1 MiB, 2048 tasks (eight 4-wave workgroups per CU: 2 to
//             64 rows per wave)
struct RangePlan {
    std::vector<RangeWin> win;
    std::vector<Task> main, auth;  // plan order: block by block, c0 ascending
    std::vector<uint32_t> slot0, nslots, n_main, n_auth;  // per block
    uint64_t total_slots = 0, main_bytes = 0, auth_bytes = 0;
    uint32_t max_slots = 0;
};
constexpr uint64_t kGcmAuthMin = 2 * (uint64_t)kSeg, kGcmAuthMax = (uint64_t)1 << 20, kGcmAuthWant = 512;
constexpr uint64_t kCpAuthMin = (uint64_t)kSeg, kCpAuthMax = (uint64_t)1 << 20, kCpAuthWant = 2048;

RangePlan plan_range(bool gcm, int n, const uint64_t *lens, const uint64_t *offs, const int64_t *limits) {
    RangePlan p;
    p.win.resize(n);
    p.slot0.assign(n, 0);
    p.nslots.assign(n, 0);
    p.n_main.assign(n, 0);
    p.n_auth.assign(n, 0);
    std::vector<uint64_t> wl(n);
    uint64_t outside = 0;
    for (int i = 0; i < n; i++) {
        p.win[i] = range_window(lens[i], offs[i], limits[i]);
        wl[i] = p.win[i].w1 - p.win[i].w0;
        outside += lens[i] - wl[i];
    }
    const Plan mp = plan_batch(gcm ? kPlanGcm : kPlanCp, wl);
    p.main_bytes = mp.task_bytes;
    const uint64_t amin = gcm ? kGcmAuthMin : kCpAuthMin, amax = gcm ? kGcmAuthMax : kCpAuthMax;
    const uint64_t want = gcm ? kGcmAuthWant : kCpAuthWant;
    uint64_t ab = amax;
    while (ab > amin && outside / ab < want) ab >>= 1;
    p.auth_bytes = ab;
    const uint32_t mslots = gcm ? kSlotsPerTask : kCpWaves, aslots = gcm ? kGcmAuthWaves : kCpAuthWaves;
    size_t mt = 0;
    for (int i = 0; i < n; i++) {
        const RangeWin &w = p.win[i];
        p.slot0[i] = (uint32_t)p.total_slots;
        for (; mt < mp.tasks.size() && mp.tasks[mt].blk == (uint32_t)i; mt++) {
            Task t = mp.tasks[mt];
            t.c0 += w.w0;
            t.c1 += w.w0;
            t.slot0 = (uint32_t)p.total_slots;
            p.main.push_back(t);
            p.total_slots += mslots;
            p.n_main[i]++;
        }
        const uint64_t runs[2][2] = {{0, w.w0}, {w.w1, lens[i]}};
        for (const auto &r : runs)
            for (uint64_t c0 = r[0]; c0 < r[1]; c0 += ab) {
                p.auth.push_back(Task{(uint32_t)i, (uint32_t)p.total_slots, c0, std::min(c0 + ab, r[1])});
                p.total_slots += aslots;
                p.n_auth[i]++;
            }
        p.nslots[i] = (uint32_t)(p.total_slots - p.slot0[i]);
        p.max_slots = std::max(p.max_slots, p.nslots[i]);
    }
    return p;
}

bool range_mode_ok(int crc_mode) { return crc_mode == JFSX_CRC_NONE || crc_mode == (JFSX_CRC_GEN | JFSX_CRC_CT); }

// the argument rules of jfsx_open_range_batch; touches neither context nor records
int check_range_args(int algo, int n, const jfsx_rblk *blks, int crc_mode, int mem) {
    if (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305) return JFSX_EINVAL;
    if (!range_mode_ok(crc_mode) || n < 0 || (n > 0 && !blks)) return JFSX_EINVAL;
    if (mem != JFSX_MEM_HOST && mem != JFSX_MEM_DEVICE) return JFSX_EINVAL;
    const bool device = mem == JFSX_MEM_DEVICE;
    for (int i = 0; i < n; i++) {
        const jfsx_rblk &b = blks[i];
        if (b.reserved || b.reserved2 || b.limit < -1) return JFSX_EINVAL;
        if (b.len > (algo == JFSX_AES256GCM ? kGcmMaxLen : kCpMaxLen)) return JFSX_EINVAL;
        const RangeWin w = range_window(b.len, b.off, b.limit);
        if (b.dst_cap < w.n || (w.n && !b.dst) || (b.len && !b.src) || (crc_mode && !b.crc)) return JFSX_EINVAL;
        if (!device) continue;
        if ((b.len && !aligned16(b.src)) || (w.n && !aligned16(b.dst)) || (crc_mode && !aligned16(b.crc)))
            return JFSX_EINVAL;
        if (w.n && b.len) {
            const uintptr_t s0 = (uintptr_t)b.src, d0 = (uintptr_t)b.dst;
            if (d0 < s0 + b.len && s0 < d0 + b.dst_cap) return JFSX_EINVAL;
        }
    }
    return 0;
}

// Under c->mu; every argument has been checked.  One synchronous chain on
// c->stream in the buffers of the synchronous paths (ws[0], its staging, the
// gather's descriptors):
//   host: C up once (pageable blocks through the context's pinned staging)
//   keysetup | [CT pass] | auth kernel | main kernel into the staging | finalize
//   BlkOut (and the CRC words of a host call) down, wait
//   the windows of the blocks that verified gathered out of the staging:
//     device: into dst (gather_pages_k writes nothing outside [dst, dst + n))
//     host:   packed, one copy down of exactly their bytes, wait, into dst
//   a failed block's dst[0, n) zeroed
int run_open_range(jfsx_ctx *c, int algo, int n, jfsx_rblk *blks, int crc_mode, bool host) {
    const bool gcm = algo == JFSX_AES256GCM;
    hipStream_t s = c->stream;
    Workspace &w = c->ws[0];
    std::vector<uint64_t> lens(n), offs(n);
    std::vector<int64_t> lims(n);
    for (int i = 0; i < n; i++) lens[i] = blks[i].len, offs[i] = blks[i].off, lims[i] = blks[i].limit;
    const RangePlan rp = plan_range(gcm, n, lens.data(), offs.data(), lims.data());
    Plan cplan;
    if (crc_mode) cplan = plan_batch(kPlanCrc, lens);
    const size_t nmt = rp.main.size(), nat = rp.auth.size(), nct = cplan.tasks.size();
    // staging: [C of a host call] [the widened windows] [the packed windows of a host call]
    std::vector<size_t> soff(n), woff(n), poff(n);
    size_t src_bytes = 0, win_bytes = 0, out_bytes = 0;
    uint64_t crc_words = 0;
    for (int i = 0; i < n; i++) {
        soff[i] = src_bytes;
        if (host) src_bytes += align256(lens[i]);
        woff[i] = win_bytes;
        win_bytes += align256(rp.win[i].w1 - rp.win[i].w0);
        poff[i] = out_bytes;
        if (host) out_bytes += align256(rp.win[i].n);
        crc_words += nseg_of(lens[i]);
    }
    int rc;
    if ((rc = ensure_dev(c, &w.stage, &w.scap, src_bytes + win_bytes + out_bytes))) return rc;
    char *const st_src = w.stage, *const st_win = w.stage + src_bytes, *const st_out = st_win + win_bytes;
    // descriptors
    size_t off = 0;
    const size_t o_keys = off; off = align256(off + sizeof(KeyIn) * n);
    const size_t o_blk = off; off = align256(off + sizeof(BlkDev) * n);
    const size_t o_mtask = off; off = align256(off + sizeof(Task) * std::max<size_t>(nmt, 1));
    const size_t o_atask = off; off = align256(off + sizeof(Task) * std::max<size_t>(nat, 1));
    const size_t o_tagin = off; off = align256(off + 16 * (size_t)n);
    const size_t o_queue = off; off = align256(off + 4);
    const size_t o_cblk = off; if (crc_mode) off = align256(off + sizeof(BlkDev) * n);
    const size_t o_ctask = off; if (crc_mode) off = align256(off + sizeof(Task) * std::max<size_t>(nct, 1));
    const size_t h_bytes = off;
    const size_t o_out = off; off = align256(off + sizeof(BlkOut) * n);
    const size_t o_crcout = off; if (crc_mode && host) off = align256(off + 4 * crc_words);
    const size_t down = crc_mode && host ? o_crcout + 4 * crc_words - o_out : sizeof(BlkOut) * n;
    const size_t o_sched = off; off = align256(off + (gcm ? sizeof(GcmSched) : sizeof(CpSched)) * n);
    const size_t o_part = off; off = align256(off + 32 * std::max<uint64_t>(rp.total_slots, 1));
    const size_t o_pexp = off; off = align256(off + 4 * std::max<uint64_t>(rp.total_slots, 1));
    if ((rc = ensure_dev(c, &w.d, &w.dcap, off))) return rc;
    if ((rc = ensure_host(&w.h, &w.hcap, std::max(h_bytes, down)))) return rc;
    char *h = w.h, *d = w.d;
    KeyIn *hk = (KeyIn *)(h + o_keys);
    BlkDev *hb = (BlkDev *)(h + o_blk);
    *(uint32_t *)(h + o_queue) = 0;
    uint64_t cw = 0;
    for (int i = 0; i < n; i++) {
        const jfsx_rblk &b = blks[i];
        memcpy(hk[i].key, b.key, 32);
        memcpy(hk[i].nonce, b.nonce, 12);
        hk[i].pad = 0;
        memset(&hb[i], 0, sizeof(BlkDev));
        hb[i].src = host ? (const uint8_t *)st_src + soff[i] : (const uint8_t *)b.src;
        // the main kernel writes plaintext byte k of the block at dst + k: the
        // window's first segment lands at the start of the block's staging
        hb[i].dst = (uint8_t *)((uintptr_t)(st_win + woff[i]) - (uintptr_t)rp.win[i].w0);
        hb[i].len = b.len;
        hb[i].slot0 = rp.slot0[i];
        hb[i].nslots = rp.nslots[i];
        hb[i].tag_in = (const uint8_t *)(d + o_tagin + 16 * (size_t)i);
        memcpy(h + o_tagin + 16 * (size_t)i, b.tag, 16);
        if (crc_mode) {
            BlkDev &cb = ((BlkDev *)(h + o_cblk))[i];
            memset(&cb, 0, sizeof(cb));
            cb.src = hb[i].src;
            cb.len = b.len;
            cb.crc = host ? (uint8_t *)(d + o_crcout + 4 * cw) : b.crc;
        }
        cw += nseg_of(b.len);
    }
    if (nmt) {
        memcpy(h + o_mtask, rp.main.data(), sizeof(Task) * nmt);
        order_largest_first((Task *)(h + o_mtask), nmt, (size_t)(gcm ? kMaxTaskBytes : kCpTaskBytes) >> 12);
    }
    if (nat) {
        memcpy(h + o_atask, rp.auth.data(), sizeof(Task) * nat);
        order_largest_first((Task *)(h + o_atask), nat, (size_t)rp.auth_bytes >> 12);
    }
    cplan.dispatch((Task *)(h + o_ctask));

    // host: the blocks' C into the staging
    // through rng_h, not the pool; every window comes down through it (below)
    char *bounce = nullptr;
    HostStage hs;
    std::vector<StageItem> up_items;
    if (host) {
        hs.resize(n, 0);
        for (int i = 0; i < n; i++) {
            if (lens[i]) HostStage::mark(hs.in, i, blks[i].src, lens[i]);
            up_items.push_back({(void *)blks[i].src, st_src + soff[i], soff[i], (size_t)lens[i], (size_t)i});
        }
        const size_t need = std::max(hs.need(src_bytes, 0), out_bytes);
        if (need && (rc = ensure_host(&c->rng_h, &c->rng_hcap, need))) return rc;
        hs.lend(bounce = c->rng_h);
    }
    const BlkDev *db = (const BlkDev *)(d + o_blk);
    uint32_t *dpart = (uint32_t *)(d + o_part), *dpexp = (uint32_t *)(d + o_pexp);
    const bool timed = c->timing && (nmt || nat);
    const auto chain = [&]() {
        if (host) {
            const int r = hs.upload(s, st_src, src_bytes, up_items);
            if (r) return r;
        }
        HIP_OK(hipMemcpyAsync(d, h, h_bytes, hipMemcpyHostToDevice, s));
        launch_begin();
        if (gcm) launch_gcm_keysetup(s, n, (const KeyIn *)(d + o_keys), db, (GcmSched *)(d + o_sched), c->tabs, c->bitslice);
        else launch_cp_keysetup(s, n, (const KeyIn *)(d + o_keys), db, (CpSched *)(d + o_sched));
        if (crc_mode) {
            for (int i = 0; i < n; i++)  // checksum() of nothing: one zero word
                if (lens[i] == 0) HIP_OK(hipMemsetAsync(((const BlkDev *)(h + o_cblk))[i].crc, 0, 4, s));
            launch_crc_segments(s, (int)nct, (const Task *)(d + o_ctask), (const BlkDev *)(d + o_cblk), c->tabs);
        }
        if (timed) HIP_OK(hipEventRecord(c->ev_k0[0], s));
        if (gcm) {
            launch_gcm_auth(s, (int)nat, (const Task *)(d + o_atask), db, (const GcmSched *)(d + o_sched), dpart, dpexp);
            launch_gcm_main(s, (int)nmt, c->ncu, (uint32_t *)(d + o_queue), true, JFSX_CRC_NONE, c->bitslice,
                            (const Task *)(d + o_mtask), db, (const GcmSched *)(d + o_sched), dpart, dpexp, c->tabs,
                            c->crc_l1);
        } else {
            launch_cp_auth(s, (int)nat, (const Task *)(d + o_atask), db, (const CpSched *)(d + o_sched), dpart, dpexp);
            launch_cp_main(s, (int)nmt, c->ncu, (uint32_t *)(d + o_queue), true, JFSX_CRC_NONE,
                           (const Task *)(d + o_mtask), db, (const CpSched *)(d + o_sched), dpart, dpexp, c->tabs);
        }
        if (timed) HIP_OK(hipEventRecord(c->ev_k1[0], s));
        if (gcm)
            launch_gcm_finalize(s, n, true, JFSX_CRC_NONE, db, (const GcmSched *)(d + o_sched), dpart, dpexp,
                                (BlkOut *)(d + o_out), rp.max_slots);
        else
            launch_cp_finalize(s, n, true, JFSX_CRC_NONE, db, (const CpSched *)(d + o_sched), dpart, dpexp,
                               (BlkOut *)(d + o_out));
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(h, d + o_out, down, hipMemcpyDeviceToHost, s));
        return 0;
    };
    rc = wait_stream(c, chain(), "hipStreamSynchronize(open_range)");
    if (rc) return rc;
    if (timed) add_elapsed_ms(c, c->ev_k0[0], c->ev_k1[0]);
    // the windows of the blocks that verified, out of the staging
    const BlkOut *ho = (const BlkOut *)h;
    std::vector<const uint8_t *> sp(n, nullptr);
    std::vector<uint8_t *> dp(n, nullptr);
    std::vector<uint64_t> dlen(n, 0);
    std::vector<GatherRun> runs(n);
    std::vector<jfsx_piece> pieces(n);
    for (int i = 0; i < n; i++) {
        const RangeWin &rw = rp.win[i];
        runs[i] = GatherRun{(uint32_t)i, 1};
        pieces[i] = jfsx_piece{i, 0, 0, rw.n};
        if (ho[i].status != JFSX_OK || !rw.n) continue;
        sp[i] = (const uint8_t *)st_win + woff[i] + (rw.o - rw.w0);
        dp[i] = host ? (uint8_t *)st_out + poff[i] : (uint8_t *)blks[i].dst;
        dlen[i] = rw.n;
    }
    const auto place = [&]() {
        const int r = gather_enqueue(c, sp.data(), n, dp.data(), dlen.data(), runs.data(), pieces.data(), false);
        if (r) return r;
        if (host) {
            // exactly the windows' bytes: runs of verified blocks that lie back to back in the packed buffer
            for (int i = 0; i < n;) {
                if (!dlen[i]) {
                    i++;
                    continue;
                }
                int j = i;
                while (j + 1 < n && dlen[j + 1] && poff[j] + dlen[j] == poff[j + 1]) j++;
                const size_t bytes = poff[j] + dlen[j] - poff[i];
                HIP_OK(hipMemcpyAsync(bounce + poff[i], st_out + poff[i], bytes, hipMemcpyDeviceToHost, s));
                i = j + 1;
            }
        } else {
            for (int i = 0; i < n; i++)
                if (ho[i].status != JFSX_OK && rp.win[i].n) HIP_OK(hipMemsetAsync(blks[i].dst, 0, rp.win[i].n, s));
        }
        return 0;
    };
    rc = wait_stream(c, place(), "hipStreamSynchronize(open_range windows)");
    if (!rc) {
        if (host) {
            std::vector<std::pair<char *, const char *>> cp;
            std::vector<size_t> cl;
            for (int i = 0; i < n; i++) {
                if (dlen[i]) {
                    cp.push_back({(char *)blks[i].dst, bounce + poff[i]});
                    cl.push_back(dlen[i]);
                } else if (rp.win[i].n) {
                    memset(blks[i].dst, 0, rp.win[i].n);
                }
            }
            par_copy(cp, cl);
            if (crc_mode) {
                const char *hw = h + (o_crcout - o_out);
                for (int i = 0; i < n; i++) {
                    memcpy(blks[i].crc, hw, 4 * nseg_of(lens[i]));
                    hw += 4 * nseg_of(lens[i]);
                }
            }
        }
        for (int i = 0; i < n; i++) {
            blks[i].status = ho[i].status;
            blks[i].out_len = ho[i].status == JFSX_OK ? rp.win[i].n : 0;
        }
    }
    return rc;
}

}  // namespace

extern "C" int jfsx_open_range_batch(jfsx_ctx *c, int algo, int n, jfsx_rblk *blks, int crc_mode, int mem) {
    if (!c) return JFSX_EINVAL;
    int rc = check_range_args(algo, n, blks, crc_mode, mem);
    if (rc || n == 0) return rc;
    {
        std::lock_guard<std::mutex> g(c->mu);
        CtxScope es_(c);
        HIP_OK(hipSetDevice(c->device));
        rc = run_open_range(c, algo, n, blks, crc_mode, mem == JFSX_MEM_HOST);
    }
    if (rc == 0) {
        std::lock_guard<std::mutex> g(c->stat_mu);
        jfsx_metrics &m = c->met;
        m.open_batches++;
        m.open_blocks += n;
        for (int i = 0; i < n; i++) {
            m.open_bytes += blks[i].len;
            m.open_fail += blks[i].status != JFSX_OK;
        }
    }
    return rc;
}

namespace {
using RangeFn = std::function<int(jfsx_rblk *, int crc_mode)>;

// data_decrypt with the window
int data_decrypt_range(const RangeFn &open, const uint8_t key[32], const void *obj, uint64_t olen, uint64_t off,
                       int64_t limit, void *out, uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc,
                       uint32_t *got_crc) {
    if (!key || !obj || limit < -1) return JFSX_EINVAL;
    int kl = 0, nl = 0;
    int rc = jfsx_parse_header(obj, olen, &kl, &nl);
    if (rc) return rc;
    const uint8_t *o = (const uint8_t *)obj;
    if (expect_crc && !got_crc) return JFSX_EINVAL;
    if (nl != 12) return JFSX_ETAG;
    const uint64_t hdr = 3 + (uint64_t)kl + nl;
    if (olen - hdr < 16) return JFSX_ETAG;
    const uint64_t len = olen - hdr - 16;
    const RangeWin w = range_window(len, off, limit);
    if (out_cap < w.n || (w.n && !out)) return JFSX_EINVAL;
    jfsx_rblk b;
    memset(&b, 0, sizeof(b));
    memcpy(b.key, key, 32);
    memcpy(b.nonce, o + 3 + kl, 12);
    memcpy(b.tag, o + hdr + len, 16);
    b.src = o + hdr;
    b.len = len;
    b.off = off;
    b.limit = limit;
    b.dst = out;
    b.dst_cap = out_cap;
    std::vector<uint8_t> segs;
    int mode = JFSX_CRC_NONE;
    if (expect_crc) {
        segs.resize(4 * nseg_of(len));
        b.crc = segs.data();
        mode = JFSX_CRC_GEN | JFSX_CRC_CT;
    }
    if ((rc = open(&b, mode))) return rc;
    if (expect_crc) {
        if ((rc = jfsx_object_crc32c(o, hdr, segs.data(), len, o + hdr + len, got_crc))) return rc;
        if (*got_crc != *expect_crc) {
            if (w.n) memset(out, 0, w.n);
            return JFSX_ECRC;
        }
    }
    if (b.status == JFSX_ETAG) return JFSX_ETAG;
    if (out_len) *out_len = w.n;
    return 0;
}
}  // namespace

extern "C" int jfsx_data_decrypt_range(jfsx_ctx *c, int algo, const uint8_t key[32], const void *obj, uint64_t olen,
                                       uint64_t off, int64_t limit, void *out, uint64_t out_cap, uint64_t *out_len,
                                       const uint32_t *expect_crc, uint32_t *got_crc) {
    if (!c || (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305)) return JFSX_EINVAL;
    return data_decrypt_range([&](jfsx_rblk *b, int m) { return jfsx_open_range_batch(c, algo, 1, b, m, JFSX_MEM_HOST); },
                              key, obj, olen, off, limit, out, out_cap, out_len, expect_crc, got_crc);
}

// Host-only view of plan_range (no device, no context), for tests; not part of
// the ABI (undeclared in jfsx.h).  kind 0 GCM, 1 ChaCha20-Poly1305.  blocks
// (nullable): n x 8 words o, n, w0, w1, slot0, nslots, main tasks, auth tasks;
// sizes (nullable): the main planner's task bytes, the auth planner's, the
// main and auth slots per task; tasks (nullable): up to cap x 5 words blk,
// kernel (0 main, 1 auth), c0, c1, slot0 in plan order, *ntasks their number.
extern "C" int jfsx_debug_range_plan(int kind, int n, const uint64_t *lens, const uint64_t *offs, const int64_t *limits,
                                     uint64_t *blocks, uint64_t *sizes, uint64_t *tasks, uint64_t cap,
                                     uint64_t *ntasks) {
    if (kind < kPlanGcm || kind > kPlanCp || n < 0 || (n && (!lens || !offs || !limits))) return JFSX_EINVAL;
    for (int i = 0; i < n; i++)
        if (lens[i] > (kind == kPlanGcm ? kGcmMaxLen : kCpMaxLen) || limits[i] < -1) return JFSX_EINVAL;
    const bool gcm = kind == kPlanGcm;
    const RangePlan p = plan_range(gcm, n, lens, offs, limits);
    for (int i = 0; blocks && i < n; i++) {
        const uint64_t v[8] = {p.win[i].o, p.win[i].n, p.win[i].w0, p.win[i].w1,
                               p.slot0[i], p.nslots[i], p.n_main[i], p.n_auth[i]};
        memcpy(blocks + 8 * i, v, sizeof(v));
    }
    if (sizes) {
        sizes[0] = p.main_bytes;
        sizes[1] = p.auth_bytes;
        sizes[2] = gcm ? kSlotsPerTask : kCpWaves;
        sizes[3] = gcm ? kGcmAuthWaves : kCpAuthWaves;
    }
    if (ntasks) *ntasks = p.main.size() + p.auth.size();
    if (tasks && cap) {
        // plan order: block by block, a block's main tasks, then its auth tasks
        size_t k = 0, mi = 0, ai = 0;
        for (int i = 0; i < n && k < cap; i++) {
            for (; mi < p.main.size() && p.main[mi].blk == (uint32_t)i; mi++) {
                if (k >= cap) break;
                const uint64_t v[5] = {(uint64_t)i, 0, p.main[mi].c0, p.main[mi].c1, p.main[mi].slot0};
                memcpy(tasks + 5 * k++, v, sizeof(v));
            }
            for (; ai < p.auth.size() && p.auth[ai].blk == (uint32_t)i; ai++) {
                if (k >= cap) break;
                const uint64_t v[5] = {(uint64_t)i, 1, p.auth[ai].c0, p.auth[ai].c1, p.auth[ai].slot0};
                memcpy(tasks + 5 * k++, v, sizeof(v));
            }
        }
    }
    return 0;
}

// The aggregator's ranged Open: one more op, defined here because its batch
// call is (jfsx_agg.cpp's agg_submit_ext).  The engine stages a host request's
// pageable memory itself (run_open_range), so the caller's record goes in as
// it is.
namespace jfsx {
typedef int (*AggBatchFn)(jfsx_ctx *c, int algo, int n, void *items, int mode, int mem);
int agg_submit_ext(jfsx_agg *a, AggBatchFn fn, int algo, int mode, int mem, void *item, size_t item_size,
                   uint64_t bytes);
}  // namespace jfsx

extern "C" int jfsx_agg_open_range(jfsx_agg *a, int algo, jfsx_rblk *blk, int crc_mode, int mem) {
    if (!a || !blk || (algo != JFSX_AES256GCM && algo != JFSX_CHACHA20P1305)) return JFSX_EINVAL;
    return jfsx::agg_submit_ext(
        a,
        [](jfsx_ctx *c, int al, int n, void *items, int mode, int m) {
            return jfsx_open_range_batch(c, al, n, (jfsx_rblk *)items, mode, m);
        },
        algo, crc_mode, mem, blk, sizeof(jfsx_rblk), blk->len);
}
