/*
 * jfsx.h -- C-ABI of libjfsx.so, the MI355X block-transform engine for the
 * JuiceFS per-block data path (AEAD Seal/Open fused with CRC32C segment
 * checksums).  Plain C types only: this is the surface a cgo shim binds
 * (see INTEGRATION.md for the Go side).
 *
 * Reference interfaces each entry point replaces (JuiceFS 1.2.0,
 * /root/reference):
 *
 *   jfsx_seal_batch      dataEncryptor.Encrypt's aead.Seal          pkg/object/encrypt.go:164-194 (Seal at :192)
 *                        + checksum() on the same plaintext         pkg/chunk/disk_cache.go:1218-1231 (called :469)
 *   jfsx_open_batch      dataEncryptor.Decrypt's aead.Open          pkg/object/encrypt.go:196-216 (Open at :215)
 *                        + checksum()/verify of the plaintext       pkg/chunk/disk_cache.go:1219, :1315-1327
 *   jfsx_data_encrypt    dataEncryptor.Encrypt (object format)      pkg/object/encrypt.go:164-194
 *   jfsx_data_decrypt    dataEncryptor.Decrypt (object format)      pkg/object/encrypt.go:196-216
 *   jfsx_open_range_batch encrypted.Get(key, off, limit): the tag   pkg/object/encrypt.go:232-255
 *                        over all of C, the window alone decrypted  (issued at pkg/chunk/cached_store.go:152-183)
 *   jfsx_checksum        checksum(data) []byte                      pkg/chunk/disk_cache.go:1218-1231
 *   jfsx_crc32c_segments the CRC loop of cacheFile.ReadAt           pkg/chunk/disk_cache.go:1315-1327
 *   jfsx_file_checksum_batch getFileChecksum (MD5-of-MD5-of-CRC32C)  sdk/java/.../JuiceFileSystemImpl.java:1286-1343
 *   jfsx_cache_verify    cacheFile.ReadAt level logic + verify      pkg/chunk/disk_cache.go:1255-1329
 *   jfsx_object_crc32c   generateChecksum / checksumReader of the   pkg/object/checksum.go:31-82
 *   (+ JFSX_CRC_CT)      stored object, fused with Seal/Open        (s3.go:140-146,173-176)
 *   jfsx_load_batch      cachedStore.load's Decrypt + Decompress +  pkg/chunk/cached_store.go:673-748
 *                        bcache.cache's checksum(), one call        (disk_cache.go:433-483)
 *   jfsx_load_objects    the same from the stored object: the       pkg/object/checksum.go:55-82,
 *                        store's checksum verify, Decrypt with its  encrypt.go:196-216, :132-134
 *                        key unwrap, Decompress, checksum()
 *   jfsx_store_batch     uploadStagingFile's verified re-read +     pkg/chunk/cached_store.go:944-999, :371-413
 *                        upload's Compress + Encrypt + checksums,   (disk_cache.go:433-483, checksum.go:31-53)
 *                        one call
 *   jfsx_store_objects   the same up to the stored object: the key  pkg/object/encrypt.go:164-194,
 *                        wrap, header | C | tag, its checksum       checksum.go:31-53
 *   jfsx_compact_objects vfs.Compact: readSlice of the live ranges,  pkg/vfs/compact.go:54-109,
 *                        zeros for holes, wSlice.upload of the new  pkg/chunk/cached_store.go:96-190
 *                        slice; jfsx_compact_plan, jfsx_gather_batch
 *   jfsx_rsa_oaep_decrypt_batch  rsaEncryptor.Decrypt, per read window  pkg/object/encrypt.go:132-134 (called :207-210)
 *   jfsx_rsa_oaep_encrypt_batch  rsaEncryptor.Encrypt, per upload window pkg/object/encrypt.go:128-130 (called :169)
 *   JFSX_AES256GCM /     NewDataEncryptor algo "aes256gcm-rsa" /    pkg/object/encrypt.go:142-162
 *   JFSX_CHACHA20P1305   "chacha20-rsa"
 *
 * RSA keys of 2048 and of 4096 bits are taken (jfsx_rsa_key_new), by every
 * call that takes a jfsx_rsa_key; 3072 bits and every other size are refused
 * there with JFSX_EINVAL and stay with the caller's own RSA.
 * RSA-OAEP key wrapping (encrypt.go:124-134) is a batch call of its own on
 * either side (jfsx_rsa_oaep_encrypt_batch / _decrypt_batch); the AEAD entry
 * points take the already-wrapped key bytes.  Randomness stays with the
 * caller: the engine takes the 32-byte data key, the 12-byte nonce and the
 * 32-byte OAEP seed per block as inputs (the reference draws all three from
 * crypto/rand, encrypt.go:165-180 and rsa.EncryptOAEP) and draws none itself.
 *
 * Threading: a context may be used from several host threads; calls on one
 * context are serialised internally (one HIP stream per context).  Use one
 * context per GPU (per device ordinal) and per submitting thread for
 * concurrency.
 *
 * Return codes: 0 on success, negative errno-style values on batch-level
 * failure (JFSX_EINVAL, JFSX_ENODEV, JFSX_EIO, JFSX_ENOMEM).  Per-block
 * results are in jfsx_blk.status.
 */
#ifndef JFSX_H
#define JFSX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JFSX_ABI_VERSION 9

/* algorithms (encrypt.go:142-145) */
#define JFSX_AES256GCM 0     /* "aes256gcm-rsa" (also the "" default)   */
#define JFSX_CHACHA20P1305 1 /* "chacha20-rsa"                          */

/* CRC32C segment checksum mode, per 32 KiB segment of the PLAINTEXT
 * (csBlock = 32 KiB, disk_cache.go:1207).  CRC arrays are big-endian uint32
 * per segment, exactly the bytes checksum() returns (buffer.go:42-44,98-101);
 * a zero-length block has one zero CRC (4 bytes), as checksum() does. */
#define JFSX_CRC_NONE 0   /* no checksum                                  */
#define JFSX_CRC_GEN 1    /* write crc[] (level != none on cache write)   */
#define JFSX_CRC_VERIFY 2 /* compare against crc[] (cache read verify)    */
/* flag OR'ed into GEN/VERIFY: the segment CRCs cover the ciphertext C (seal:
 * output, open: input) instead of the plaintext -- the bytes the object store
 * checksums (pkg/object/checksum.go:31-53, s3.go:173-176); fold them into the
 * whole-object value with jfsx_object_crc32c. */
#define JFSX_CRC_CT 4
/* flag OR'ed into JFSX_CRC_GEN only: BOTH checksums in one call -- crc points
 * at 8*max(1,ceil(len/32K)) bytes, the plaintext segment CRCs (checksum() of
 * the block, as CRC_GEN) followed by the ciphertext segment CRCs (as
 * CRC_GEN|CRC_CT).  This is what an upload of one block to an S3-class store
 * with a disk cache needs: bcache.stage checksums the plaintext and the store's
 * Put checksums the sealed object (pkg/chunk/cached_store.go:439-451,
 * pkg/object/s3.go:173-176).  The ciphertext pass runs on the copy of the
 * block already in device memory, so it adds no host or PCIe traffic. */
#define JFSX_CRC_BOTH 8

/* where src/dst/crc pointers of a batch live */
#define JFSX_MEM_DEVICE 0 /* device memory (jfsx_alloc_device / hipMalloc) */
#define JFSX_MEM_HOST 1   /* host memory; staged through the engine          */
/* JFSX_MEM_HOST buffers may be page-locked (jfsx_alloc_pinned*, or memory the
 * HIP runtime knows as registered) or ordinary pageable memory (a Go-heap
 * slice, malloc).  Page-locked blocks are copied by DMA directly; the engine
 * copies a pageable block into pinned staging it owns on the calling thread
 * before the upload, and a pageable output out of it after the download, and
 * never keeps a pointer to caller memory past the call (cgo's rules). */

/* per-block status */
#define JFSX_OK 0
#define JFSX_ETAG 1 /* AEAD authentication failed (Go: cipher's errOpen)      */
#define JFSX_ECRC 2 /* "data checksum %d != expect %d" (disk_cache.go:1324)   */
#define JFSX_EOF 3  /* jfsx_cache_verify: short read (File.ReadAt's io.EOF)    */
#define JFSX_EFORMAT 4 /* malformed LZ4 block / zstd frame (the library's error) */
#define JFSX_EDSTSIZE 5 /* zstd: the frames decode to more than dst_cap bytes */

/* batch-level errors */
#define JFSX_EINVAL (-22)
#define JFSX_ENODEV (-19)
#define JFSX_EIO (-5)
#define JFSX_ENOMEM (-12)
#define JFSX_EAGAIN (-11) /* jfsx_wait: not finished within the timeout     */
#define JFSX_EMISFORMED (-74) /* "misformed ciphertext: %d %d" (encrypt.go:199-201) */

typedef struct jfsx_ctx jfsx_ctx;

/* One 4 MiB-class block.  For JFSX_MEM_DEVICE batches src/dst must be
 * 16-byte aligned; dst may equal src (in place, as aead.Seal(p[:0]...) and
 * aead.Open(ciphertext[:0]...) are).  Length limits (JFSX_EINVAL beyond them):
 *   AES-256-GCM        len <= (2^32 - 2) * 16 B  (the cipher's own: 32-bit
 *                      block counter from 2; crypto/cipher gcm.go
 *                      gcmMaxPlaintext, where Go's Seal panics and Open fails)
 *   ChaCha20-Poly1305  len <= (2^32 - 1) * 16 B  (the engine's: it counts
 *                      Poly1305 blocks in 32 bits; just under 64 GiB, below
 *                      the cipher's 2^38 - 64 B of x/crypto v0.19.0
 *                      chacha20poly1305.go)
 * Open with a failed tag (status JFSX_ETAG) releases nothing: dst is zeroed,
 * as Go's in-place aead.Open (encrypt.go:215) clears out on a mismatch, and a
 * plaintext CRC_GEN array is zeroed too. */
typedef struct jfsx_blk {
    uint8_t key[32];      /* data key (encrypt.go:165)                        */
    uint8_t nonce[12];    /* nonce (encrypt.go:177)                           */
    uint32_t reserved;    /* must be 0                                        */
    const void *src;      /* seal: plaintext  / open: ciphertext (no tag)     */
    void *dst;            /* seal: ciphertext / open: plaintext               */
    uint64_t len;         /* bytes of src/dst                                 */
    uint8_t tag[16];      /* seal: out / open: in                             */
    uint8_t *crc;         /* GEN: out, VERIFY: in; 4*max(1,ceil(len/32K)) B   */
    int32_t status;       /* out: JFSX_OK / JFSX_ETAG / JFSX_ECRC             */
    int32_t crc_bad_seg;  /* out: first failing segment (VERIFY), else -1     */
    uint32_t crc_got;     /* out: CRC computed for crc_bad_seg                */
    uint32_t crc_expect;  /* out: CRC expected for crc_bad_seg                */
} jfsx_blk;

/* One checksum range: [data, data+len) is a segment-aligned window of a
 * cache block; crc[k] is the BE32 CRC of its k-th 32 KiB segment. */
typedef struct jfsx_range {
    const void *data;
    uint64_t len;
    uint8_t *crc;         /* GEN: out, VERIFY: in                             */
    int32_t status;       /* out: JFSX_OK / JFSX_ECRC                         */
    int32_t bad_seg;      /* out: first failing segment, -1 none              */
    uint32_t got, expect; /* out                                              */
} jfsx_range;

int jfsx_abi_version(void);
int jfsx_device_count(int *n);

/* Diagnostics for a batch-level JFSX_EIO / JFSX_ENOMEM: the HIP failure behind
 * it, as its hipError_t value and "name (text) at file:line in call", for the
 * calls made on ctx (from any thread, the aggregator's dispatchers and the
 * async queue's worker included) or, with ctx NULL, for the calling thread.
 * hip_error 0 and an empty msg when none was recorded; a newer failure
 * replaces an older one.  A sticky device fault (hipErrorIllegalAddress and
 * the like) leaves the context unusable: close it and fall back.  The Go shim
 * logs this text before it falls back to the CPU path. */
int jfsx_last_error(jfsx_ctx *ctx, int *hip_error, char *msg, size_t cap);

/* context = one GPU + one HIP stream + device workspace + pinned staging.
 * flags: 0, or JFSX_CTX_BITSLICE: AES-256-GCM computes the keystream of whole
 * 32 KiB segments with the bitsliced AES on the VALU instead of the T-table
 * AES in LDS (same bytes; a throughput trade-off). */
#define JFSX_CTX_BITSLICE 1u
/* AES-256-GCM's fused CRC32C in the T-table kernel: where the CRC covers the
 * side the kernel loads (Seal over the plaintext, Open with JFSX_CRC_CT), part
 * of its table lookups can go through the vector L1 instead of the LDS (same
 * bytes).  JFSX_CTX_CRC_LDS: all from the LDS;
 * JFSX_CTX_CRC_L1: the L1 path; neither: JFSX_CRC_L1=0/1 in the environment
 * when the context opens, else the build's default.  Both: JFSX_EINVAL. */
#define JFSX_CTX_CRC_LDS 2u
#define JFSX_CTX_CRC_L1 4u
int jfsx_ctx_open(int device, uint32_t flags, jfsx_ctx **out);
int jfsx_ctx_close(jfsx_ctx *ctx);
int jfsx_ctx_sync(jfsx_ctx *ctx);
/* returns the context's hipStream_t (as void*) for callers that order their
 * own copies against the engine's work */
void *jfsx_ctx_stream(jfsx_ctx *ctx);
/* kernel timing: when enabled, HIP events bracket the main transform kernel of
 * every batch on the context's stream; query returns the summed milliseconds
 * and the number of launches since the last reset */
int jfsx_ctx_set_timing(jfsx_ctx *ctx, int enable);
/* host-ingest pipeline slot size (default 256 MiB): JFSX_MEM_HOST batches are
 * streamed through 3 device staging slots of this size, H2D | transform | D2H
 * overlapped on three streams */
int jfsx_ctx_set_slot_bytes(jfsx_ctx *ctx, uint64_t bytes);
int jfsx_ctx_kernel_time(jfsx_ctx *ctx, double *ms_total, uint64_t *launches, int reset);

/* Engine counters for the shim's metrics hooks -- the byte / op counters the
 * reference keeps around the block path (cachedStore's Prometheus collectors,
 * pkg/chunk/cached_store.go:847-932: object request bytes and durations,
 * cache hits / misses / read bytes).  Per context, cumulative since open or the
 * last reset; a batch is counted when it returns 0.  bytes = plaintext
 * (AEAD), range (CRC) and input / output (codecs); *_fail = blocks whose
 * status was not JFSX_OK (tag, checksum, malformed, too small).  zstd_serial =
 * zstd objects the block-parallel decoder handed to the serial decoder (frame
 * shapes outside its fast path, or frames it rejects).  kernel_ms /
 * kernel_launches: the main-kernel time, counted only while
 * jfsx_ctx_set_timing is enabled. */
typedef struct jfsx_metrics {
    uint64_t seal_batches, seal_blocks, seal_bytes;
    uint64_t open_batches, open_blocks, open_bytes, open_fail;
    uint64_t crc_batches, crc_ranges, crc_bytes, crc_fail;
    uint64_t lz4c_blocks, lz4c_in, lz4c_out;
    uint64_t lz4d_blocks, lz4d_in, lz4d_out, lz4d_fail;
    uint64_t zstdc_blocks, zstdc_in, zstdc_out;
    uint64_t zstdd_blocks, zstdd_in, zstdd_out, zstdd_fail, zstd_serial;
    double kernel_ms;
    uint64_t kernel_launches;
} jfsx_metrics;
int jfsx_ctx_metrics(jfsx_ctx *ctx, jfsx_metrics *out, int reset);

/* memory helpers (engine-owned pinned staging, device buffers); pinned memory
 * is portable: any context of the process (any GPU) may stream from it.
 * Device buffers from jfsx_alloc_device are registered by address, so a
 * multi-device context can route a device-memory block to the GPU that owns
 * it (jfsx_mctx_seal_batch with JFSX_MEM_DEVICE). */
int jfsx_alloc_pinned(jfsx_ctx *ctx, size_t bytes, void **p);
int jfsx_free_pinned(jfsx_ctx *ctx, void *p);
int jfsx_alloc_device(jfsx_ctx *ctx, size_t bytes, void **p);
int jfsx_free_device(jfsx_ctx *ctx, void *p);

/* NUMA placement of pinned staging, so that at N GPUs on a multi-socket node
 * every GPU streams from memory on its own socket (the reference's uploaders
 * fill Go-heap pages wherever the scheduler ran them, pkg/chunk/page.go:33-60;
 * the shim copies them into this staging).
 *   jfsx_device_numa_node  host NUMA node closest to `device` (-1 unknown)
 *   jfsx_alloc_pinned_node pinned portable memory whose pages are bound to
 *                          `node` while they are allocated (-1: the node of the
 *                          context's device); where the node cannot be bound
 *                          (a cpuset without it) the default placement is used
 *   jfsx_host_numa_node    node of the pages of [p, p+bytes), sampled every
 *                          64 MiB: -1 unknown, -2 pages on more than one node
 * Free with jfsx_free_pinned. */
int jfsx_device_numa_node(int device, int *node);
int jfsx_alloc_pinned_node(jfsx_ctx *ctx, size_t bytes, int node, void **p);
int jfsx_host_numa_node(const void *p, size_t bytes, int *node);
int jfsx_memcpy_h2d(jfsx_ctx *ctx, void *dst, const void *src, size_t bytes);
int jfsx_memcpy_d2h(jfsx_ctx *ctx, void *dst, const void *src, size_t bytes);

/* Batched AEAD over blocks, fused with CRC32C segment checksums of the
 * plaintext.  mem = JFSX_MEM_DEVICE or JFSX_MEM_HOST.  Synchronous: returns
 * when tags, CRCs and statuses are written back into blks.
 * JFSX_MEM_HOST batches stream through the context's pipeline of 8 staging
 * slots (H2D | transform | D2H on three streams).  The pipeline is shared by
 * every thread calling on the context and never drains between calls: a call
 * enqueues its groups and then waits for its own groups only, so concurrent
 * callers (the aggregator's dispatchers, per-object shims) keep both copy
 * directions busy back to back.  Device batches hold the context for the
 * whole call. */
int jfsx_seal_batch(jfsx_ctx *ctx, int algo, int n, jfsx_blk *blks, int crc_mode, int mem);
int jfsx_open_batch(jfsx_ctx *ctx, int algo, int n, jfsx_blk *blks, int crc_mode, int mem);

/* CRC32C per 32 KiB segment over n ranges (cache-hit verify, none-cipher
 * volumes, staging re-read).  mode = JFSX_CRC_GEN or JFSX_CRC_VERIFY. */
int jfsx_crc32c_segments(jfsx_ctx *ctx, int n, jfsx_range *ranges, int mode, int mem);

/* Asynchronous variants: the batch is queued on the context's worker thread
 * (batches of one context run in submission order) and the call returns a
 * ticket at once.  blks/ranges and every buffer they name must stay valid
 * until jfsx_wait has returned for the ticket.  jfsx_wait returns the batch's
 * return code (as the synchronous call would) and retires the ticket;
 * timeout_ms < 0 waits without limit, 0 polls; JFSX_EAGAIN if the batch has
 * not finished in time (the ticket stays live).  jfsx_ctx_close runs the
 * queued batches before it releases the context. */
typedef uint64_t jfsx_ticket;
int jfsx_seal_batch_async(jfsx_ctx *ctx, int algo, int n, jfsx_blk *blks, int crc_mode, int mem, jfsx_ticket *t);
int jfsx_open_batch_async(jfsx_ctx *ctx, int algo, int n, jfsx_blk *blks, int crc_mode, int mem, jfsx_ticket *t);
int jfsx_crc32c_segments_async(jfsx_ctx *ctx, int n, jfsx_range *ranges, int mode, int mem, jfsx_ticket *t);
int jfsx_wait(jfsx_ctx *ctx, jfsx_ticket t, int timeout_ms);

/* Aggregator: per-block calls in the reference's shape --
 * one synchronous Encrypt / Decrypt / cache-read verify per goroutine
 * (encrypt.go:164-216, disk_cache.go:1315-1327) -- coalesced into batches.
 * jfsx_agg_seal / _open / _crc32c block the calling thread until its block
 * is done and return what a one-block batch would (per-block results in
 * blk->status or range->status).  Any number of threads may call at once.  A
 * dispatcher thread groups waiting requests with the same (op, algo, mode,
 * mem) and issues one batch when the group reaches max_blocks (0: 256) or
 * max_bytes (0: 1 GiB), or when the oldest request has waited window_us.  A
 * request the engine rejects (JFSX_EINVAL) fails alone: the batch is retried
 * one request at a time.  Free the aggregator before closing its context. */
typedef struct jfsx_agg jfsx_agg;
int jfsx_agg_new(jfsx_ctx *ctx, int max_blocks, uint64_t max_bytes, uint32_t window_us, jfsx_agg **out);
int jfsx_agg_free(jfsx_agg *agg);
int jfsx_agg_seal(jfsx_agg *agg, int algo, jfsx_blk *blk, int crc_mode, int mem);
int jfsx_agg_open(jfsx_agg *agg, int algo, jfsx_blk *blk, int crc_mode, int mem);
int jfsx_agg_crc32c(jfsx_agg *agg, jfsx_range *range, int mode, int mem);
/* requests taken, batches issued, requests those batches carried */
int jfsx_agg_stats(jfsx_agg *agg, uint64_t *calls, uint64_t *batches, uint64_t *blocks);
/* Dispatch: each context gets several dispatcher threads (4; the environment
 * variable JFSX_AGG_DISPATCHERS overrides, 1..32), so several batches of one
 * device are in flight at once (host batches pipeline, see jfsx_seal_batch).
 * A group waits for its window only while the engine is idle; while another
 * of the aggregator's batches is running, a free dispatcher takes what is
 * queued at once (the time spent queued behind the running batch is the
 * batching).  For per-object callers in host memory keep max_bytes near
 * 16 MiB, so that a 20-caller closed loop (max-uploads) is cut into several
 * batches in flight instead of one batch that all callers wait for. */

/* dataEncryptor.Encrypt / Decrypt (encrypt.go:164-216) through the
 * aggregator: the same object format and results as jfsx_data_encrypt /
 * jfsx_data_decrypt, with the Seal / Open issued as one aggregated request, so
 * the shim's per-object Encrypt from max-uploads goroutines batches. */
int jfsx_agg_data_encrypt(jfsx_agg *agg, int algo, const uint8_t key[32], const uint8_t nonce[12],
                          const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                          uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc);
int jfsx_agg_data_decrypt(jfsx_agg *agg, int algo, const uint8_t key[32], const void *obj, uint64_t olen, void *out,
                          uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc, uint32_t *got_crc);
/* The same, and checksum() of the plaintext in the same pass (seg_crc,
 * nullable: 4*max(1,ceil(len/32K)) bytes, the cache file's trailer): the
 * block the reference touches twice -- wSlice.upload stages it in the disk
 * cache (bcache.stage -> checksum, disk_cache.go:433-483) and then uploads it
 * (store.upload -> Encrypt, cached_store.go:415-472); store.load decrypts it
 * and then caches it (bcache.cache -> checksum, cached_store.go:673-748) --
 * crosses PCIe once.  With obj_crc / expect_crc as well, both checksums come
 * out of the one call (JFSX_CRC_BOTH).  Decrypt: seg_crc is zeroed when the
 * call fails (tag or object checksum), as the plaintext is. */
int jfsx_agg_data_encrypt_ex(jfsx_agg *agg, int algo, const uint8_t key[32], const uint8_t nonce[12],
                             const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                             uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc, uint8_t *seg_crc);
int jfsx_agg_data_decrypt_ex(jfsx_agg *agg, int algo, const uint8_t key[32], const void *obj, uint64_t olen,
                             void *out, uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc,
                             uint32_t *got_crc, uint8_t *seg_crc);

/* Multi-device context (SURVEY §8b jfsx_open_ctx(dev_mask), §8e): one
 * jfsx_ctx per selected GPU (bit d of dev_mask = device d; 0 = every visible
 * device).  Blocks are independent (own key, nonce, tag, CRCs), so the parts
 * of a batch run concurrently, one persistent worker thread per device; no
 * device-to-device traffic.  A JFSX_MEM_HOST batch is cut into one contiguous
 * run of blocks per device, balanced by bytes.  A JFSX_MEM_DEVICE batch is
 * routed by ownership: every block goes to the GPU whose memory holds its
 * src, dst and crc (buffers from jfsx_alloc_device on a member context, or any
 * device allocation); a block whose buffers span GPUs, or live on a GPU
 * outside the context, fails the batch with JFSX_EINVAL before anything runs.
 * Results land in blks exactly as with a single context.  A batch-level error
 * of any device is returned (the first one, in device order). */
typedef struct jfsx_mctx jfsx_mctx;
int jfsx_mctx_open(uint64_t dev_mask, uint32_t flags, jfsx_mctx **out);
int jfsx_mctx_close(jfsx_mctx *m);
int jfsx_mctx_ndev(jfsx_mctx *m);                 /* devices in the context   */
jfsx_ctx *jfsx_mctx_ctx(jfsx_mctx *m, int i);     /* i-th device's context    */
int jfsx_mctx_seal_batch(jfsx_mctx *m, int algo, int n, jfsx_blk *blks, int crc_mode, int mem);
int jfsx_mctx_open_batch(jfsx_mctx *m, int algo, int n, jfsx_blk *blks, int crc_mode, int mem);
int jfsx_mctx_crc32c_segments(jfsx_mctx *m, int n, jfsx_range *ranges, int mode, int mem);
/* Aggregator over every device of a multi-device context: one dispatcher
 * thread per device takes the next ready group from one shared queue, so the
 * per-block callers (≤ max-uploads upload goroutines, cached_store.go:371-472;
 * readers, :673-748) spread over all GPUs.  Same call semantics as jfsx_agg_new. */
int jfsx_agg_new_mctx(jfsx_mctx *m, int max_blocks, uint64_t max_bytes, uint32_t window_us, jfsx_agg **out);
/* batches issued by the aggregator's dispatcher for device slot i */
int jfsx_agg_dev_batches(jfsx_agg *agg, int i, uint64_t *batches);

/* checksum(data) on the GPU: out receives 4*max(1,ceil(len/32K)) bytes.
 * data and out are host memory. */
int jfsx_checksum(jfsx_ctx *ctx, const void *data, uint64_t len, uint8_t *out);

/* Hadoop's file checksum, MD5-of-MD5-of-CRC32C, what `hadoop fs -checksum` and
 * distcp compare (getFileChecksum, sdk/java/src/main/java/io/juicefs/
 * JuiceFileSystemImpl.java:1286-1343): a CRC32C per bytes_per_crc chunk (big
 * endian), an MD5 over the chunk CRCs of every block_bytes of the file, and an
 * MD5 over Hadoop's DataOutputBuffer of the block digests (its whole backing
 * array: the 16 k digest bytes zero-padded to the smallest 32 * 2^j >= 16 k).
 * A span with no chunk gives MD5(32 zero bytes) with crc32c = 0 and
 * bytes_per_crc = crc_per_block = 0; otherwise crc32c = 1, bytes_per_crc as
 * given and crc_per_block = len > block_bytes ? block_bytes / bytes_per_crc : 0. */
typedef struct jfsx_fsum {
    const void *data;        /* the span to hash: bytes [0, len) of the file   */
    uint64_t len;            /* = jfsx_file_checksum_span(...)                 */
    uint8_t md5[16];         /* out                                            */
    uint32_t bytes_per_crc;  /* out: 512, or 0 when no chunk                   */
    uint32_t crc32c;         /* out: 1 CRC32C, 0 CRC32 (the no-chunk case)     */
    uint64_t crc_per_block;  /* out                                            */
} jfsx_fsum;
/* bytes of a file of file_size that getFileChecksum(f, length) hashes: it reads
 * bytes_per_crc at a time while it has fewer than length, so a length that is
 * no chunk multiple runs on to the chunk end (or EOF), except below one chunk */
uint64_t jfsx_file_checksum_span(uint64_t file_size, uint64_t length, uint32_t bytes_per_crc);
/* n files in one call: one chunk-CRC launch over all of them, one MD5 launch
 * over all their blocks, one download of 16 bytes per block, the last MD5 on
 * the host.  bytes_per_crc must be 512; block_bytes a non-zero multiple of it.
 * JFSX_MEM_DEVICE: data 16-byte aligned.  JFSX_MEM_HOST: pageable or pinned
 * memory at any alignment, staged through engine-owned pinned memory. */
int jfsx_file_checksum_batch(jfsx_ctx *ctx, int n, jfsx_fsum *files,
                             uint32_t bytes_per_crc, uint64_t block_bytes, int mem);
/* host only, no device: the block and file MD5s over chunk CRCs already computed
 * (big-endian words), e.g. by the fused Seal/Open CRC_GEN of a <= 512 B block */
int jfsx_file_checksum_fold(const uint8_t *chunk_crcs, uint64_t nchunks, uint64_t span_len,
                            uint32_t bytes_per_crc, uint64_t block_bytes, jfsx_fsum *out);

/* cacheFile.ReadAt verify (disk_cache.go:1255-1329) over an in-memory cache
 * file image: file = data(length) ‖ BE32 CRCs, level 0 none / 1 full /
 * 2 shrink / 3 extend (the level openCacheFile resolved).  Copies
 * [off, off+size) into out.  Returns 0 ok, JFSX_ECRC on mismatch (got,
 * expect, bad_seg filled), JFSX_EOF on a short read, <0 on argument errors.
 * *n_out is what Go's ReadAt returns as n.  file and out are host memory of
 * any alignment; the verified window is staged through a per-context pinned
 * arena (no per-call allocation). */
int jfsx_cache_verify(jfsx_ctx *ctx, const void *file, uint64_t file_size, uint64_t length, int level,
                      uint64_t off, uint64_t size, void *out, uint64_t *n_out, uint32_t *got,
                      uint32_t *expect, int64_t *bad_seg);

/* dataEncryptor.Encrypt with an already-wrapped key: writes
 * BE16(wlen) | 12 | wrapped | nonce | C | tag into out (host memory).
 * out_cap must be >= 3+wlen+12+len+16.  obj_crc (nullable) receives the
 * object-store checksum of the whole output, generateChecksum's value
 * (checksum.go:31-53), computed in the same pass as the Seal. */
int jfsx_data_encrypt(jfsx_ctx *ctx, int algo, const uint8_t key[32], const uint8_t nonce[12],
                      const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                      uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc);
/* dataEncryptor.Decrypt after the key is unwrapped: parses the header
 * (JFSX_EMISFORMED if 3+klen+nlen >= olen), opens, and writes the plaintext
 * to out only when the tag verifies (returns JFSX_ETAG otherwise).  With
 * expect_crc non-null the object checksum is verified in the same pass
 * (checksumReader, checksum.go:55-82): on mismatch returns JFSX_ECRC with the
 * computed value in *got_crc ("verify checksum failed: %d != %d") and releases
 * no plaintext; the checksum failure takes precedence over JFSX_ETAG. */
int jfsx_data_decrypt(jfsx_ctx *ctx, int algo, const uint8_t key[32], const void *obj, uint64_t olen,
                      void *out, uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc,
                      uint32_t *got_crc);
/* the two above with checksum() of the plaintext in the same pass (seg_crc,
 * nullable; see jfsx_agg_data_encrypt_ex) */
int jfsx_data_encrypt_ex(jfsx_ctx *ctx, int algo, const uint8_t key[32], const uint8_t nonce[12],
                         const uint8_t *wrapped, int wlen, const void *plaintext, uint64_t len, void *out,
                         uint64_t out_cap, uint64_t *out_len, uint32_t *obj_crc, uint8_t *seg_crc);
int jfsx_data_decrypt_ex(jfsx_ctx *ctx, int algo, const uint8_t key[32], const void *obj, uint64_t olen,
                         void *out, uint64_t out_cap, uint64_t *out_len, const uint32_t *expect_crc,
                         uint32_t *got_crc, uint8_t *seg_crc);

/* Ranged Open -- encrypted.Get(key, off, limit) (pkg/object/encrypt.go:232-255),
 * the read rSlice.ReadAt issues for a small read that misses the cache on an
 * encrypted, uncompressed volume (pkg/chunk/cached_store.go:152-183).  The tag
 * is checked over all of C, the keystream runs only under the window, and only
 * the window is released.  The window is Go's slice rule (encrypt.go:246-253):
 *   o = min(off, len);  n = (limit == -1 || limit > len - o) ? len - o : limit
 * Per block: the tag is always checked, for n == 0 and len == 0 too (Go
 * decrypts before it slices).  JFSX_OK: out_len = n and dst[0, n) holds the
 * plaintext bytes [o, o + n), the bytes jfsx_open_batch writes at dst + o.
 * JFSX_ETAG: out_len = 0 and dst[0, n) is zero.  No byte of dst at or past n
 * is written; with n == 0 dst may be NULL and is not touched.
 * crc_mode: JFSX_CRC_NONE, or JFSX_CRC_GEN | JFSX_CRC_CT, which fills crc
 * with what jfsx_open_batch returns in that mode (the ciphertext segment CRCs
 * of all of C, on a good tag and on a bad one).  The plaintext outside the
 * window is never formed, so the plaintext CRC modes are JFSX_EINVAL.
 * JFSX_EINVAL before anything runs, with the records untouched: an unknown
 * algo, any other crc_mode, reserved or reserved2 non-zero, limit < -1, len
 * beyond the cipher's limit (jfsx_blk), dst_cap < n, a NULL dst with n > 0, a
 * NULL crc with GEN | CT, a NULL src with len > 0; with JFSX_MEM_DEVICE also
 * src, dst or crc not 16-byte aligned, or dst[0, dst_cap) overlapping
 * src[0, len).  off and limit have no alignment rule.  Blocks with n == 0 and
 * a batch of no blocks are legal.
 * JFSX_MEM_HOST: pageable or pinned memory at any alignment; C goes up once
 * and exactly n bytes come down, only for a block whose tag verified.  The
 * call is synchronous and single-buffered.
 * Metrics: a returned batch counts as open_batches / open_blocks; open_bytes
 * grows by len, the bytes authenticated; open_fail counts per JFSX_ETAG. */
typedef struct jfsx_rblk {
    uint8_t key[32];      /* data key                                         */
    uint8_t nonce[12];    /* nonce                                            */
    uint32_t reserved;    /* must be 0                                        */
    uint8_t tag[16];      /* in                                               */
    const void *src;      /* C, the whole ciphertext without header and tag   */
    uint64_t len;         /* bytes of C = bytes of the plaintext              */
    uint64_t off;         /* encrypted.Get's off                              */
    int64_t limit;        /* encrypted.Get's limit; -1: to the end            */
    void *dst;            /* receives the window only                         */
    uint64_t dst_cap;
    uint8_t *crc;         /* GEN|CT: out, 4*max(1,ceil(len/32K)) B            */
    uint64_t out_len;     /* out                                              */
    int32_t status;       /* out: JFSX_OK / JFSX_ETAG                         */
    int32_t reserved2;    /* must be 0                                        */
} jfsx_rblk;
int jfsx_open_range_batch(jfsx_ctx *ctx, int algo, int n, jfsx_rblk *blks, int crc_mode, int mem);
/* one more aggregator op: requests with the same (algo, crc_mode, mem)
 * coalesce into jfsx_open_range_batch calls, with jfsx_agg_open's semantics
 * (a request the engine rejects fails alone) */
int jfsx_agg_open_range(jfsx_agg *agg, int algo, jfsx_rblk *blk, int crc_mode, int mem);
/* jfsx_data_decrypt with the window: the same header parsing and
 * JFSX_EMISFORMED, JFSX_ECRC before JFSX_ETAG when expect_crc is given;
 * *out_len = n on success, out_cap >= n; nothing is released on any failure */
int jfsx_data_decrypt_range(jfsx_ctx *ctx, int algo, const uint8_t key[32], const void *obj, uint64_t olen,
                            uint64_t off, int64_t limit, void *out, uint64_t out_cap, uint64_t *out_len,
                            const uint32_t *expect_crc, uint32_t *got_crc);

/* crc32.Update(crc, MakeTable(Castagnoli), data) on the host (small spans:
 * object header and tag) */
uint32_t jfsx_crc32c_update(uint32_t crc, const void *data, uint64_t n);
/* CRC32C of A||B from crc(A), crc(B), len(B) (GF(2) shift by x^(8 len B)) */
uint32_t jfsx_crc32c_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);
/* Batched RSA-OAEP key unwrap: replaces, per object,
 * rsaEncryptor.Decrypt = rsa.DecryptOAEP(sha256, rand, priv, wrapped,
 * label) (pkg/object/encrypt.go:124-134, called at :207-210) for every object
 * of a batch at once, on the GPU.  The key is given by its CRT components
 * (Go's Primes[0], Primes[1], Precomputed.Dp, Dq, Qinv), big-endian,
 * prime_bytes each.  Two key sizes are taken: RSA-2048 (prime_bytes = 128,
 * modulus length k = 256) and RSA-4096 (prime_bytes = 256, k = 512), with odd
 * primes whose top bit is set and dp, dq >= 2.  Every other prime_bytes (64,
 * 192 for a 3072-bit key, 512, ...) is JFSX_EINVAL: such a volume keeps the
 * host's rsa.DecryptOAEP / EncryptOAEP.  Keys of both sizes may be live on one
 * context.  jfsx_rsa_key_bytes returns k (JFSX_EINVAL for a NULL key).
 * ct: host memory, item i at ct + i*ct_stride, ct_len[i] <= k bytes (a shorter
 * one is the big-endian integer it is; 0 or more than k bytes is the
 * decryption error).  msg_len[i] = message length (up to k - 66), or -1 for
 * the decryption error (Go's "crypto/rsa: decryption error"); up to msg_stride
 * bytes of each message are copied to msg + i*msg_stride. */
typedef struct jfsx_rsa_key jfsx_rsa_key;
int jfsx_rsa_key_new(jfsx_ctx *ctx, const uint8_t *p, const uint8_t *q, const uint8_t *dp, const uint8_t *dq,
                     const uint8_t *qinv, int prime_bytes, const uint8_t *label, int label_len, jfsx_rsa_key **out);
int jfsx_rsa_key_free(jfsx_rsa_key *key);
int jfsx_rsa_key_bytes(const jfsx_rsa_key *key);
int jfsx_rsa_oaep_decrypt_batch(jfsx_ctx *ctx, const jfsx_rsa_key *key, int n, const uint8_t *ct, uint64_t ct_stride,
                                const uint32_t *ct_len, uint8_t *msg, uint64_t msg_stride, int32_t *msg_len);
/* Batched RSA-OAEP key wrap, the write side of the unwrap: replaces, per
 * object, rsaEncryptor.Encrypt = rsa.EncryptOAEP(sha256, rand, &priv.PublicKey,
 * key, label) (pkg/object/encrypt.go:128-130, called at :169) for every object
 * of an upload window at once, on the GPU.  key: as above (its n = p q and its
 * label); e: the public exponent, 2 <= e <= 2^31 - 1 as Go's checkPub takes it.
 * All pointers are host memory.  Item i reads msg_len[i] bytes at msg +
 * i*msg_stride and its 32-byte OAEP seed at seed + 32*i: the seeds are the
 * caller's randomness (Go reads them from rand), the engine draws none.  It
 * writes exactly k = jfsx_rsa_key_bytes(key) bytes (256 or 512) at ct +
 * i*ct_stride.  status[i] = 0, or -1 for Go's "message too long for RSA key
 * size" (msg_len[i] > k - 66, that is 190 or 446; the k bytes are then zero,
 * the other items unaffected).  JFSX_EINVAL, before anything runs: null seed,
 * ct or status, ct_stride < k, msg_len[i] > msg_stride, e out of range, n < 0.
 * n == 0 returns 0. */
int jfsx_rsa_oaep_encrypt_batch(jfsx_ctx *ctx, const jfsx_rsa_key *key, uint32_t e, int n, const uint8_t *msg,
                                uint64_t msg_stride, const uint32_t *msg_len, const uint8_t *seed /* n x 32 bytes */,
                                uint8_t *ct, uint64_t ct_stride, int32_t *status);

/* object-store checksum of header || C || tag (checksum.go:31-53) from the
 * big-endian 32 KiB segment CRCs of C that a GEN|CT batch returned */
int jfsx_object_crc32c(const void *hdr, uint64_t hlen, const uint8_t *seg_crcs, uint64_t clen,
                       const uint8_t *tag, uint32_t *out);

/* LZ4 block stage: the "lz4" Compressor of pkg/compress
 * (compress.go:107-125) that cachedStore.upload runs before the object is
 * put (cached_store.go:371-392) and cachedStore.load after it is read
 * (:680-745).  Bytes are those of the LZ4 C library the reference binds
 * through github.com/hungys/go-lz4: jfsx_lz4_compress_batch writes what
 * LZ4_compress_default(src, dst, len, bound) writes; jfsx_lz4_decompress_batch
 * decodes as LZ4_decompress_safe(src, dst, len, cap) does (status
 * JFSX_EFORMAT where it returns < 0).  One zblk per block: compress needs
 * dst_cap >= jfsx_lz4_bound(src_len) (JFSX_EINVAL otherwise), as
 * cachedStore.upload's CompressBound-sized buffer; src_len <= 0x7E000000.
 * mem = JFSX_MEM_DEVICE or JFSX_MEM_HOST.  The empty-input error of
 * LZ4.Decompress ("decompress an empty input") is the caller's: a zero-length
 * src decodes as LZ4_decompress_safe does (JFSX_EFORMAT). */
typedef struct jfsx_zblk {
    const void *src;
    uint64_t src_len;
    void *dst;
    uint64_t dst_cap;
    uint64_t out_len;  /* out: bytes written to dst                      */
    int32_t status;    /* out: JFSX_OK / JFSX_EFORMAT (decompress)       */
    int32_t reserved;  /* zstd decompress, out: 0, or why the block-parallel
                          decoder handed the object to the serial one: 1 frame
                          shape / headers, 2 Huffman stream, 3 sequence stream,
                          4 sequence execution, 5 raw / RLE block, 6 last
                          literals, 7 content size, 8 content checksum */
} jfsx_zblk;
/* LZ4_compressBound: n + n/255 + 16 (0 for n > 0x7E000000) */
uint64_t jfsx_lz4_bound(uint64_t n);
int jfsx_lz4_compress_batch(jfsx_ctx *ctx, int n, jfsx_zblk *blks, int mem);
int jfsx_lz4_decompress_batch(jfsx_ctx *ctx, int n, jfsx_zblk *blks, int mem);
/* the same per block, through the aggregator (one synchronous call per
 * goroutine, as cachedStore.upload / load call Compress / Decompress), and
 * over a multi-device context (JFSX_MEM_HOST) */
int jfsx_agg_lz4_compress(jfsx_agg *agg, jfsx_zblk *blk, int mem);
int jfsx_agg_lz4_decompress(jfsx_agg *agg, jfsx_zblk *blk, int mem);
int jfsx_mctx_lz4_compress_batch(jfsx_mctx *m, int n, jfsx_zblk *blks, int mem);
int jfsx_mctx_lz4_decompress_batch(jfsx_mctx *m, int n, jfsx_zblk *blks, int mem);

/* Zstandard decompression (load side of "zstd" volumes):
 * ZStandard.Decompress of pkg/compress (compress.go:93-100,
 * github.com/DataDog/zstd v1.5.0 -> ZSTD_decompress), as cachedStore.load
 * calls it (cached_store.go:680-745).  Each zblk's src holds zstd frames
 * (concatenated frames and skippable frames allowed, as ZSTD_decompress);
 * out_len = decoded bytes; status JFSX_EFORMAT where ZSTD_decompress returns
 * an error (malformed frame, dictionary id, checksum mismatch, or output
 * larger than dst_cap); dst_cap < 2^31, src_len <= 0x7E000000 (JFSX_EINVAL
 * otherwise).  A frame that is well formed as far as it was decoded but does
 * not fit in dst_cap gets JFSX_EDSTSIZE (ZSTD_decompress's
 * dstSize_tooSmall): the caller can retry with the frame content size. */
int jfsx_zstd_decompress_batch(jfsx_ctx *ctx, int n, jfsx_zblk *blks, int mem);
/* per block through the aggregator, and over a multi-device context */
int jfsx_agg_zstd_decompress(jfsx_agg *agg, jfsx_zblk *blk, int mem);
int jfsx_mctx_zstd_decompress_batch(jfsx_mctx *m, int n, jfsx_zblk *blks, int mem);

/* Zstandard compression (upload side of "zstd" volumes):
 * ZStandard.Compress of pkg/compress (compress.go:82-91,
 * zstd.CompressLevel(dst, src, 1) -> ZSTD_compress(dst, bound, src, n, 1)), as
 * cachedStore.upload calls it before the Put (cached_store.go:371-392, :387).
 * Each zblk's dst receives one level-1 frame, out_len bytes, byte for byte
 * what the zstd library's one-shot level-1 compressor writes (checked against
 * the system libzstd 1.4.8; see DESIGN.md for the 1.5.0 the reference pins).
 * dst_cap >= jfsx_zstd_bound(src_len) (JFSX_EINVAL otherwise), as upload's
 * CompressBound-sized buffer; src_len <= 0x7E000000. */
uint64_t jfsx_zstd_bound(uint64_t n); /* ZSTD_compressBound */
int jfsx_zstd_compress_batch(jfsx_ctx *ctx, int n, jfsx_zblk *blks, int mem);
int jfsx_agg_zstd_compress(jfsx_agg *agg, jfsx_zblk *blk, int mem);
int jfsx_mctx_zstd_compress_batch(jfsx_mctx *m, int n, jfsx_zblk *blks, int mem);

/* One-call block load: the read miss of a volume formatted with --compress
 * lz4 / zstd (cachedStore.load, pkg/chunk/cached_store.go:673-748) -- Decrypt
 * (encrypt.go:196-216), Decompress into the page (cached_store.go:738) and
 * bcache.cache's checksum() (disk_cache.go:433-483) -- for a batch of stored
 * block images in one synchronous call.  Every intermediate stays in device
 * memory: JFSX_MEM_HOST moves each image up once and each page (with its CRC
 * array) down once, JFSX_MEM_DEVICE synchronises the stream once.  A decoder is
 * never started on bytes whose tag has not verified.
 *   algo      JFSX_AES256GCM, JFSX_CHACHA20P1305, or JFSX_CIPHER_NONE for a
 *             volume without --encrypt-rsa-key (src is the compressed block)
 *   codec     JFSX_CODEC_LZ4 or JFSX_CODEC_ZSTD (a volume with no codec is
 *             served by jfsx_open_batch with JFSX_CRC_GEN)
 *   crc_mode  JFSX_CRC_NONE or JFSX_CRC_GEN
 *   mem       JFSX_MEM_DEVICE: jfsx_blk's alignment rule where the AEAD and
 *             CRC kernels touch a buffer -- src 16-byte aligned with a cipher,
 *             dst 16-byte aligned with JFSX_CRC_GEN -- and dst distinct from
 *             src; JFSX_MEM_HOST: pageable or pinned memory at any alignment
 * Limits (JFSX_EINVAL beyond them, before anything runs): src_len <=
 * 0x7E000000, len < 2^32, and len < 2^31 for zstd.  Per-block result, the
 * first rule that applies:
 *   tag does not verify           JFSX_ETAG                          out_len 0
 *   decoder rejects the image     JFSX_EFORMAT (LZ4: also an image that
 *                                 decodes to more than len bytes), or
 *                                 JFSX_EDSTSIZE (zstd frame larger than len)
 *                                                                    out_len 0
 *   decoder produced n < len      JFSX_ESHORT                        out_len n
 *   otherwise                     JFSX_OK                            out_len len
 * On any status other than JFSX_OK the page (dst[0, len)) and the CRC array
 * are all zero when the call returns.  len == 0 is legal: the image must decode
 * to nothing, and the CRC array is 4 zero bytes, as checksum() gives.  The call
 * is counted in jfsx_metrics as the separate calls would be: open_* (unless
 * JFSX_CIPHER_NONE), lz4d_* / zstdd_* over the blocks that reached the decoder
 * (those whose tag verified), crc_* over the n pages (with JFSX_CRC_GEN). */
#define JFSX_CIPHER_NONE (-1) /* algo: the volume has no --encrypt-rsa-key      */
#define JFSX_CODEC_LZ4 1      /* compress.go:104-125                            */
#define JFSX_CODEC_ZSTD 2     /* compress.go:93-102                             */
#define JFSX_ESHORT 6 /* per-block: decoded n < len ("read %s fully: %s (%d < %d)", cached_store.go:740-743) */
typedef struct jfsx_lblk {
    uint8_t key[32];      /* as jfsx_blk; ignored with JFSX_CIPHER_NONE       */
    uint8_t nonce[12];
    uint32_t reserved;    /* must be 0                                        */
    uint8_t tag[16];      /* in; ignored with JFSX_CIPHER_NONE                */
    const void *src;      /* stored image: C without header and tag, or the compressed block itself */
    uint64_t src_len;
    void *dst;            /* the page                                         */
    uint64_t len;         /* page length = block size the key names (cached_store.go:938-942) */
    uint8_t *crc;         /* CRC_GEN: out, 4*max(1,ceil(len/32K)) bytes; unused with CRC_NONE */
    uint64_t out_len;     /* out: bytes the decoder produced (0 unless it ran) */
    int32_t status;       /* out                                              */
    int32_t codec_info;   /* out: zstd, why the serial decoder took it (as jfsx_zblk.reserved) */
} jfsx_lblk;
int jfsx_load_batch(jfsx_ctx *ctx, int algo, int codec, int n, jfsx_lblk *blks, int crc_mode, int mem);

/* One-call block store: the write side of a volume formatted with --compress
 * lz4 / zstd -- the staged re-read of --writeback (uploadStagingFile ->
 * cacheFile.ReadAt's CRC verify, pkg/chunk/cached_store.go:944-999) or
 * bcache.stage's checksum() of the page (:439; disk_cache.go:433-483),
 * cachedStore.upload's Compress (:371-413), store.put's Encrypt
 * (encrypt.go:164-194) and the object store's checksum of what is put
 * (pkg/object/checksum.go:31-53) -- for a batch of pages in one synchronous
 * call.  JFSX_MEM_HOST moves each page up once and each stored image down
 * once; the compressed bytes never leave device memory.  The call waits twice:
 * the Seal is planned from the compressed lengths, which come back first (a
 * few dozen bytes per block).
 *   algo      JFSX_AES256GCM, JFSX_CHACHA20P1305, or JFSX_CIPHER_NONE (dst
 *             receives the compressed block itself)
 *   codec     JFSX_CODEC_LZ4 or JFSX_CODEC_ZSTD (a volume with no codec is
 *             served by jfsx_seal_batch already: JFSX_CRC_BOTH gives both
 *             checksums)
 *   crc_mode  the low two bits are about the page: JFSX_CRC_NONE, JFSX_CRC_GEN
 *             (checksum(page) into crc, the direct upload of wSlice.upload) or
 *             JFSX_CRC_VERIFY (crc holds the staged file's CRCs).  JFSX_CRC_CT
 *             may be OR'ed in, or given alone: obj_crc receives the object
 *             checksum CRC32C(hdr || dst[0, out_len) || tag), the value
 *             jfsx_object_crc32c folds (without a cipher: CRC32C(hdr || image))
 *   mem       JFSX_MEM_HOST: pageable or pinned memory at any alignment; only
 *             dst[0, out_len) is written.  JFSX_MEM_DEVICE: src 16-byte aligned
 *             when the page CRC runs (GEN / VERIFY), dst 16-byte aligned when a
 *             cipher or JFSX_CRC_CT touches it, dst distinct from src, crc in
 *             device memory (hdr stays host memory)
 * Anything else is JFSX_EINVAL, and so are the limits of the separate calls
 * (len <= 0x7E000000 and the ciphers' own), reserved != 0, and dst_cap below
 * jfsx_lz4_bound(len) / jfsx_zstd_bound(len) -- all before anything runs.  The bytes are those of the separate calls: jfsx_lz4/zstd_compress_batch,
 * then jfsx_seal_batch on its output with the same key and nonce; tag, crc and
 * obj_crc likewise.  A block whose page fails JFSX_CRC_VERIFY gets JFSX_ECRC
 * with crc_bad_seg / crc_got / crc_expect as jfsx_blk reports them, out_len 0,
 * tag and obj_crc zero; neither the compressor nor the cipher is started on its
 * bytes, dst[0, dst_cap) is not written, and the other blocks of the batch are
 * unaffected.  jfsx_metrics counts what the separate calls would: crc_* over the
 * n pages (crc_fail for JFSX_ECRC), lz4c_* / zstdc_* and seal_* over the blocks
 * that passed the verify (seal_bytes = the sum of out_len), and the CRC launch
 * that JFSX_CRC_CT adds without a cipher as jfsx_crc32c_segments would. */
typedef struct jfsx_sblk {
    uint8_t key[32];      /* as jfsx_blk; ignored with JFSX_CIPHER_NONE           */
    uint8_t nonce[12];
    uint32_t reserved;    /* must be 0                                            */
    uint8_t tag[16];      /* out; zero with JFSX_CIPHER_NONE or a failed block    */
    const void *src;      /* the page                                             */
    uint64_t len;
    void *dst;            /* stored image: C (no header, no tag), or the compressed block */
    uint64_t dst_cap;     /* >= jfsx_lz4_bound(len) / jfsx_zstd_bound(len)        */
    uint8_t *crc;         /* GEN: out, VERIFY: in; 4*max(1,ceil(len/32K)) B; unused otherwise */
    const void *hdr;      /* JFSX_CRC_CT: object header bytes, HOST memory, nullable */
    uint32_t hdr_len;
    uint32_t obj_crc;     /* out with JFSX_CRC_CT: CRC32C(hdr || dst[0,out_len) || tag) */
    uint64_t out_len;     /* out: bytes of the stored image, 0 for a failed block */
    int32_t status;       /* out: JFSX_OK / JFSX_ECRC                             */
    int32_t crc_bad_seg;  /* out, as jfsx_blk (VERIFY)                            */
    uint32_t crc_got, crc_expect;
} jfsx_sblk;
int jfsx_store_batch(jfsx_ctx *ctx, int algo, int codec, int n, jfsx_sblk *blks, int crc_mode, int mem);

/* One-call object load: the whole read miss (cachedStore.load,
 * pkg/chunk/cached_store.go:673-748) from the stored object to the page -- the
 * object store's checksum verify (checksumReader, pkg/object/checksum.go:55-82),
 * dataEncryptor.Decrypt with its key unwrap (encrypt.go:196-216; rsaEncryptor
 * .Decrypt, :132-134), Decompress into the page (cached_store.go:738) and
 * bcache.cache's checksum() (disk_cache.go:433-483) -- for a batch of objects in
 * one synchronous call.  It is jfsx_load_batch with the two steps a reader ran
 * around it moved onto the device: the wrapped data keys go up once and the
 * unwrapped keys are handed from the RSA kernels to the AEAD key setup in
 * device memory (no unwrapped key is ever copied to the host, and neither the
 * call nor the record has an output that carries one), and the object checksum
 * is folded from the segment CRCs of the uploaded image before Open runs on it.
 * The call waits once.  A decoder is never started on bytes of a block that
 * failed its checksum, its header, its key unwrap or its tag.
 *   key       jfsx_rsa_key_new's key on ctx's device with a cipher; NULL with
 *             JFSX_CIPHER_NONE
 *   algo      JFSX_AES256GCM, JFSX_CHACHA20P1305, or JFSX_CIPHER_NONE (hdr_len
 *             must then be 0)
 *   codec     JFSX_CODEC_LZ4, JFSX_CODEC_ZSTD, or JFSX_CODEC_NONE for a volume
 *             without --compress: src_len == len, a cipher is required (with
 *             neither there is nothing but jfsx_crc32c_segments to run), and
 *             Open writes the page itself
 *   crc_mode  JFSX_CRC_NONE or JFSX_CRC_GEN for the page, with JFSX_CRC_CT
 *             OR'ed in or given alone: the object checksum CRC32C(hdr || src ||
 *             tag) -- without a cipher CRC32C(src) -- is computed into obj_crc
 *             and compared with expect_crc
 *   mem       as jfsx_load_batch; in addition, with JFSX_MEM_DEVICE, src is
 *             16-byte aligned when JFSX_CRC_CT reads it, and dst is 16-byte
 *             aligned with JFSX_CODEC_NONE (Open writes it).  hdr and tag are
 *             host memory in both modes.
 * Limits are those of jfsx_load_batch.  Any argument error is JFSX_EINVAL
 * before anything runs, with the records untouched: the above, reserved != 0,
 * hdr_len != 0 with a NULL hdr, a key of another device.
 * Per-block result, the first rule that applies (the order the reference
 * fails: checksum.go:55-70, encrypt.go:196-216, cached_store.go:738-743):
 *   1 JFSX_CRC_CT: obj_crc != expect_crc               JFSX_ECRC
 *   2 cipher: hdr_len < 3 or != 3 + klen + nlen        JFSX_EHEADER
 *   3 cipher: the unwrap fails (also klen == 0,        JFSX_EKEY, key_len -1
 *     klen > k, c >= n), or gives a message that       JFSX_EKEY, key_len = its length
 *     is not 32 bytes long
 *   4 cipher: nlen != 12, or the tag does not verify   JFSX_ETAG
 *   5 the decoder and length rows of jfsx_load_batch   JFSX_EFORMAT / JFSX_EDSTSIZE / JFSX_ESHORT
 * (k = jfsx_rsa_key_bytes(key), Go's len(ciphertext) > k check: an object
 * wrapped under a 2048-bit key and loaded with a 4096-bit one has klen = 256
 * <= k, is unwrapped as the number it is, and fails the OAEP check: rule 3.)
 * out_len is as in jfsx_load_batch (0 for rules 1-4).  On any status other than
 * JFSX_OK the page and the CRC array are all zero.  obj_crc is the computed
 * value whenever JFSX_CRC_CT is set.  key_len is what the unwrap returned for
 * the block (32 for a good one, -1 for the decryption error), and 0 where none
 * ran for it: JFSX_CIPHER_NONE, or a header that names no key (rule 2).
 * jfsx_metrics counts what the separate calls would: open_* over the blocks
 * that reached Open with their own key (rules 1-3 passed; open_fail: rule 4),
 * lz4d_* / zstdd_* over the blocks that reached the decoder (rules 1-4 passed),
 * crc_* over the n pages with JFSX_CRC_GEN and, with JFSX_CRC_CT, over the n
 * images as jfsx_crc32c_segments would (crc_fail: rule 1). */
#define JFSX_CODEC_NONE 0   /* jfsx_load_objects / jfsx_store_objects only: the volume has no --compress */
#define JFSX_EKEY    7      /* per-block: "decryt key: crypto/rsa: decryption error" (encrypt.go:207-210),
                               or an unwrapped key that is not 32 bytes (NewCipher's key size error) */
#define JFSX_EHEADER 8      /* per-block: "misformed ciphertext: %d %d" (encrypt.go:199-201) */
typedef struct jfsx_oblk {
    const void *hdr;      /* HOST memory, both mem modes: BE16(klen) | nlen | wrapped key | nonce */
    uint32_t hdr_len;     /* 0 with JFSX_CIPHER_NONE                          */
    uint32_t reserved;    /* must be 0                                        */
    uint8_t tag[16];      /* in: the object's last 16 bytes; ignored with JFSX_CIPHER_NONE */
    const void *src;      /* C: the object after the header, without the tag (or the stored block itself) */
    uint64_t src_len;
    void *dst;            /* the page                                         */
    uint64_t len;
    uint8_t *crc;         /* CRC_GEN: out, 4*max(1,ceil(len/32K)) bytes       */
    uint32_t expect_crc;  /* in with JFSX_CRC_CT: the store's checksum of hdr || src || tag */
    uint32_t obj_crc;     /* out with JFSX_CRC_CT: the value computed         */
    uint64_t out_len;     /* out                                              */
    int32_t status;       /* out                                              */
    int32_t codec_info;   /* out, as jfsx_lblk                                */
    int32_t key_len;      /* out: unwrapped key length, -1 decryption error, 0 when no unwrap ran */
    int32_t reserved2;
} jfsx_oblk;
int jfsx_load_objects(jfsx_ctx *ctx, const jfsx_rsa_key *key, int algo, int codec, int n,
                      jfsx_oblk *blks, int crc_mode, int mem);

/* One-call object store: the write side of jfsx_load_objects -- from the page
 * to the stored object that store.put hands to the object store
 * (dataEncryptor.Encrypt, pkg/object/encrypt.go:164-194):
 *   BE16(k) | 12 | wrapped key (k) | nonce (12) | C | tag (16)
 * (k = jfsx_rsa_key_bytes(key): 256, or 512 with a 4096-bit key)
 * for a batch of pages in one synchronous call: the page's verify or
 * checksum(), rsaEncryptor.Encrypt of the data key (encrypt.go:169), Compress,
 * Seal, the header and tag around C, and the object store's checksum of all of
 * it (checksum.go:31-53).  The wrapped key and the tag never leave device
 * memory on their own: the object comes down whole, and obj_crc is folded on
 * the device.  The data key goes up once.
 *   key, e    as jfsx_rsa_oaep_encrypt_batch: the key lives on ctx's device, e
 *             is in Go's checkPub range
 *   algo      JFSX_AES256GCM or JFSX_CHACHA20P1305 (without a cipher the object
 *             is the image: jfsx_store_batch)
 *   codec     JFSX_CODEC_NONE (C is the sealed page, img_len == len),
 *             JFSX_CODEC_LZ4 or JFSX_CODEC_ZSTD
 *   crc_mode  as jfsx_store_batch: NONE / GEN / VERIFY for the page, with
 *             JFSX_CRC_CT OR'ed in or given alone for obj_crc
 *   mem       JFSX_MEM_HOST: pageable or pinned memory at any alignment; only
 *             obj[0, out_len) is written.  JFSX_MEM_DEVICE: (uintptr_t)obj % 16
 *             == 1, so that C at obj + 15 + k is 16-byte aligned (15 + k is
 *             15 mod 16 for k = 256 and for k = 512: one rule for both key
 *             sizes) and the wrapped key at obj + 3 and the nonce at obj + 3
 *             + k are dword aligned; src
 *             16-byte aligned when a page CRC or the Seal reads it (GEN /
 *             VERIFY, or JFSX_CODEC_NONE); obj distinct from src; crc in device
 *             memory
 * JFSX_EINVAL before anything runs, with the records untouched: anything else,
 * the limits of the separate calls, reserved != 0, obj_cap below
 * jfsx_object_bound_key(key, codec, len), a NULL crc with GEN / VERIFY, a NULL key, a
 * key of another device, e out of range.  The bytes are those of the separate
 * calls: jfsx_rsa_oaep_encrypt_batch on key and seed, the compressor, then
 * jfsx_seal_batch with key and nonce.  A page that fails JFSX_CRC_VERIFY gets
 * JFSX_ECRC with crc_bad_seg / crc_got / crc_expect as jfsx_blk fills them and
 * out_len, img_len and obj_crc 0; neither the compressor nor the cipher is
 * started on its bytes, obj[0, obj_cap) is not written, and the other blocks
 * are unaffected.  The call waits once with JFSX_CODEC_NONE unless the pages
 * are verified, else twice, as jfsx_store_batch.  jfsx_metrics counts crc_*
 * over the n pages (GEN / VERIFY), lz4c_* / zstdc_* and seal_* over the blocks
 * that passed the verify (seal_bytes = the sum of img_len). */
/* the header of an RSA-2048 volume's object; with another key it is 15 +
 * jfsx_rsa_key_bytes(key) (527 at 4096 bits) */
#define JFSX_OBJ_HDR_BYTES 271 /* BE16(256) | 12 | 256-byte wrapped key | 12-byte nonce */
#define JFSX_OBJ_TAG_BYTES 16
/* 271 + (len | jfsx_lz4_bound(len) | jfsx_zstd_bound(len)) + 16; 0 for an unknown
 * codec.  An RSA-2048 volume's bound: it is too small for a 4096-bit key, and
 * jfsx_store_objects answers it with JFSX_EINVAL there. */
uint64_t jfsx_object_bound(int codec, uint64_t len);
/* the same for key: (15 + k) + image bound + 16; 0 for a NULL key or an unknown codec */
uint64_t jfsx_object_bound_key(const jfsx_rsa_key *key, int codec, uint64_t len);
typedef struct jfsx_soblk {
    uint8_t key[32];      /* data key: the caller's randomness (encrypt.go:165) */
    uint8_t nonce[12];    /* encrypt.go:177                                     */
    uint32_t reserved;    /* must be 0                                          */
    uint8_t seed[32];     /* OAEP seed, as jfsx_rsa_oaep_encrypt_batch takes it */
    const void *src;      /* the page                                           */
    uint64_t len;
    void *obj;            /* out: header | C | tag, contiguous                  */
    uint64_t obj_cap;     /* >= jfsx_object_bound_key(key, codec, len)          */
    uint8_t *crc;         /* page CRCs. GEN: out, VERIFY: in; unused otherwise  */
    uint64_t out_len;     /* out: bytes of the object, 0 for a failed block     */
    uint64_t img_len;     /* out: bytes of C                                    */
    uint32_t obj_crc;     /* out with JFSX_CRC_CT: CRC32C of obj[0, out_len)    */
    int32_t status;       /* out: JFSX_OK / JFSX_ECRC                           */
    int32_t crc_bad_seg;  /* out, as jfsx_sblk                                  */
    uint32_t crc_got, crc_expect;
    uint32_t reserved2;
} jfsx_soblk;
int jfsx_store_objects(jfsx_ctx *ctx, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n,
                       jfsx_soblk *blks, int crc_mode, int mem);

/* One-call slice compaction (vfs.Compact, pkg/vfs/compact.go:54-109): the live
 * ranges of a chunk's old slices are read block by block (readSlice,
 * rSlice.ReadAt, pkg/chunk/cached_store.go:96-190) and written, with zeros for
 * holes (Id == 0), as one new slice that wSlice.upload cuts into blocks,
 * compresses and encrypts.  Three entry points, from the inside out.
 *
 * jfsx_compact_plan -- host only, no device: from the slice list, in the order
 * Compact receives it (meta.Slice, pkg/meta/interface.go:250-255), to the work.
 *   srcs     one entry per distinct stored block that some slice reads, in
 *            order of first use: indx = p / block_size, bsize = min(block_size,
 *            size - indx * block_size) (rSlice.blockSize, cached_store.go:65-71);
 *            the caller forms the key chunks/{id/1e6}/{id/1e3}/{id}_{indx}_{bsize}
 *            (:73-78).  A block that two records of one id touch appears once.
 *   pages    the new slice of sum(len) bytes cut into pages of block_size, the
 *            last one shorter: its run of pieces, and page_len[j] its bytes
 *   pieces   consecutive in their page; src indexes srcs, -1 means zeros.  A
 *            piece crosses neither a source block nor a page boundary, and two
 *            neighbours of one page that continue each other (the same source
 *            at contiguous src_off, or both holes) are merged.
 * Two-call sizing: n_src, n_page and n_piece are always written; when any
 * capacity is too small the arrays stay untouched and the call returns
 * JFSX_ENOMEM.  JFSX_ENOMEM with nothing written: a plan that cannot be held
 * (a count beyond 2^31 - 1, as a tiny block_size under a total near 2^32
 * gives, or memory for it that the host does not have).  JFSX_EINVAL: block_size == 0, n < 0, a NULL count, reserved !=
 * 0, len == 0, off + len > size with id != 0, a total beyond 2^32 - 1. */
#define JFSX_ESRC 9   /* per-page: a source block of the page did not load ("can't compact ... retry later",
                         compact.go:83) */
typedef struct jfsx_slice {
    uint64_t id;          /* 0: a hole of len bytes */
    uint32_t size, off, len;
    uint32_t reserved;    /* must be 0 */
} jfsx_slice;
typedef struct jfsx_csrc {
    uint64_t id;
    uint32_t indx, bsize;
} jfsx_csrc;
typedef struct jfsx_cpage {
    uint32_t piece_first, piece_count;
    int32_t src_bad;      /* out of jfsx_compact_objects: the failed source of a JFSX_ESRC page, else -1 */
    uint32_t reserved;    /* must be 0 */
} jfsx_cpage;
typedef struct jfsx_piece {
    int32_t src;          /* index of the source, -1: zeros */
    uint32_t reserved;    /* must be 0 */
    uint64_t src_off;     /* ignored for a hole */
    uint64_t len;         /* > 0 */
} jfsx_piece;
int jfsx_compact_plan(uint32_t block_size, int n, const jfsx_slice *slices, int src_cap, jfsx_csrc *srcs, int *n_src,
                      int page_cap, jfsx_cpage *pages, uint64_t *page_len, int *n_page, int piece_cap,
                      jfsx_piece *pieces, int *n_piece);

/* jfsx_gather_batch -- the pages assembled by one kernel launch (gather_pages_k,
 * jfsx_gather.hip).  Every byte of dst[j].data[0, len) is written exactly once:
 * a data piece writes src[piece.src].data[src_off, src_off + len), a hole piece
 * zeros; no memset runs in front and nothing outside a destination is written.
 * Loads are confined to the naturally aligned 16-byte chunks that overlap a
 * piece's source bytes.
 *   JFSX_MEM_DEVICE  src[i].data and dst[j].data are 16-byte aligned; lengths,
 *                    src_off and piece boundaries are arbitrary; no destination
 *                    overlaps a source or another destination
 *   JFSX_MEM_HOST    any alignment; staged as the other calls stage: pageable
 *                    buffers through one pinned bounce buffer, packed, one
 *                    copy up and one down; engine-pinned buffers where they lie
 * JFSX_EINVAL before anything runs, with the records untouched: a piece index
 * outside [-1, n_src), src_off + len > src.len, a piece of len 0, reserved !=
 * 0, a sum of piece lengths that is not dst.len, a piece range outside
 * n_piece, a NULL data with len > 0, a broken alignment or overlap rule.  A
 * destination of len 0 without pieces writes nothing; two pieces may read the
 * same source bytes. */
typedef struct jfsx_gsrc {
    const void *data;
    uint64_t len;
} jfsx_gsrc;
typedef struct jfsx_gdst {
    void *data;
    uint64_t len;
    uint32_t piece_first, piece_count;
} jfsx_gdst;
int jfsx_gather_batch(jfsx_ctx *ctx, int n_src, const jfsx_gsrc *src, int n_dst, jfsx_gdst *dst, int n_piece,
                      const jfsx_piece *pieces, int mem);

/* jfsx_compact_objects -- stored objects in, stored objects out, host memory on
 * both sides; the pages live and die in device memory.  Under the context's
 * lock, on its stream:
 *   1 load    the images go up and jfsx_load_objects' chain runs into
 *             engine-owned device pages; the call waits for the source verdicts
 *   2 gate    a page is good when every source its pieces name came back
 *             JFSX_OK with out_len == len.  Any other page gets JFSX_ESRC,
 *             pages[j].src_bad = the source of its first piece that failed,
 *             out_len, img_len and obj_crc 0; neither the compressor nor the
 *             cipher nor the key wrap's result touches its bytes and obj[0,
 *             obj_cap) is not written.  Good pages have src_bad = -1.
 *   3 gather  one launch over the good pages
 *   4 store   jfsx_store_objects' chain from the device pages into the engine's
 *             packed objects, then out_len bytes per object come down
 * src[i] is a jfsx_oblk as jfsx_load_objects takes it with JFSX_MEM_HOST (hdr,
 * tag, src, src_len, expect_crc; len = the page length its key names) with dst
 * and crc NULL; it gets status, out_len, codec_info, key_len and obj_crc as
 * that call reports them.  dst[j] is a jfsx_soblk as jfsx_store_objects takes
 * it (key, nonce, seed, obj, obj_cap, crc; len = the page length) with src
 * NULL; it gets what that call reports.  The bytes are those of the separate
 * calls with the same keys, nonces and seeds.
 *   src_crc_mode  0 or JFSX_CRC_CT
 *   dst_crc_mode  JFSX_CRC_NONE or JFSX_CRC_GEN, JFSX_CRC_CT optional
 *   algo          JFSX_AES256GCM or JFSX_CHACHA20P1305
 *   codec         JFSX_CODEC_NONE, JFSX_CODEC_LZ4 or JFSX_CODEC_ZSTD
 * Argument errors (JFSX_EINVAL before the context or its device is touched, the
 * records unchanged): those of the two calls for host memory, the gather's
 * piece rules with src[i].len and dst[j].len as the lengths, pages[j].reserved
 * != 0, a non-NULL dst / crc of a source or src of a destination.  Returns 0
 * when blocks or pages failed.  jfsx_metrics counts what the separate calls
 * count: jfsx_load_objects over the n_src sources and jfsx_store_objects over
 * the good pages. */
int jfsx_compact_objects(jfsx_ctx *ctx, const jfsx_rsa_key *key, uint32_t e, int algo, int codec, int n_src,
                         jfsx_oblk *src, int src_crc_mode, int n_dst, jfsx_soblk *dst, jfsx_cpage *pages,
                         int dst_crc_mode, int n_piece, const jfsx_piece *pieces);

/* header helper: returns wrapped-key length and offset/size of the nonce so a
 * caller can unwrap the key first (encrypt.go:197-205) */
int jfsx_parse_header(const void *obj, uint64_t olen, int *klen, int *nlen);

/* synthetic input generator used by bench/tests: fills len bytes of device
 * memory with the SplitMix64 stream of (seed, block) (documented in
 * DESIGN.md; identical to oracle/jfs_oracle.c:orc_gen_block) */
int jfsx_gen_synthetic(jfsx_ctx *ctx, void *dst, uint64_t len, uint64_t seed, uint64_t block);
/* batched form: block i (global index block0 + i) is written at
 * dst + i*stride with lens[i] bytes (lens: host array), one launch for the
 * whole batch */
int jfsx_gen_synthetic_batch(jfsx_ctx *ctx, void *dst, uint64_t stride, int n, const uint64_t *lens, uint64_t seed,
                             uint64_t block0);
/* fills n keys (32 B) and nonces (12 B) with the same per-block stream as
 * orc_gen_key, host side */
void jfsx_gen_key(uint64_t seed, uint64_t block, uint8_t key[32], uint8_t nonce[12]);

/* PCIe probe on the streams the host-ingest ring uses (H2D stream, D2H
 * stream): `bytes` between engine-pinned host memory and device memory in
 * 8 chunks per direction, best of 3; out[0] H2D alone, out[1] D2H alone,
 * out[2] / out[3] H2D / D2H rate while both directions run at once (chunks
 * issued alternately, as the ring issues them), in GB/s.  The ring moves equal
 * bytes up and down, so min(out[2], out[3]) bounds a host-ingest seal. */
int jfsx_pcie_probe(jfsx_ctx *ctx, uint64_t bytes, double out[4]);

/* diagnostics: the lookup tables the kernels stage into LDS, built on the host
 * without a device (AES T0|T2 x32 replicated: 16384 dwords; CRC32C slice-by-16
 * and 1008/4032/1024/4096-byte shift tables: 8192 dwords; CRC lane/power constants: 192) */
int jfsx_debug_tables(uint32_t *aes, uint32_t *crc, uint32_t *crcx);

#ifdef __cplusplus
}
#endif
#endif /* JFSX_H */
