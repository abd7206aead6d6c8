"""Mirror of pkg/compress/compress.go on the GPU engine, and the compress /
decompress steps of the chunk store's block upload and load.

  Compressor interface {Name, CompressBound, Compress, Decompress}  compress.go:30-36
  NewCompressor("lz4" | "zstd" | "none" | "")                       compress.go:38-50
  noOp (copy; "buffer too short: %d < %d")                         compress.go:52-70
  LZ4 (lz4.CompressDefault / lz4.DecompressSafe;
       "decompress an empty input")                                compress.go:104-125
  ZStandard.Compress (zstd.CompressLevel(dst, src, 1))             compress.go:82-91
  ZStandard.Decompress (zstd.Decompress; "buffer too short")       compress.go:93-102
  upload_block: CompressBound buffer, Compress, then Put           cached_store.go:371-392
  load_block: Get, Decompress into the block, "read %s fully"      cached_store.go:673-745

The LZ4 block codec runs on the HIP engine (jfsx_lz4_compress_batch /
jfsx_lz4_decompress_batch, jfsx_lz4.hip), bit-exact to the LZ4 C library the
reference binds; CompressBatch / DecompressBatch are the batched entry points
(one engine call per batch).  Zstandard runs on the engine both ways:
jfsx_zstd_compress_batch (jfsx_zstdc.hip) writes the zstd library's level-1
frames byte for byte, jfsx_zstd_decompress_batch (jfsx_zstd.hip) decodes as
ZSTD_decompress.  load_blocks_fused is load_block as one engine call
(jfsx_load_batch: Decrypt, Decompress and the cache's checksum() chained in
device memory), upload_blocks_fused is upload_block the same way
(jfsx_store_batch: checksum(), Compress, Encrypt and the object checksum).
"""
from . import engine as E
from .encrypt import default_engine


class CompressError(Exception):
    pass


class noOp:
    def Name(self):
        return "Noop"

    def CompressBound(self, n):
        return n

    def Compress(self, dst, src):
        if len(dst) < len(src):
            raise CompressError("buffer too short: %d < %d" % (len(dst), len(src)))
        dst[:len(src)] = src
        return len(src)

    def Decompress(self, dst, src):
        if len(dst) < len(src):
            raise CompressError("buffer too short: %d < %d" % (len(dst), len(src)))
        dst[:len(src)] = src
        return len(src)


class LZ4:
    """The "lz4" compressor.  Compress/Decompress follow Go's (dst, src) ->
    (n, error) shape: they return n and raise CompressError for the error."""

    def __init__(self, eng=None):
        self._eng = eng

    @property
    def eng(self):
        return self._eng or default_engine()

    def Name(self):
        return "LZ4"

    def CompressBound(self, n):
        return int(E.lz4_bound(n))

    def Compress(self, dst, src):
        out = self.CompressBatch([src])[0]
        if len(dst) < len(out):
            raise CompressError("buffer too short: %d < %d" % (len(dst), len(out)))
        dst[:len(out)] = out
        return len(out)

    def Decompress(self, dst, src):
        if len(src) == 0:
            raise CompressError("decompress an empty input")
        (st, out), = self.eng.lz4_decompress([src], [len(dst)])
        if st != E.OK:
            raise CompressError("lz4: malformed block")
        dst[:len(out)] = out
        return len(out)

    # -- batched: one GPU call for many blocks -----------------------------
    def CompressBatch(self, blocks):
        """blocks -> compressed bytes per block (LZ4_compress_default)."""
        return self.eng.lz4_compress(blocks)

    def DecompressBatch(self, blobs, sizes):
        """(compressed blob, destination size) per block -> decoded bytes,
        or a CompressError instance for a block that does not decode."""
        out = []
        todo = [i for i, b in enumerate(blobs) if len(b)]
        res = dict(zip(todo, self.eng.lz4_decompress([blobs[i] for i in todo], [sizes[i] for i in todo])))
        for i in range(len(blobs)):
            if i not in res:
                out.append(CompressError("decompress an empty input"))
            else:
                st, d = res[i]
                out.append(d if st == E.OK else CompressError("lz4: malformed block"))
        return out


class ZStandard:
    """The "zstd" compressor (DataDog/zstd v1.5.0, level 1): Compress and
    Decompress both run on the engine.  jfsx_zstd_compress_batch is bit-exact
    to the system libzstd 1.4.8's ZSTD_compress(level 1); byte parity with the
    v1.5.0 library the reference links is unpinned (its vendored C is not in
    the reference tree), but every frame is valid zstd and reads back through
    this Decompress and through libzstd's ZSTD_decompress alike.
    jfsx_zstd_decompress_batch decodes as ZSTD_decompress."""

    def __init__(self, level=1, eng=None):
        if level != 1:
            raise ValueError("the engine implements zstd level 1 (compress.go:28 ZSTD_LEVEL)")
        self.level = level
        self._eng = eng

    @property
    def eng(self):
        return self._eng or default_engine()

    def Name(self):
        return "Zstd"

    def CompressBound(self, n):
        return int(E.zstd_bound(n))  # ZSTD_COMPRESSBOUND(n)

    def Compress(self, dst, src):
        """compress.go:82-91: zstd.CompressLevel allocates a new buffer when
        cap(dst) < CompressBound(len(src)), and Compress reports that as
        "buffer too short: %d < %d" (cap(dst), cap(d))."""
        bound = self.CompressBound(len(src))
        if len(dst) < bound:
            raise CompressError("buffer too short: %d < %d" % (len(dst), bound))
        out = self.CompressBatch([src])[0]
        dst[:len(out)] = out
        return len(out)

    def Decompress(self, dst, src):
        d = self.DecompressBatch([src], [len(dst)])[0]
        if isinstance(d, Exception):
            raise d
        dst[:len(d)] = d
        return len(d)

    # -- batched: one GPU call for many blocks -----------------------------
    def CompressBatch(self, blocks):
        """blocks -> one level-1 frame per block (ZSTD_compress(level 1))."""
        return self.eng.zstd_compress(blocks)

    def DecompressBatch(self, blobs, sizes):
        """(frames, destination size) per block -> decoded bytes, or a
        CompressError:
          * an empty input: DataDog's ErrEmptySlice ("Bytes slice is empty");
          * frames that decode, but not into the destination: zstd.Decompress
            returns a larger buffer, which compress.go:98-100 reports as
            "buffer too short: %d < %d" (len(dst), decoded size);
          * anything else the decoder rejects: "zstd: corrupted frame"."""
        out = [None] * len(blobs)
        todo = []
        for i, b in enumerate(blobs):
            if len(b) == 0:
                out[i] = CompressError("Bytes slice is empty")
            else:
                todo.append(i)
        res = self.eng.zstd_decompress([blobs[i] for i in todo], [sizes[i] for i in todo]) if todo else []
        short = []
        for i, (st, d) in zip(todo, res):
            if st == E.OK:
                out[i] = d
            elif st == E.EDSTSIZE:
                short.append(i)
            else:
                out[i] = CompressError("zstd: corrupted frame")
        # the decoded size of a frame that does not fit: its content size
        # field when it has one, else doubling capacities (up to 2^31 - 1)
        caps = {i: max(_frame_content_size(blobs[i]) or 0, 2 * sizes[i], 1 << 16) for i in short}
        while short:
            res = self.eng.zstd_decompress([blobs[i] for i in short], [min(caps[i], (1 << 31) - 1) for i in short])
            again = []
            for i, (st, d) in zip(short, res):
                if st == E.OK:
                    out[i] = CompressError("buffer too short: %d < %d" % (sizes[i], len(d)))
                elif st == E.EDSTSIZE and caps[i] < (1 << 31) - 1:
                    caps[i] *= 2
                    again.append(i)
                else:
                    out[i] = CompressError("zstd: corrupted frame")
            short = again
        return out


def _frame_content_size(b):
    """Frame_Content_Size of the first frame's header (RFC 8878 3.1.1.1), or
    None when absent or unreadable."""
    b = bytes(b[:18])
    if len(b) < 6 or b[:4] != b"\x28\xb5\x2f\xfd":
        return None
    fhd = b[4]
    single, fcs_id, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    pos = 5 + (0 if single else 1) + (0, 1, 2, 4)[did]
    size = (1 if single else 0, 2, 4, 8)[fcs_id]
    if size == 0 or len(b) < pos + size:
        return None
    v = int.from_bytes(b[pos:pos + size], "little")
    return v + 256 if size == 2 else v


def NewCompressor(algr, eng=None):
    """compress.go:38-50: None for an unknown name."""
    algr = algr.lower()
    if algr == "zstd":
        return ZStandard(1, eng)
    if algr == "lz4":
        return LZ4(eng)
    if algr in ("none", ""):
        return noOp()
    return None


# ---------------------------------------------------------------------------
# chunk-store steps around the codec (cached_store.go)
# ---------------------------------------------------------------------------
def upload_blocks(store, keys, blocks, compressor):
    """cachedStore.upload for a batch of blocks: compress each (into a
    CompressBound-sized buffer when the bound exceeds the block), then Put."""
    if isinstance(compressor, (LZ4, ZStandard)):
        outs = compressor.CompressBatch(blocks)
    else:
        outs = []
        for b in blocks:
            buf = bytearray(max(compressor.CompressBound(len(b)), len(b)))
            n = compressor.Compress(buf, bytes(b))
            outs.append(bytes(buf[:n]))
    for k, o in zip(keys, outs):
        store.Put(k, o)
    return outs


def load_blocks(store, keys, lengths, compressor):
    """cachedStore.load for a batch: Get each object, decompress into a page of
    the block's length; a short result is "read %s fully: %s (%d < %d)"."""
    objs = [store.Get(k, 0, -1) for k in keys]
    compressed = [compressor.CompressBound(n) > n for n in lengths]
    if isinstance(compressor, (LZ4, ZStandard)):
        dec = compressor.DecompressBatch(objs, lengths)
    else:
        dec = []
        for o, n in zip(objs, lengths):
            page = bytearray(n)
            try:
                m = compressor.Decompress(page, o)
                dec.append(bytes(page[:m]))
            except CompressError as e:
                dec.append(e)
    out = []
    for k, o, n, c, d in zip(keys, objs, lengths, compressed, dec):
        if not c:
            d = o[:n]
        if isinstance(d, Exception):
            raise CompressError("read %s fully: %s (%d < %d)" % (k, d, 0, n))
        if len(d) < n:
            raise CompressError("read %s fully: %s (%d < %d)" % (k, None, len(d), n))
        out.append(d)
    return out


def load_blocks_fused(store, keys, lengths, compressor, enc=None, checksums=True):
    """cachedStore.load for a batch in one engine call (jfsx_load_batch): the
    raw objects of `store` are opened (with enc, a DataEncryptor: header parse
    and batched key unwrap on the way), decompressed into pages of the blocks'
    lengths and checksummed without leaving the device in between
    (cached_store.go:673-748; bcache.cache's checksum(), disk_cache.go:433-483).

    Returns what load_blocks(NewEncrypted(store, enc) or store, ...) returns,
    and raises what it raises: a decrypt failure of any object first
    ("Decrypt: ..." as Encrypted.Get wraps DataEncryptor.Decrypt's error), then,
    in key order, "read %s fully: %s (%d < %d)".  With checksums=True the result
    is (pages, crcs): crcs[i] is checksum(pages[i]), the trailer write_cache_file
    appends."""
    from .encrypt import _ERR_OPEN, EncryptError
    if not isinstance(compressor, (LZ4, ZStandard)):
        raise ValueError("load_blocks_fused needs the lz4 or zstd compressor (an uncompressed volume loads "
                         "through DataEncryptor.DecryptBatch)")
    lz4 = isinstance(compressor, LZ4)
    empty = "decompress an empty input" if lz4 else "Bytes slice is empty"
    eng = compressor.eng
    objs = [store.Get(k, 0, -1) for k in keys]
    lengths = [int(n) for n in lengths]
    dec_err = [None] * len(keys)  # per block: the error Decrypt would return
    items = [None] * len(keys)
    if enc is None:
        algo = E.CIPHER_NONE
        for k, o, n in zip(keys, objs, lengths):
            if len(o) == 0:  # LZ4.Decompress / zstd.Decompress reject it before the codec runs
                raise CompressError("read %s fully: %s (%d < %d)" % (k, empty, 0, n))
        items = list(objs)
    else:
        algo = enc.algo
        parsed = []
        for i, c in enumerate(objs):
            c = bytes(c)
            if len(c) < 3:
                dec_err[i] = "misformed ciphertext: 0 0"
                continue
            keyLen, nonceLen = (c[0] << 8) + c[1], c[2]
            if 3 + keyLen + nonceLen >= len(c):
                dec_err[i] = "misformed ciphertext: %d %d" % (keyLen, nonceLen)
                continue
            parsed.append((i, c, keyLen, nonceLen))
        wrapped = [c[3:3 + kl] for _, c, kl, _ in parsed]
        if hasattr(enc.keyEncryptor, "DecryptBatch"):
            dkeys = enc.keyEncryptor.DecryptBatch(wrapped, eng)
        else:
            dkeys = []
            for w in wrapped:
                try:
                    dkeys.append(enc.keyEncryptor.Decrypt(w))
                except Exception as e:
                    dkeys.append(e)
        for (i, c, keyLen, nonceLen), key in zip(parsed, dkeys):
            nonce, ct = c[3 + keyLen:3 + keyLen + nonceLen], c[3 + keyLen + nonceLen:]
            if isinstance(key, Exception):
                dec_err[i] = "decryt key: " + str(key)
            elif len(key) != enc.keyLen:
                dec_err[i] = "crypto/aes: invalid key size %d" % len(key)
            elif nonceLen != 12 or len(ct) < 16:
                dec_err[i] = _ERR_OPEN[algo]
            else:
                items[i] = (key, nonce, ct[:-16], ct[-16:])
    for e in dec_err:
        if e is not None:
            raise EncryptError("Decrypt: %s" % e)
    res = eng.load(algo, E.CODEC_LZ4 if lz4 else E.CODEC_ZSTD, items, lengths, crc=checksums)
    info = eng.load_info
    for st, _, _ in res:
        if st == E.ETAG:
            raise EncryptError("Decrypt: %s" % _ERR_OPEN[algo])
    pages, crcs = [], []
    for i, (k, n, (st, page, crc)) in enumerate(zip(keys, lengths, res)):
        if enc is not None and len(items[i][2]) == 0:
            raise CompressError("read %s fully: %s (%d < %d)" % (k, empty, 0, n))
        if st == E.EDSTSIZE:
            # the text names the decoded size: decode this object alone into a
            # buffer that holds it, as ZStandard.DecompressBatch does
            blob = objs[i] if enc is None else enc.Decrypt(objs[i])
            d = compressor.DecompressBatch([blob], [n])[0]
            raise CompressError("read %s fully: %s (%d < %d)" % (k, d, 0, n))
        if st == E.EFORMAT:
            raise CompressError("read %s fully: %s (%d < %d)"
                                % (k, "lz4: malformed block" if lz4 else "zstd: corrupted frame", 0, n))
        if st == E.ESHORT:
            raise CompressError("read %s fully: %s (%d < %d)" % (k, None, info[i][0], n))
        pages.append(page)
        crcs.append(crc)
    return (pages, crcs) if checksums else pages


def load_objects_fused(store, keys, lengths, compressor, enc, checksums=True, object_checksums=None):
    """cachedStore.load for a batch in one engine call that starts at the stored
    object (jfsx_load_objects): the object store's checksum verify
    (checksumReader, checksum.go:55-82; object_checksums[i] is the decimal
    string the store kept for keys[i], or None), the header parse and the
    data-key unwrap, Open, Decompress and checksum() run back to back on the
    device, and no unwrapped data key comes back to the host.  enc is the
    volume's DataEncryptor, or None for a volume without one; compressor may be
    the "none" compressor when enc is given.

    Returns what load_blocks_fused returns and raises what it raises, in its
    order: first, in key order, a checksum mismatch (ChecksumVerifyError, the
    store's read error, which precedes Decrypt); then a decrypt failure of any
    object; then, in key order, "read %s fully: %s (%d < %d)".  Without a codec
    that is what load_blocks(NewEncrypted(store, enc), ...) gives.  An RSA key
    the engine does not take (not RSA-2048 with CRT parameters) goes through
    load_blocks_fused / DataEncryptor.DecryptBatch instead."""
    from .checksum import ChecksumVerifyError, parse_checksum
    from .encrypt import _ERR_OPEN, EncryptError
    coded = isinstance(compressor, (LZ4, ZStandard))
    if enc is None and not coded:
        raise ValueError("load_objects_fused needs a cipher or the lz4 / zstd compressor")
    lz4 = isinstance(compressor, LZ4)
    codec = E.CODEC_NONE if not coded else E.CODEC_LZ4 if lz4 else E.CODEC_ZSTD
    empty = "decompress an empty input" if lz4 else "Bytes slice is empty"
    eng = compressor.eng if coded else enc.eng
    keys, lengths = list(keys), [int(n) for n in lengths]
    objs = [bytes(store.Get(k, 0, -1)) for k in keys]
    want = [parse_checksum(object_checksums[i]) if object_checksums is not None else None for i in range(len(keys))]
    verify = any(w is not None for w in want)
    dk = None
    if enc is not None:
        dk = enc.keyEncryptor._device_key(eng) if hasattr(enc.keyEncryptor, "_device_key") else None
        if dk is None:  # the engine refuses the key: unwrap on the host, as before
            for o, w in zip(objs, want):
                if w is not None and E.crc32c_update(0, o) != w:
                    raise ChecksumVerifyError(E.crc32c_update(0, o), w)
            if coded:
                return load_blocks_fused(store, keys, lengths, compressor, enc=enc, checksums=checksums)
            pages = []
            for k, n, r in zip(keys, lengths, enc.DecryptBatch(objs)):
                if isinstance(r, Exception):
                    raise EncryptError("Decrypt: %s" % r)
                if len(r) < n:
                    raise CompressError("read %s fully: %s (%d < %d)" % (k, None, len(r), n))
                pages.append(r[:n])
            return (pages, [eng.checksum(p) for p in pages]) if checksums else pages
    algo = E.CIPHER_NONE if enc is None else enc.algo
    # what the host decides before the call: objects too short to cut into
    # header, C and tag (encrypt.go:199-201, and Open's length check)
    early = [None] * len(keys)
    items, plen = [None] * len(keys), list(lengths)
    for i, (o, n) in enumerate(zip(objs, lengths)):
        if enc is None:
            items[i] = o
            continue
        keyLen, nonceLen = ((o[0] << 8) + o[1], o[2]) if len(o) >= 3 else (0, 0)
        h = 3 + keyLen + nonceLen
        if len(o) < 3 or h >= len(o):
            early[i] = "misformed ciphertext: %d %d" % (keyLen, nonceLen)
        elif len(o) - h < 16:
            early[i] = _ERR_OPEN[algo]  # runs after the unwrap in the reference; see below
        else:
            items[i] = (o[:h], o[h:-16], o[-16:])
            if not coded:
                plen[i] = len(o) - h - 16  # Open's output is the page; cut to the block's length below
    run = [i for i in range(len(keys)) if early[i] is None and not (enc is None and len(objs[i]) == 0)]
    res = [None] * len(keys)
    info = [None] * len(keys)
    if run:
        # the verify is batch-wide: an object the store kept no checksum for is given its own
        expect = [want[i] if want[i] is not None else E.crc32c_update(0, objs[i]) for i in run] if verify else None
        got = eng.load_objects(dk, algo, codec, [items[i] for i in run], [plen[i] for i in run], crc=checksums,
                               expect=expect)
        for j, i in enumerate(run):
            res[i], info[i] = got[j], eng.load_info[j]
    # 1. the store's read: checksum mismatches, in key order
    for i, o in enumerate(objs):
        if want[i] is None:
            continue
        crc = info[i][3] if res[i] is not None else E.crc32c_update(0, o)
        if crc != want[i]:
            raise ChecksumVerifyError(crc, want[i])
    # 2. Decrypt's failures before Open (header, key), then Open's
    for i in range(len(keys)):
        if early[i] is not None and early[i] != _ERR_OPEN[algo]:
            raise EncryptError("Decrypt: %s" % early[i])
        if res[i] is not None and res[i][0] == E.EHEADER:
            o = objs[i]
            raise EncryptError("Decrypt: misformed ciphertext: %d %d" % ((o[0] << 8) + o[1], o[2]))
        if res[i] is not None and res[i][0] == E.EKEY:
            kl = info[i][2]
            raise EncryptError("Decrypt: %s" % ("decryt key: crypto/rsa: decryption error" if kl < 0
                                                else "crypto/aes: invalid key size %d" % kl))
    for i in range(len(keys)):
        if early[i] is not None or (res[i] is not None and res[i][0] == E.ETAG):
            raise EncryptError("Decrypt: %s" % _ERR_OPEN[algo])
    # 3. Decompress and the length check, in key order
    pages, crcs = [], []
    for i, (k, n) in enumerate(zip(keys, lengths)):
        if res[i] is None or (coded and enc is not None and len(items[i][1]) == 0):
            raise CompressError("read %s fully: %s (%d < %d)" % (k, empty, 0, n))
        st, page, crc = res[i]
        if st == E.EDSTSIZE:
            d = compressor.DecompressBatch([objs[i] if enc is None else enc.Decrypt(objs[i])], [n])[0]
            raise CompressError("read %s fully: %s (%d < %d)" % (k, d, 0, n))
        if st == E.EFORMAT:
            raise CompressError("read %s fully: %s (%d < %d)"
                                % (k, "lz4: malformed block" if lz4 else "zstd: corrupted frame", 0, n))
        if st == E.ESHORT or len(page) < n:
            raise CompressError("read %s fully: %s (%d < %d)" % (k, None, info[i][0] if coded else len(page), n))
        if len(page) > n:  # no codec: the object holds more than the block's length
            page = page[:n]
            crc = eng.checksum(page) if checksums else None
        pages.append(page)
        crcs.append(crc)
    return (pages, crcs) if checksums else pages


def upload_blocks_fused(store, keys, blocks, compressor, enc=None, checksums=True):
    """cachedStore.upload for a batch in one engine call (jfsx_store_batch): each
    block is checksummed (bcache.stage's checksum(), disk_cache.go:433-483),
    compressed and, with enc (a DataEncryptor), sealed without leaving the
    device in between (cached_store.go:371-413, :439); the raw `store` receives
    header || C || tag per block, or the compressed block itself without enc --
    the objects load_blocks(NewEncrypted(store, enc) or store, ...) and
    load_blocks_fused read back.

    Key and nonce of block i are drawn from enc's rand in DataEncryptor.Encrypt's
    order (key, then the wrap on the host by keyEncryptor.Encrypt, then the
    nonce; encrypt.go:165-180), block by block; with DataEncryptor(wrap="gpu")
    the keys of all blocks are wrapped in one engine call first, each block's
    OAEP seed drawn between its key and its nonce (DataEncryptor.draw_keys).
    Returns (objects, crcs) with crcs[i] == checksum(blocks[i]), or the objects
    alone with checksums=False."""
    if not isinstance(compressor, (LZ4, ZStandard)):
        raise ValueError("upload_blocks_fused needs the lz4 or zstd compressor (an uncompressed volume uploads "
                         "through DataEncryptor.EncryptBatch)")
    eng = compressor.eng
    codec = E.CODEC_LZ4 if isinstance(compressor, LZ4) else E.CODEC_ZSTD
    blocks = [bytes(b) for b in blocks]
    hdrs = []
    if enc is None:
        algo, items = E.CIPHER_NONE, blocks
        hdrs = [b""] * len(blocks)
    else:
        algo, items = enc.algo, []
        for b, (key, cipherkey, nonce) in zip(blocks, enc.draw_keys(len(blocks))):
            hdrs.append(bytes([len(cipherkey) >> 8, len(cipherkey) & 0xFF, len(nonce)]) + cipherkey + nonce)
            items.append((key, nonce, b))
    if not blocks:
        return ([], []) if checksums else []
    res = eng.store(algo, codec, items, crc=checksums)
    objs, crcs = [], []
    for k, h, (st, img, tag, crc, _) in zip(keys, hdrs, res):
        if st != E.OK:  # no page CRCs were given to verify: the engine has no other per-block failure
            raise CompressError("store %s: engine status %d" % (k, st))
        obj = h + img + (tag or b"")
        store.Put(k, obj)
        objs.append(obj)
        crcs.append(crc)
    return (objs, crcs) if checksums else objs


def upload_objects_fused(store, keys, blocks, compressor, enc, checksums=True, object_checksums=False):
    """cachedStore.upload for a batch in one engine call that ends at the stored
    object (jfsx_store_objects): the data keys' RSA-OAEP wrap, checksum() of
    every block, Compress, Seal, the header and tag around C and the object
    store's checksum run back to back on the device, and `store` receives what
    comes down, as it is.  enc is the volume's DataEncryptor; compressor may be
    the "none" compressor or None for a volume without --compress.

    Key, OAEP seed and nonce of block i are drawn from enc's rand block by
    block (DataEncryptor.draw_raw), the order DataEncryptor(wrap="gpu") draws
    them in: with the same rand the objects are byte for byte those of
    upload_blocks_fused with such an encryptor and, without a codec, those of
    its EncryptBatch.  Returns (objects, crcs) with crcs[i] ==
    checksum(blocks[i]), or the objects alone with checksums=False; with
    object_checksums=True the decimal checksum strings of the objects
    (checksum.go:31-53) follow as one more element.  An RSA key the engine does
    not take goes through upload_blocks_fused / DataEncryptor.EncryptBatch."""
    from .encrypt import rsa_public_exponent
    coded = isinstance(compressor, (LZ4, ZStandard))
    if enc is None:
        raise ValueError("upload_objects_fused needs a DataEncryptor (a volume without one: upload_blocks_fused)")
    codec = E.CODEC_NONE if not coded else E.CODEC_LZ4 if isinstance(compressor, LZ4) else E.CODEC_ZSTD
    eng = compressor.eng if coded else enc.eng
    blocks = [bytes(b) for b in blocks]
    ke = enc.keyEncryptor
    dk = ke._device_key(eng) if hasattr(ke, "_device_key") else None
    e = rsa_public_exponent(ke.privKey) if dk is not None else 0
    if dk is None or not 2 <= e <= 0x7FFFFFFF:
        if coded:
            res = upload_blocks_fused(store, keys, blocks, compressor, enc=enc, checksums=checksums)
            objs = res[0] if checksums else res
        else:
            objs = enc.EncryptBatch(blocks)
            for k, o in zip(keys, objs):
                store.Put(k, o)
            res = (objs, [eng.checksum(b) for b in blocks]) if checksums else objs
        if not object_checksums:
            return res
        sums = [str(E.crc32c_update(0, o)) for o in objs]
        return (res[0], res[1], sums) if checksums else (res, sums)
    if not blocks:
        out = ([], []) if checksums else []
        return (out + ([],) if checksums else (out, [])) if object_checksums else out
    items = [(key, seed, nonce, b) for b, (key, seed, nonce) in zip(blocks, enc.draw_raw(len(blocks)))]
    res = eng.store_objects(dk, e, enc.algo, codec, items, crc=checksums, object_crc=object_checksums)
    objs, crcs, sums = [], [], []
    for k, (st, obj, crc, ocrc) in zip(keys, res):
        if st != E.OK:  # no page CRCs were given to verify: the engine has no other per-block failure
            raise CompressError("store %s: engine status %d" % (k, st))
        store.Put(k, obj)
        objs.append(obj)
        crcs.append(crc)
        sums.append(str(ocrc) if object_checksums else None)
    out = (objs, crcs) if checksums else objs
    if object_checksums:
        return (objs, crcs, sums) if checksums else (objs, sums)
    return out


def compact_fused(store, slices, new_id, block_size, compressor, enc, checksums=True, object_checksums=None):
    """vfs.Compact (pkg/vfs/compact.go:54-109) for one chunk in one engine call
    (jfsx_compact_objects): the live ranges of the old slices are read block by
    block, written with zeros for holes as the new slice new_id, and that slice
    is cut into blocks, compressed and sealed.  Stored objects go up and stored
    objects come down; the pages exist in device memory only.

    slices are (id, size, off, len) in the order Compact receives them
    (meta.Slice), id 0 a hole.  The planner (jfsx_compact_plan) names the
    source blocks, each is fetched once with store.Get(block_key(id, indx,
    bsize)); object_checksums maps a source key to the decimal string the store
    kept for it (a key it lacks is not verified).  Key, OAEP seed and nonce of
    new block j are drawn from enc's rand block by block, as
    upload_objects_fused draws them.  If every page comes back JFSX_OK the
    objects are Put as block_key(new_id, j, len_j); if a Get fails or a page
    does not, nothing is Put and CompressError names the failing source key and
    its status (the reference's writer.Abort()).

    Returns (keys, objects, crcs) with crcs[j] == checksum(page j), or (keys,
    objects) with checksums=False; with object_checksums given, the decimal
    checksum strings of the new objects follow as one more element."""
    from .checksum import parse_checksum
    from .chunk import block_key
    from .encrypt import rsa_public_exponent
    coded = isinstance(compressor, (LZ4, ZStandard))
    if enc is None:
        raise ValueError("compact_fused needs a DataEncryptor")
    codec = E.CODEC_NONE if not coded else E.CODEC_LZ4 if isinstance(compressor, LZ4) else E.CODEC_ZSTD
    eng = compressor.eng if coded else enc.eng
    ke = enc.keyEncryptor
    dk = ke._device_key(eng) if hasattr(ke, "_device_key") else None
    e = rsa_public_exponent(ke.privKey) if dk is not None else 0
    if dk is None or not 2 <= e <= 0x7FFFFFFF:
        raise ValueError("compact_fused needs an RSA-2048 key with CRT parameters")
    srcs, pages, pieces = E.compact_plan(block_size, slices)
    skeys = [block_key(sid, indx, bsize) for sid, indx, bsize in srcs]
    sources, expect = [], []
    for k in skeys:
        try:
            o = bytes(store.Get(k, 0, -1))
        except Exception as ex:
            raise CompressError("compact %d: read %s: %s" % (new_id, k, ex))
        klen, nlen = ((o[0] << 8) + o[1], o[2]) if len(o) >= 3 else (0, 0)
        h = 3 + klen + nlen
        if len(o) < 3 or len(o) < h + 16:  # too short to cut into header, C and tag (encrypt.go:199-201)
            raise CompressError("compact %d: read %s: misformed ciphertext: %d %d" % (new_id, k, klen, nlen))
        sources.append((o[:h], o[h:-16], o[-16:]))
        w = parse_checksum(object_checksums.get(k)) if object_checksums is not None else None
        expect.append(w if w is not None else (E.crc32c_update(0, o) if object_checksums is not None else None))
    nkeys = [block_key(new_id, j, n) for j, (_, _, n) in enumerate(pages)]
    if not pages:
        out = ([], [], []) if checksums else ([], [])
        return out + ([],) if object_checksums is not None else out
    res = eng.compact_objects(dk, e, enc.algo, codec, sources, [b for _, _, b in srcs], enc.draw_raw(len(pages)),
                              pages, pieces, crc=checksums, expect=expect if object_checksums is not None else None,
                              object_crc=object_checksums is not None)
    for (st, _, _, _, bad) in res:
        if st == E.ESRC:
            raise CompressError("compact %d: source %s: engine status %d" % (new_id, skeys[bad],
                                                                             eng.compact_info[bad][0]))
        if st != E.OK:
            raise CompressError("compact %d: engine status %d" % (new_id, st))
    for k, (_, obj, _, _, _) in zip(nkeys, res):
        store.Put(k, obj)
    out = (nkeys, [r[1] for r in res]) + (([r[2] for r in res],) if checksums else ())
    if object_checksums is not None:
        out += ([str(r[3]) for r in res],)
    return out
