"""The one-call object paths on a volume with a 4096-bit RSA key:
jfsx_store_objects, jfsx_load_objects and jfsx_compact_objects with the 527-byte
header BE16(512) | 12 | wrapped key (512) | nonce, against the separate calls
(jfsx_rsa_oaep_encrypt_batch, the compressor, jfsx_seal_batch,
jfsx_object_crc32c), the big-integer model of tests/rsa_model_wide.py and
tests/compact_model.py, in host and in device memory; the per-block verdicts
of a load; the key's own object bound; and the Python mirror's DataEncryptor on
a 4096-bit key without a host unwrap."""
import numpy as np
import pytest

from juicefs_amd import encrypt as enc
from juicefs_amd import engine as E
from tests import compact_model as CM
from tests import lz4_data
from tests import rsa_model as M2
from tests import rsa_model_wide as M

pytestmark = pytest.mark.gpu

CIPHERS = [E.AES256GCM, E.CHACHA20P1305]
CODECS = [E.CODEC_NONE, E.CODEC_LZ4, E.CODEC_ZSTD]
CODEC_IDS = ["none", "lz4", "zstd"]
KEY = "plain_q_gt_p"
HDR, TAG = 527, 16
LENGTHS = (0, 1, 32769, 100003)
KINDS = ("text", "runs", "zeros", "random")


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dk(eng):
    h = eng.rsa_key(*M.components(M.fixed_keys()[KEY]))
    yield h
    eng.rsa_key_free(h)


def draw(i):
    """(data key, OAEP seed, nonce) of block i."""
    return M.det_bytes(32, "obj4096 key", i), M.det_bytes(32, "obj4096 seed", i), M.det_bytes(12, "obj4096 nonce", i)


def pages_of(seed):
    return [lz4_data.sample(KINDS[i % 4], n, seed=seed) for i, n in enumerate(LENGTHS)]


def cut(o):
    return o[:HDR], o[HDR:-TAG], o[-TAG:]


def nseg(n):
    return max(1, -(-n // E.SEG))


def separate(eng, dk, algo, codec, draws, pages):
    """[(status, object, page crcs, obj_crc)] from the separate calls."""
    wrapped = eng.oaep_encrypt_batch(dk, [k for k, _, _ in draws], [s for _, s, _ in draws])
    k = M.fixed_keys()[KEY]
    assert wrapped == [M.encrypt(k, dkey, seed) for dkey, seed, _ in draws]  # the model's 512 bytes
    hdrs = [bytes([2, 0, 12]) + w + n for w, (_, _, n) in zip(wrapped, draws)]
    assert all(len(h) == HDR for h in hdrs)
    if codec != E.CODEC_NONE:
        res = eng.store(algo, codec, [(k, n, p) for (k, _, n), p in zip(draws, pages)], crc=True, headers=hdrs)
        return [(st, h + img + tag, crc, ocrc) for (st, img, tag, crc, ocrc), h in zip(res, hdrs)]
    out = []
    for (key, _, n), p, h in zip(draws, pages, hdrs):
        src = np.frombuffer(p, np.uint8).copy() if p else np.zeros(1, np.uint8)
        dst = np.empty(max(len(p), 1), np.uint8)
        cw = np.empty(8 * nseg(len(p)), np.uint8)
        arr, cnt = eng.make_blocks([{"key": key, "nonce": n, "src": src.ctypes.data, "dst": dst.ctypes.data,
                                     "len": len(p), "crc": cw.ctypes.data}])
        eng.seal_batch(algo, arr, cnt, E.CRC_GEN | E.CRC_BOTH, E.MEM_HOST)
        tag, half = bytes(arr[0].tag), 4 * nseg(len(p))
        out.append((E.OK, h + dst[:len(p)].tobytes() + tag, cw[:half].tobytes(),
                    E.object_crc32c(h, cw[half:].tobytes(), len(p), tag)))
    return out


def store_device(eng, dk, algo, codec, draws, pages, obj_mod=1):
    """jfsx_store_objects in device memory, obj % 16 == obj_mod: (rc, [(status, object, crcs, obj_crc)])."""
    caps = [E.object_bound(codec, len(p), dk) for p in pages]
    poff, ooff, coff = [], [], []
    po = oo = co = 0
    for p, cap in zip(pages, caps):
        poff.append(po), ooff.append(oo + obj_mod), coff.append(co)
        po += (len(p) + 31) & ~15
        oo += (cap + 47) & ~15
        co += 4 * nseg(len(p))
    src = np.zeros(max(po, 16), np.uint8)
    for p, o in zip(pages, poff):
        src[o:o + len(p)] = np.frombuffer(p, np.uint8)
    sbuf, obuf, cbuf = eng.alloc(src.size), eng.alloc(oo + 16), eng.alloc(co + 16)
    try:
        sbuf.upload(src)
        obuf.upload(np.full(oo + 16, 0xA5, np.uint8))
        specs = [{"key": k, "nonce": n, "seed": s, "src": sbuf.ptr + poff[i] if len(pages[i]) else None,
                  "len": len(pages[i]), "obj": obuf.ptr + ooff[i], "obj_cap": caps[i], "crc": cbuf.ptr + coff[i]}
                 for i, (k, s, n) in enumerate(draws)]
        arr, cnt = eng.make_soblocks(specs)
        rc = eng.L.jfsx_store_objects(eng.ctx, dk, M.E, algo, codec, cnt, arr, E.CRC_GEN | E.CRC_CT, E.MEM_DEVICE)
        if rc:
            return rc, None
        obj, cw = obuf.download(), cbuf.download()
        return 0, [(arr[i].status, obj[ooff[i]:ooff[i] + arr[i].out_len].tobytes(),
                    cw[coff[i]:coff[i] + 4 * nseg(len(pages[i]))].tobytes(), arr[i].obj_crc) for i in range(cnt)]
    finally:
        for b in (sbuf, obuf, cbuf):
            b.free()


def load_device(eng, dk, algo, codec, objs, lengths, expect):
    """jfsx_load_objects in device memory: [(status, page, crcs, key_len)]."""
    ioff, poff, coff = [], [], []
    io = po = co = 0
    for o, n in zip(objs, lengths):
        ioff.append(io), poff.append(po), coff.append(co)
        io += (len(o) - HDR - TAG + 31) & ~15
        po += (n + 31) & ~15
        co += 4 * nseg(n)
    img = np.zeros(max(io, 16), np.uint8)
    for o, at in zip(objs, ioff):
        c = o[HDR:-TAG]
        img[at:at + len(c)] = np.frombuffer(c, np.uint8)
    ibuf, pbuf, cbuf = eng.alloc(img.size), eng.alloc(po + 16), eng.alloc(co + 16)
    hdrs = [np.frombuffer(o[:HDR], np.uint8).copy() for o in objs]
    try:
        ibuf.upload(img)
        specs = [{"hdr": hdrs[i].ctypes.data, "hdr_len": HDR, "tag": o[-TAG:],
                  "src": ibuf.ptr + ioff[i] if len(o) > HDR + TAG else None, "src_len": len(o) - HDR - TAG,
                  "dst": pbuf.ptr + poff[i] if lengths[i] else None, "len": lengths[i], "crc": cbuf.ptr + coff[i],
                  "expect_crc": expect[i]} for i, o in enumerate(objs)]
        arr, cnt = eng.make_oblocks(specs)
        eng.load_objects_batch(dk, algo, codec, arr, cnt, E.CRC_GEN | E.CRC_CT, E.MEM_DEVICE)
        pg, cw = pbuf.download(), cbuf.download()
        return [(arr[i].status, pg[poff[i]:poff[i] + lengths[i]].tobytes(),
                 cw[coff[i]:coff[i] + 4 * nseg(lengths[i])].tobytes(), arr[i].key_len) for i in range(cnt)]
    finally:
        for b in (ibuf, pbuf, cbuf):
            b.free()


# ---- 1. store = the separate calls, load brings the pages back, both memories
@pytest.mark.parametrize("codec", CODECS, ids=CODEC_IDS)
@pytest.mark.parametrize("algo", CIPHERS, ids=["gcm", "chacha"])
def test_store_equals_separate_calls_and_loads_back(eng, dk, algo, codec):
    pages = pages_of(41)
    draws = [draw(100 + i) for i in range(len(pages))]
    sep = separate(eng, dk, algo, codec, draws, pages)
    got = eng.store_objects(dk, M.E, algo, codec, [(k, s, n, p) for (k, s, n), p in zip(draws, pages)])
    for i, (a, b) in enumerate(zip(got, sep)):
        assert a == b, (i, LENGTHS[i], "host")
    rc, dev = store_device(eng, dk, algo, codec, draws, pages)
    assert rc == 0
    for i, (a, b) in enumerate(zip(dev, sep)):
        assert a == b, (i, LENGTHS[i], "device")
    objs = [g[1] for g in got]
    assert all(o[:3] == bytes([2, 0, 12]) for o in objs)
    assert [E.object_bound(codec, len(p), dk) for p in pages] == \
        [E.object_bound(codec, len(p)) + 256 for p in pages]
    # the wrapped key is the model's, and the model unwraps it
    k = M.fixed_keys()[KEY]
    assert M.decrypt(k, objs[1][3:515]) == draws[1][0]
    back = eng.load_objects(dk, algo, codec, [cut(o) for o in objs], [len(p) for p in pages], crc=True,
                            expect=[g[3] for g in got])
    for i, ((st, page, crc), p) in enumerate(zip(back, pages)):
        assert (st, page, crc, eng.load_info[i][2]) == (E.OK, p, got[i][2], 32), i
    backd = load_device(eng, dk, algo, codec, objs, [len(p) for p in pages], [g[3] for g in got])
    for i, ((st, page, crc, kl), p) in enumerate(zip(backd, pages)):
        assert (st, page, crc, kl) == (E.OK, p, got[i][2], 32), i


# ---- 2. per-block verdicts ---------------------------------------------------
@pytest.mark.parametrize("codec", [E.CODEC_NONE, E.CODEC_LZ4], ids=["none", "lz4"])
def test_load_verdicts(eng, dk, codec):
    algo = E.AES256GCM
    pages = [lz4_data.sample("text", n, seed=43) for n in (1000, 40000, 33, 70000, 5000, 2000)]
    draws = [draw(200 + i) for i in range(len(pages))]
    got = eng.store_objects(dk, M.E, algo, codec, [(k, s, n, p) for (k, s, n), p in zip(draws, pages)])
    objs = [g[1] for g in got]
    # 1: klen = 513; 2: a header wrapped under a 2048-bit key; 3: a flipped wrapped-key byte; 4: a flipped tag
    o = objs[1]
    objs[1] = bytes([2, 1, 12]) + b"\0" + o[3:]
    k2 = M2.fixed_keys()["plain_q_gt_p"]
    w2 = M2.ct256(M2.encrypt_em(k2, M2.oaep_encode(draws[2][0], draws[2][1])))
    objs[2] = bytes([1, 0, 12]) + w2 + objs[2][515:]
    o = bytearray(objs[3])
    o[3 + 300] ^= 1
    objs[3] = bytes(o)
    o = bytearray(objs[4])
    o[-1] ^= 0x80
    objs[4] = bytes(o)
    items = [(o[:-TAG - len(c)], c, o[-TAG:]) for o, c in ((o, cut(g[1])[1]) for o, g in zip(objs, got))]
    assert [len(h) for h, _, _ in items] == [527, 528, 271, 527, 527, 527]
    back = eng.load_objects(dk, algo, codec, items, [len(p) for p in pages], crc=True)
    want = [E.OK, E.EKEY, E.EKEY, E.EKEY, E.ETAG, E.OK]
    assert [st for st, _, _ in back] == want
    assert [eng.load_info[i][2] for i in range(6)] == [32, -1, -1, -1, 32, 32]
    for i, ((st, page, crc), p) in enumerate(zip(back, pages)):
        if want[i] == E.OK:
            assert (page, crc) == (p, got[i][2]), i  # the neighbours are unaffected
        else:
            assert page == bytes(len(p)) and crc == bytes(len(crc)), i  # page and CRC array all zero


# ---- 3. the key's own bound --------------------------------------------------
def test_object_bound_is_the_keys(eng, dk):
    algo, codec = E.AES256GCM, E.CODEC_NONE
    page = lz4_data.sample("text", 5000, seed=47)
    key, seed, nonce = draw(300)
    bound = E.object_bound(codec, len(page), dk)
    assert bound == 527 + 5000 + 16 and E.object_bound(codec, len(page)) == 271 + 5000 + 16
    assert E.object_bound(3, 10, dk) == 0 and int(eng.L.jfsx_object_bound_key(None, codec, 10)) == 0
    src = np.frombuffer(page, np.uint8).copy()
    for cap, want in ((bound, 0), (bound - 1, E.EINVAL), (E.object_bound(codec, len(page)), E.EINVAL)):
        obj = np.full(bound + 64, 0xA5, np.uint8)
        crc = np.full(4, 0xA5, np.uint8)
        arr, cnt = eng.make_soblocks([{"key": key, "nonce": nonce, "seed": seed, "src": src.ctypes.data,
                                       "len": len(page), "obj": obj.ctypes.data, "obj_cap": cap,
                                       "crc": crc.ctypes.data}])
        b = arr[0]
        b.status, b.out_len, b.img_len, b.obj_crc = 77, 78, 79, 80
        rc = eng.L.jfsx_store_objects(eng.ctx, dk, M.E, algo, codec, cnt, arr, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
        assert rc == want, cap
        if want:  # JFSX_EINVAL, not an overrun: the record and the buffers untouched
            assert (b.status, b.out_len, b.img_len, b.obj_crc) == (77, 78, 79, 80)
            assert (obj == 0xA5).all() and (crc == 0xA5).all()
        else:
            assert (b.status, b.out_len) == (E.OK, bound) and (obj[bound:] == 0xA5).all()
    # device memory: obj % 16 == 1 is the rule at this width too
    rc, _ = store_device(eng, dk, algo, codec, [draw(301)], [page], obj_mod=0)
    assert rc == E.EINVAL


# ---- 4. compaction -----------------------------------------------------------
def test_compact_three_blocks_into_two_pages(eng, dk):
    algo, codec, bs = E.CHACHA20P1305, E.CODEC_LZ4, 65536
    rng = np.random.default_rng(0x4096)
    data = {7: lz4_data.sample("text", 2 * bs, seed=53), 9: rng.integers(0, 256, 30000, dtype=np.uint8).tobytes()}
    # slice 7's two blocks, a hole, the head of slice 9: 64 KiB and a ragged tail
    slices = [(7, 2 * bs, 100, bs + 5000), (0, 777, 0, 777), (9, 30000, 0, 20001)]
    sources, pages, pieces = CM.plan(bs, slices)
    blocks = CM.slice_blocks(data, bs)
    src_pages = [blocks[(sid, indx)] for sid, indx, _ in sources]
    new_pages = CM.compact_bytes(slices, data, bs)
    assert len(src_pages) == 3 and [len(p) for p in new_pages] == [bs, 5000 + 777 + 20001]
    assert any(s < 0 for s, _, _ in pieces)
    sd = [draw(400 + i) for i in range(3)]
    stored = eng.store_objects(dk, M.E, algo, codec, [(k, s, n, p) for (k, s, n), p in zip(sd, src_pages)])
    src_objs = [g[1] for g in stored]
    draws = [draw(500 + j) for j in range(len(pages))]
    one = eng.compact_objects(dk, M.E, algo, codec, [cut(o) for o in src_objs], [len(p) for p in src_pages], draws,
                              pages, pieces, expect=[g[3] for g in stored])
    assert [c[3] for c in eng.compact_info] == [32, 32, 32]
    sep = separate(eng, dk, algo, codec, draws, new_pages)  # the model's pages through the separate calls
    assert [(st, obj, crc, ocrc) for st, obj, crc, ocrc, _ in one] == sep
    assert [bad for _, _, _, _, bad in one] == [-1, -1]


# ---- 5. the Python mirror ----------------------------------------------------
def test_data_encryptor_round_trip_without_host_unwrap(eng, monkeypatch):
    priv = enc.GenerateRsaKey(4096)
    rsae = enc.NewRSAEncryptor(priv)
    assert rsae._device_key(eng) is not None and E.rsa_key_bytes(rsae._device_key(eng)) == 512
    de = enc.DataEncryptor(rsae, E.AES256GCM, eng, wrap="gpu")
    pages = [b"", b"x", lz4_data.sample("text", 40000, seed=59)]
    monkeypatch.setattr(enc.RsaEncryptor, "Encrypt", lambda *a: pytest.fail("host wrap"))
    objs = de.EncryptBatch(pages)
    assert all(o[:3] == bytes([2, 0, 12]) and len(o) == 527 + len(p) + 16 for o, p in zip(objs, pages))
    monkeypatch.undo()
    assert [rsae.Decrypt(o[3:515]) is not None for o in objs] == [True] * 3  # libcrypto unwraps them
    monkeypatch.setattr(enc.RsaEncryptor, "Decrypt", lambda *a: pytest.fail("host unwrap"))
    assert de.DecryptBatch(objs) == pages
    # a 3072-bit key is still the host's
    monkeypatch.undo()
    assert enc.NewRSAEncryptor(enc.GenerateRsaKey(3072))._device_key(eng) is None
