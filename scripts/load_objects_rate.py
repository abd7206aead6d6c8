#!/usr/bin/env python3
"""Wall time of the one-call object load (jfsx_load_objects) against the same
objects through the separate calls, host memory, one JSON line.

Workload: --blocks objects of --block-mib MiB of word text (tests.lz4_data
"text"), compressed by the engine's own compressors (or not at all), sealed by
jfsx_seal_batch under per-object data keys that are wrapped with a fixed
RSA-2048 key (tests/golden/rsa_keys.json, tests.rsa_model); AES-256-GCM x
{lz4, zstd, no codec}.  Per case, in one process and on one context:
  one     jfsx_load_objects(CRC_GEN | CRC_CT), JFSX_MEM_HOST
  seq     jfsx_rsa_oaep_decrypt_batch, the keys copied into the block records,
          then with a codec   jfsx_load_batch(CRC_GEN) and, for the store's
                              checksum, jfsx_crc32c_segments(GEN) over the
                              stored images
               without one    jfsx_open_batch(CRC_GEN | CRC_BOTH)
          then jfsx_object_crc32c per object and the compare
alternating one / seq: --warmup rounds, then the median of --reps (>= 5) rounds
with the min-max spread of each path.  Every buffer is pageable (numpy).
bytes_h2d / bytes_d2h: what each path moves over PCIe, from the shapes (s =
stored bytes, L = page bytes, c = page CRC bytes, t = image CRC bytes, w = 256 n
wrapped-key bytes, k = 32 n key bytes):
  seq     codec: w + k + 2 s up, k + L + c + t down; none: w + k + s up, k + L + c + t down
  one     w + s up, L + c down
Both paths' pages, CRC arrays and object checksums are compared with the
plaintext, the expected checksum and each other before anything is reported.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def run_case(eng, E, M, rsa, plains, codec, algo, reps, warmup):
    n = len(plains)
    lens = [len(p) for p in plains]
    coded = codec != E.CODEC_NONE
    comps = plains if not coded else eng.lz4_compress(plains) if codec == E.CODEC_LZ4 else eng.zstd_compress(plains)
    keys = [E.gen_key(0x0B7, i) for i in range(n)]
    imgs = [np.frombuffer(c, np.uint8).copy() for c in comps]
    arr, m = eng.make_blocks([{"key": k, "nonce": nn, "src": a.ctypes.data, "dst": a.ctypes.data, "len": a.size}
                              for (k, nn), a in zip(keys, imgs)])
    eng.seal_batch(algo, arr, m, E.CRC_NONE, E.MEM_HOST)
    tags = [bytes(arr[i].tag) for i in range(n)]
    name, dkey = rsa
    k = M.fixed_keys()[name]
    wrapped = [M.ct256(M.encrypt_em(k, M.oaep_encode(key, M.det_bytes(32, "rate", i))))
               for i, (key, _) in enumerate(keys)]
    hdrs = [np.frombuffer(bytes([1, 0, 12]) + w + nn, np.uint8).copy() for w, (_, nn) in zip(wrapped, keys)]
    expect = [E.crc32c_update(E.crc32c_update(E.crc32c_update(0, h), a), t) for h, a, t in zip(hdrs, imgs, tags)]
    nseg = [max(1, -(-L // E.SEG)) for L in lens]
    iseg = [max(1, -(-a.size // E.SEG)) for a in imgs]
    # one call
    pages1 = [np.empty(L, np.uint8) for L in lens]
    crcs1 = [np.empty(4 * s, np.uint8) for s in nseg]
    oarr, m = eng.make_oblocks([{"hdr": hdrs[i].ctypes.data, "hdr_len": hdrs[i].size, "tag": tags[i],
                                 "src": imgs[i].ctypes.data, "src_len": imgs[i].size, "dst": pages1[i].ctypes.data,
                                 "len": lens[i], "crc": crcs1[i].ctypes.data, "expect_crc": expect[i]}
                                for i in range(n)])
    # the separate calls
    ct = np.concatenate([np.frombuffer(w, np.uint8) for w in wrapped])
    ct_len = np.full(n, 256, np.uint32)
    msg = np.zeros(n * 32, np.uint8)
    msg_len = np.zeros(n, np.int32)
    pages2 = [np.empty(L, np.uint8) for L in lens]
    crcs2 = [np.empty(4 * s * (1 if coded else 2), np.uint8) for s in nseg]
    icrc = [np.empty(4 * s, np.uint8) for s in iseg]
    if coded:
        larr, _ = eng.make_lblocks([{"key": bytes(32), "nonce": nn, "tag": tags[i], "src": imgs[i].ctypes.data,
                                     "src_len": imgs[i].size, "dst": pages2[i].ctypes.data, "len": lens[i],
                                     "crc": crcs2[i].ctypes.data} for i, (_, nn) in enumerate(keys)])
        rarr = (E.jfsx_range * n)()
        for i in range(n):
            rarr[i].data, rarr[i].len, rarr[i].crc = imgs[i].ctypes.data, imgs[i].size, icrc[i].ctypes.data
    else:
        larr, _ = eng.make_blocks([{"key": bytes(32), "nonce": nn, "tag": tags[i], "src": imgs[i].ctypes.data,
                                    "dst": pages2[i].ctypes.data, "len": lens[i], "crc": crcs2[i].ctypes.data}
                                   for i, (_, nn) in enumerate(keys)])
    sums2 = [0] * n

    def one():
        eng.load_objects_batch(dkey, algo, codec, oarr, m, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)

    def seq():
        rc = eng.L.jfsx_rsa_oaep_decrypt_batch(eng.ctx, dkey, n, ct.ctypes.data, 256, ct_len.ctypes.data,
                                               msg.ctypes.data, 32, msg_len.ctypes.data)
        assert rc == 0
        for i in range(n):
            ctypes.memmove(larr[i].key, msg.ctypes.data + 32 * i, 32)
        if coded:
            eng.load_batch(algo, codec, larr, n, E.CRC_GEN, E.MEM_HOST)
            eng.crc32c_segments(rarr, n, E.CRC_GEN, E.MEM_HOST)
        else:
            eng.open_batch(algo, larr, n, E.CRC_GEN | E.CRC_BOTH, E.MEM_HOST)
        for i in range(n):
            segs = icrc[i] if coded else crcs2[i][4 * nseg[i]:]
            sums2[i] = E.object_crc32c(hdrs[i], segs, imgs[i].size, tags[i])
            assert sums2[i] == expect[i]

    t_one, t_seq = [], []
    for r in range(warmup + reps):
        for fn, acc in ((one, t_one), (seq, t_seq)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                acc.append(dt)
    for i in range(n):
        assert (oarr[i].status, oarr[i].out_len, oarr[i].key_len, oarr[i].obj_crc) == (E.OK, lens[i], 32, expect[i]), i
        assert larr[i].status == E.OK and msg_len[i] == 32, i
        assert pages1[i].tobytes() == plains[i] and pages2[i].tobytes() == plains[i], i
        assert crcs1[i].tobytes() == crcs2[i][:4 * nseg[i]].tobytes(), i
    s, L, c, t = sum(a.size for a in imgs), sum(lens), 4 * sum(nseg), 4 * sum(iseg)
    w, kb = 256 * n, 32 * n
    row = {"stored_bytes": s, "page_bytes": L, "crc_bytes": c, "one": spread(t_one), "seq": spread(t_seq),
           "seq_calls": 3 if coded else 2, "one_bytes_h2d": w + s, "one_bytes_d2h": L + c,
           "seq_bytes_h2d": w + kb + (2 * s if coded else s), "seq_bytes_d2h": kb + L + c + t,
           "key_bytes_on_host_one": 0, "key_bytes_on_host_seq": kb}
    row["one_page_GBps"] = round(L / (row["one"]["median_ms"] * 1e-3) / 1e9, 2)
    row["seq_page_GBps"] = round(L / (row["seq"]["median_ms"] * 1e-3) / 1e9, 2)
    row["one_over_seq"] = round(row["one"]["median_ms"] / row["seq"]["median_ms"], 3)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--block-mib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    from juicefs_amd import engine as E
    from tests import lz4_data
    from tests import rsa_model as M
    plains = [lz4_data.sample("text", a.block_mib << 20, seed=i) for i in range(a.blocks)]
    eng = E.Engine(0)
    name = next(iter(M.fixed_keys()))
    dkey = eng.rsa_key(*M.components(M.fixed_keys()[name]))
    out = {"tool": "load_objects_rate", "blocks": a.blocks, "block_mib": a.block_mib, "kind": "text", "mem": "host",
           "cipher": "aes256gcm", "reps": reps, "warmup": max(a.warmup, 1), "cases": {}}
    for cname, codec in (("lz4", E.CODEC_LZ4), ("zstd", E.CODEC_ZSTD), ("none", E.CODEC_NONE)):
        out["cases"][cname] = run_case(eng, E, M, (name, dkey), plains, codec, E.AES256GCM, reps, max(a.warmup, 1))
    eng.rsa_key_free(dkey)
    eng.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
