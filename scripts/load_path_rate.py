#!/usr/bin/env python3
"""Wall time of the one-call block load (jfsx_load_batch) against the same
blocks through the separate calls, host memory, one JSON line.

Workload: --blocks blocks of --block-mib MiB of word text (tests.lz4_data
"text"), compressed by the engine's own compressors and sealed by
jfsx_seal_batch; both codecs x {AES-256-GCM, no cipher}.  Per case, in one
process and on one context:
  one     jfsx_load_batch(CRC_GEN), JFSX_MEM_HOST
  seq     jfsx_open_batch -> jfsx_lz4/zstd_decompress_batch ->
          jfsx_crc32c_segments(GEN), JFSX_MEM_HOST (no cipher: the last two)
alternating one / seq: --warmup rounds, then the median of --reps (>= 5) rounds
with the min-max spread of each path.  Every buffer is pageable (numpy), as a
Go-heap slice is.  bytes_h2d / bytes_d2h: what each path moves over PCIe, from
the shapes (s = stored bytes, L = page bytes, c = CRC bytes):
  seq     2s + L up, s + L + c down   (no cipher: s + L up, L + c down)
  one     s up, L + c down
Both paths' pages and CRC arrays are compared with the plaintext and with each
other before anything is reported.
"""
import argparse
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


def run_case(eng, E, plains, codec, algo, reps, warmup):
    n = len(plains)
    lens = [len(p) for p in plains]
    comps = eng.lz4_compress(plains) if codec == E.CODEC_LZ4 else eng.zstd_compress(plains)
    keys = [E.gen_key(0x10AD, i) for i in range(n)]
    imgs = [np.frombuffer(c, np.uint8).copy() for c in comps]
    tags = [None] * n
    if algo != E.CIPHER_NONE:
        arr, m = eng.make_blocks([{"key": k, "nonce": nn, "src": a.ctypes.data, "dst": a.ctypes.data, "len": a.size}
                                  for (k, nn), a in zip(keys, imgs)])
        eng.seal_batch(algo, arr, m, E.CRC_NONE, E.MEM_HOST)
        tags = [bytes(arr[i].tag) for i in range(n)]
    nseg = [max(1, -(-L // E.SEG)) for L in lens]
    # one call
    pages1 = [np.empty(L, np.uint8) for L in lens]
    crcs1 = [np.empty(4 * k, np.uint8) for k in nseg]
    larr, m = eng.make_lblocks([{"key": k if tags[i] else None, "nonce": nn, "tag": tags[i], "src": imgs[i].ctypes.data,
                                 "src_len": imgs[i].size, "dst": pages1[i].ctypes.data, "len": lens[i],
                                 "crc": crcs1[i].ctypes.data} for i, (k, nn) in enumerate(keys)])
    # the separate calls
    opened = [np.empty(a.size, np.uint8) for a in imgs]
    pages2 = [np.empty(L, np.uint8) for L in lens]
    crcs2 = [np.empty(4 * k, np.uint8) for k in nseg]
    if algo != E.CIPHER_NONE:
        oarr, _ = eng.make_blocks([{"key": k, "nonce": nn, "src": imgs[i].ctypes.data, "dst": opened[i].ctypes.data,
                                    "len": imgs[i].size, "tag": tags[i]} for i, (k, nn) in enumerate(keys)])
    zsrc = opened if algo != E.CIPHER_NONE else imgs
    zarr, _ = eng.make_zblocks((zsrc[i].ctypes.data, zsrc[i].size, pages2[i].ctypes.data, lens[i]) for i in range(n))
    rarr = (E.jfsx_range * n)()
    for i in range(n):
        rarr[i].data, rarr[i].len, rarr[i].crc = pages2[i].ctypes.data, lens[i], crcs2[i].ctypes.data
    decode = eng.lz4_decompress_batch if codec == E.CODEC_LZ4 else eng.zstd_decompress_batch

    def one():
        eng.load_batch(algo, codec, larr, m, E.CRC_GEN, E.MEM_HOST)

    def seq():
        if algo != E.CIPHER_NONE:
            eng.open_batch(algo, oarr, n, E.CRC_NONE, E.MEM_HOST)
        decode(zarr, n, E.MEM_HOST)
        eng.crc32c_segments(rarr, n, E.CRC_GEN, E.MEM_HOST)

    t_one, t_seq = [], []
    for r in range(warmup + reps):
        for fn, acc in ((one, t_one), (seq, t_seq)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                acc.append(dt)
    for i in range(n):
        assert larr[i].status == E.OK and larr[i].out_len == lens[i] and zarr[i].status == E.OK, i
        assert pages1[i].tobytes() == plains[i] and pages2[i].tobytes() == plains[i], i
        assert crcs1[i].tobytes() == crcs2[i].tobytes(), i
    s, L, c = sum(a.size for a in imgs), sum(lens), 4 * sum(nseg)
    aead = algo != E.CIPHER_NONE
    row = {"stored_bytes": s, "page_bytes": L, "crc_bytes": c, "one": spread(t_one), "seq": spread(t_seq),
           "seq_calls": 3 if aead else 2,
           "one_bytes_h2d": s, "one_bytes_d2h": L + c,
           "seq_bytes_h2d": (2 * s if aead else s) + L, "seq_bytes_d2h": (s if aead else 0) + L + c}
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
    a = ap.parse_args()
    reps = max(a.reps, 5)
    from juicefs_amd import engine as E
    from tests import lz4_data
    plains = [lz4_data.sample("text", a.block_mib << 20, seed=i) for i in range(a.blocks)]
    eng = E.Engine(0)
    out = {"tool": "load_path_rate", "blocks": a.blocks, "block_mib": a.block_mib, "kind": "text", "mem": "host",
           "reps": reps, "warmup": max(a.warmup, 1), "cases": {}}
    for cname, codec in (("lz4", E.CODEC_LZ4), ("zstd", E.CODEC_ZSTD)):
        for aname, algo in (("aes256gcm", E.AES256GCM), ("none", E.CIPHER_NONE)):
            out["cases"]["%s-%s" % (cname, aname)] = run_case(eng, E, plains, codec, algo, reps, max(a.warmup, 1))
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
