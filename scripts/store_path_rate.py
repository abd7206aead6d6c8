#!/usr/bin/env python3
"""Wall time of the one-call block store (jfsx_store_batch) against the same
pages through the separate calls, host memory; one JSON line, also written to
profiles/storepath/store_path_rate.json.

Workload: --blocks pages of --block-mib MiB of word text (tests.lz4_data
"text") with their checksum() arrays, as a staged file holds them; both codecs
x {AES-256-GCM, no cipher}.  Per case, in one process and on one context:
  one     jfsx_store_batch(CRC_VERIFY | CRC_CT), JFSX_MEM_HOST
  seq     jfsx_crc32c_segments(VERIFY) -> jfsx_lz4/zstd_compress_batch ->
          jfsx_seal_batch(GEN | CT) + jfsx_object_crc32c, JFSX_MEM_HOST
          (no cipher: the object checksum is a second jfsx_crc32c_segments(GEN)
          over the compressed blocks)
alternating one / seq: --warmup rounds, then the median of --reps (>= 5) rounds
with the min-max spread of each path.  Every buffer is pageable (numpy), as a
Go-heap slice is.  bytes_h2d / bytes_d2h: what each path moves over PCIe, from
the shapes (L = page bytes, s = stored bytes, c = page CRC bytes):
  seq     2L + s + c up, 2s down   (no cipher: 2L + s + c up, s down)
  one     L + c up, s down
Both paths' images, tags and object checksums are compared with each other
before anything is reported.
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

HDR = bytes((7 * i + 3) & 0xFF for i in range(271))


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def run_case(eng, E, plains, crcs, codec, algo, reps, warmup):
    n = len(plains)
    lens = [len(p) for p in plains]
    aead = algo != E.CIPHER_NONE
    bound = E.lz4_bound if codec == E.CODEC_LZ4 else E.zstd_bound
    caps = [int(bound(L)) for L in lens]
    keys = [E.gen_key(0x570E, i) for i in range(n)]
    pages = [np.frombuffer(p, np.uint8).copy() for p in plains]
    crcin = [np.frombuffer(c, np.uint8).copy() for c in crcs]
    hdr = np.frombuffer(HDR, np.uint8).copy()
    # one call
    dst1 = [np.empty(c, np.uint8) for c in caps]
    sarr, m = eng.make_sblocks([{"key": k if aead else None, "nonce": nn, "src": pages[i].ctypes.data, "len": lens[i],
                                 "dst": dst1[i].ctypes.data, "dst_cap": caps[i], "crc": crcin[i].ctypes.data,
                                 "hdr": hdr.ctypes.data, "hdr_len": hdr.size} for i, (k, nn) in enumerate(keys)])
    # the separate calls
    rarr = (E.jfsx_range * n)()
    for i in range(n):
        rarr[i].data, rarr[i].len, rarr[i].crc = pages[i].ctypes.data, lens[i], crcin[i].ctypes.data
    comp2 = [np.empty(c, np.uint8) for c in caps]
    zarr, _ = eng.make_zblocks((pages[i].ctypes.data, lens[i], comp2[i].ctypes.data, caps[i]) for i in range(n))
    dst2 = [np.empty(c, np.uint8) for c in caps]
    seg2 = [np.empty(4 * max(1, -(-c // E.SEG)), np.uint8) for c in caps]
    compress = eng.lz4_compress_batch if codec == E.CODEC_LZ4 else eng.zstd_compress_batch
    obj2 = [0] * n

    def one():
        eng.store_batch(algo, codec, sarr, m, E.CRC_VERIFY | E.CRC_CT, E.MEM_HOST)

    def seq():
        eng.crc32c_segments(rarr, n, E.CRC_VERIFY, E.MEM_HOST)
        compress(zarr, n, E.MEM_HOST)
        if aead:
            barr, _ = eng.make_blocks([{"key": k, "nonce": nn, "src": comp2[i].ctypes.data, "dst": dst2[i].ctypes.data,
                                        "len": zarr[i].out_len, "crc": seg2[i].ctypes.data}
                                       for i, (k, nn) in enumerate(keys)])
            eng.seal_batch(algo, barr, n, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
            return barr
        garr = (E.jfsx_range * n)()
        for i in range(n):
            garr[i].data, garr[i].len, garr[i].crc = comp2[i].ctypes.data, zarr[i].out_len, seg2[i].ctypes.data
        eng.crc32c_segments(garr, n, E.CRC_GEN, E.MEM_HOST)
        return None

    def fold(barr):
        """The host fold of the separate path (jfsx_object_crc32c's arithmetic),
        outside the timed region: in C it costs microseconds, here a Python loop."""
        for i in range(n):
            if aead:
                obj2[i] = eng.object_crc32c(HDR, seg2[i], zarr[i].out_len, bytes(barr[i].tag))
                continue
            crc = E.crc32c_update(0, HDR)
            for j in range(max(1, -(-zarr[i].out_len // E.SEG))):
                lj = min(E.SEG, zarr[i].out_len - j * E.SEG)
                crc = E.crc32c_combine(crc, int.from_bytes(seg2[i][4 * j:4 * j + 4].tobytes(), "big"), lj)
            obj2[i] = crc

    t_one, t_seq = [], []
    barr = None
    for r in range(warmup + reps):
        for fn, acc in ((one, t_one), (seq, t_seq)):
            t0 = time.perf_counter()
            res = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if fn is seq:
                barr = res
            if r >= warmup:
                acc.append(dt)
    fold(barr)
    for i in range(n):
        assert sarr[i].status == E.OK and rarr[i].status == E.OK and sarr[i].out_len == zarr[i].out_len, i
        img2 = dst2[i] if aead else comp2[i]
        assert dst1[i][:sarr[i].out_len].tobytes() == img2[:zarr[i].out_len].tobytes(), i
        assert sarr[i].obj_crc == obj2[i], i
        if aead:
            assert bytes(sarr[i].tag) == bytes(barr[i].tag), i
    s, L, c = sum(int(sarr[i].out_len) for i in range(n)), sum(lens), sum(a.size for a in crcin)
    row = {"page_bytes": L, "stored_bytes": s, "crc_bytes": c, "one": spread(t_one), "seq": spread(t_seq),
           "seq_calls": 3,
           "one_bytes_h2d": L + c, "one_bytes_d2h": s,
           "seq_bytes_h2d": 2 * L + s + c, "seq_bytes_d2h": 2 * s if aead else s}
    row["one_page_GBps"] = round(L / (row["one"]["median_ms"] * 1e-3) / 1e9, 2)
    row["seq_page_GBps"] = round(L / (row["seq"]["median_ms"] * 1e-3) / 1e9, 2)
    row["one_over_seq"] = round(row["one"]["median_ms"] / row["seq"]["median_ms"], 3)
    row["ranges_overlap"] = not (row["one"]["max_ms"] < row["seq"]["min_ms"] or
                                 row["seq"]["max_ms"] < row["one"]["min_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--block-mib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storepath", "store_path_rate.json"))
    a = ap.parse_args()
    reps = max(a.reps, 5)
    from juicefs_amd import engine as E
    from tests import lz4_data
    plains = [lz4_data.sample("text", a.block_mib << 20, seed=i) for i in range(a.blocks)]
    eng = E.Engine(0)
    crcs = [eng.checksum(p) for p in plains]
    out = {"tool": "store_path_rate", "blocks": a.blocks, "block_mib": a.block_mib, "kind": "text", "mem": "host",
           "reps": reps, "warmup": max(a.warmup, 1), "cases": {}}
    for cname, codec in (("lz4", E.CODEC_LZ4), ("zstd", E.CODEC_ZSTD)):
        for aname, algo in (("aes256gcm", E.AES256GCM), ("none", E.CIPHER_NONE)):
            out["cases"]["%s-%s" % (cname, aname)] = run_case(eng, E, plains, crcs, codec, algo, reps,
                                                              max(a.warmup, 1))
    eng.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
