#!/usr/bin/env python3
"""Wall and CPU time of the one-call object store (jfsx_store_objects) against
the same pages through the separate calls, host memory; one JSON line, also
written to profiles/storeobjects/store_objects_rate.json.

Workload: --blocks pages of --block-mib MiB of word text (tests.lz4_data
"text") with their checksum() arrays, as a staged file holds them; AES-256-GCM;
codecs none, lz4 and zstd; RSA key "plain_p_gt_q" of tests/golden/rsa_keys.json.
Per case, in one process and on one context:
  one     jfsx_store_objects(CRC_VERIFY | CRC_CT), JFSX_MEM_HOST: the objects
          come back whole, with obj_crc
  seq     jfsx_rsa_oaep_encrypt_batch, then jfsx_store_batch(CRC_VERIFY |
          CRC_CT) -- without a codec jfsx_crc32c_segments(VERIFY) and
          jfsx_seal_batch(GEN | CT) -- then, per object, the host's header
          build, the copy of header, image and tag into the object buffer, and
          jfsx_object_crc32c
alternating one / seq: --warmup rounds, then the median of --reps (>= 5) rounds
with the min-max spread of each path, and the process CPU time of each path
(time.process_time around the same region, median).  Every buffer is pageable
(numpy), as a Go-heap slice is.  The host assembly of seq is three numpy slice
copies and one ctypes call per object: a lower bound on what a per-object Go
loop costs.  Both paths' objects and object checksums are compared with each
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

HDR, TAG = 271, 16


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def run_case(eng, E, dk, e, plains, crcs, codec, reps, warmup):
    n = len(plains)
    algo = E.AES256GCM
    lens = [len(p) for p in plains]
    coded = codec != E.CODEC_NONE
    caps = [E.object_bound(codec, L) for L in lens]
    draws = [(bytes(E.gen_key(0x50B, i)[0]), bytes(E.gen_key(0x5EED, i)[0]), bytes(E.gen_key(0x50B, i)[1]))
             for i in range(n)]  # key, OAEP seed, nonce
    pages = [np.frombuffer(p, np.uint8).copy() for p in plains]
    crcin = [np.frombuffer(c, np.uint8).copy() for c in crcs]
    # one call
    obj1 = [np.empty(c, np.uint8) for c in caps]
    oarr, m = eng.make_soblocks([{"key": k, "seed": s, "nonce": nn, "src": pages[i].ctypes.data, "len": lens[i],
                                  "obj": obj1[i].ctypes.data, "obj_cap": caps[i], "crc": crcin[i].ctypes.data}
                                 for i, (k, s, nn) in enumerate(draws)])
    # the separate calls
    obj2 = [np.empty(c, np.uint8) for c in caps]
    img2 = [np.empty(c - HDR - TAG, np.uint8) for c in caps]
    seg2 = [np.empty(4 * max(1, -(-(c - HDR - TAG) // E.SEG)), np.uint8) for c in caps]
    rarr = (E.jfsx_range * n)()
    for i in range(n):
        rarr[i].data, rarr[i].len, rarr[i].crc = pages[i].ctypes.data, lens[i], crcin[i].ctypes.data
    crc2, len2 = [0] * n, [0] * n

    def one():
        eng.store_objects_batch(dk, e, algo, codec, oarr, m, E.CRC_VERIFY | E.CRC_CT, E.MEM_HOST)

    def seq():
        wrapped = eng.oaep_encrypt_batch(dk, [k for k, _, _ in draws], [s for _, s, _ in draws], e)
        hdrs = [bytes([1, 0, 12]) + w + nn for w, (_, _, nn) in zip(wrapped, draws)]
        if coded:
            hbuf = [np.frombuffer(h, np.uint8) for h in hdrs]
            sarr, _ = eng.make_sblocks([{"key": k, "nonce": nn, "src": pages[i].ctypes.data, "len": lens[i],
                                         "dst": img2[i].ctypes.data, "dst_cap": img2[i].size,
                                         "crc": crcin[i].ctypes.data, "hdr": hbuf[i].ctypes.data, "hdr_len": HDR}
                                        for i, (k, _, nn) in enumerate(draws)])
            eng.store_batch(algo, codec, sarr, n, E.CRC_VERIFY | E.CRC_CT, E.MEM_HOST)
            res = [(sarr[i].out_len, bytes(sarr[i].tag), sarr[i].obj_crc) for i in range(n)]
        else:
            eng.crc32c_segments(rarr, n, E.CRC_VERIFY, E.MEM_HOST)
            barr, _ = eng.make_blocks([{"key": k, "nonce": nn, "src": pages[i].ctypes.data,
                                        "dst": img2[i].ctypes.data, "len": lens[i], "crc": seg2[i].ctypes.data}
                                       for i, (k, _, nn) in enumerate(draws)])
            eng.seal_batch(algo, barr, n, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)
            res = [(lens[i], bytes(barr[i].tag), None) for i in range(n)]
        # the host's assembly and, where the engine has not folded it, the fold
        for i, (ln, tag, ocrc) in enumerate(res):
            o = obj2[i]
            o[:HDR] = np.frombuffer(hdrs[i], np.uint8)
            o[HDR:HDR + ln] = img2[i][:ln]
            o[HDR + ln:HDR + ln + TAG] = np.frombuffer(tag, np.uint8)
            len2[i] = HDR + ln + TAG
            crc2[i] = ocrc if ocrc is not None else eng.object_crc32c(hdrs[i], seg2[i], ln, tag)

    t = {"one": [], "seq": []}
    cpu = {"one": [], "seq": []}
    for r in range(warmup + reps):
        for name, fn in (("one", one), ("seq", seq)):
            c0, t0 = time.process_time(), time.perf_counter()
            fn()
            dt, dc = (time.perf_counter() - t0) * 1e3, (time.process_time() - c0) * 1e3
            if r >= warmup:
                t[name].append(dt)
                cpu[name].append(dc)
    for i in range(n):
        assert oarr[i].status == E.OK and oarr[i].out_len == len2[i], i
        assert obj1[i][:len2[i]].tobytes() == obj2[i][:len2[i]].tobytes(), i
        assert oarr[i].obj_crc == crc2[i], i
    L, c = sum(lens), sum(a.size for a in crcin)
    s = sum(int(oarr[i].img_len) for i in range(n))
    row = {"page_bytes": L, "image_bytes": s, "object_bytes": s + n * (HDR + TAG), "crc_bytes": c,
           "one": spread(t["one"]), "seq": spread(t["seq"]),
           "one_cpu": spread(cpu["one"]), "seq_cpu": spread(cpu["seq"]),
           "seq_calls": 2 if coded else 3,
           # over PCIe, from the shapes: keys and seeds 64 n up on both paths
           "one_bytes_h2d": L + c + 64 * n, "one_bytes_d2h": s + n * (HDR + TAG),
           "seq_bytes_h2d": (L + c if coded else 2 * L + c) + 64 * n, "seq_bytes_d2h": s + 256 * n}
    row["one_page_GBps"] = round(L / (row["one"]["median_ms"] * 1e-3) / 1e9, 2)
    row["seq_page_GBps"] = round(L / (row["seq"]["median_ms"] * 1e-3) / 1e9, 2)
    row["one_over_seq"] = round(row["one"]["median_ms"] / row["seq"]["median_ms"], 3)
    row["one_over_seq_cpu"] = round(row["one_cpu"]["median_ms"] / row["seq_cpu"]["median_ms"], 3)
    row["ranges_overlap"] = not (row["one"]["max_ms"] < row["seq"]["min_ms"] or
                                 row["seq"]["max_ms"] < row["one"]["min_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--block-mib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "storeobjects", "store_objects_rate.json"))
    a = ap.parse_args()
    reps = max(a.reps, 5)
    from juicefs_amd import engine as E
    from tests import lz4_data
    from tests import rsa_model as M
    plains = [lz4_data.sample("text", a.block_mib << 20, seed=i) for i in range(a.blocks)]
    eng = E.Engine(0)
    dk = eng.rsa_key(*M.components(M.fixed_keys()["plain_p_gt_q"]))
    crcs = [eng.checksum(p) for p in plains]
    out = {"tool": "store_objects_rate", "blocks": a.blocks, "block_mib": a.block_mib, "kind": "text", "mem": "host",
           "cipher": "aes256gcm", "crc_mode": "VERIFY|CT", "reps": reps, "warmup": max(a.warmup, 1), "cases": {}}
    for cname, codec in (("none", E.CODEC_NONE), ("lz4", E.CODEC_LZ4), ("zstd", E.CODEC_ZSTD)):
        out["cases"][cname] = run_case(eng, E, dk, M.E, plains, crcs, codec, reps, max(a.warmup, 1))
    eng.rsa_key_free(dk)
    eng.close()
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
