#!/usr/bin/env python3
"""Wall and CPU time of one-call slice compaction (jfsx_compact_objects)
against the same work through the separate calls, host memory; one JSON line,
also written to profiles/compact/compact_rate.json.

Workload: --pages new pages of --block-mib MiB assembled from --sources stored
blocks of the same size of word text (tests.lz4_data "text"); pieces of 1-3
MiB at odd offsets and of odd lengths, about 5 % of the bytes holes;
AES-256-GCM; codecs none, lz4 and zstd; RSA key "plain_p_gt_q" of
tests/golden/rsa_keys.json; JFSX_CRC_CT on the sources, JFSX_CRC_GEN | JFSX_CRC_CT
on the new pages.  The source objects are made once by jfsx_store_objects.
Per case, in one process and on one context:
  one     jfsx_compact_objects: images up, objects down
  seq     jfsx_load_objects (JFSX_MEM_HOST) into host pages, a host loop of
          numpy slice copies (and zero fills) that assembles the new pages,
          jfsx_store_objects (JFSX_MEM_HOST)
alternating one / seq: --warmup rounds, then the median of --reps (>= 5) rounds
with the min-max spread of each path, and the process CPU time of each path
(time.process_time around the same region, median).  Every buffer is pageable
(numpy), as a Go-heap slice is.  Both paths' objects, page CRCs and object
checksums are compared with each other before anything is reported.

The gather launch alone: jfsx_gather_batch (JFSX_MEM_DEVICE) over the same
pieces between the context's timing events (jfsx_ctx_set_timing), and, in the
same process, hipMemcpyAsync device-to-device of the same total bytes between
two events on the null stream; medians of the same number of rounds.
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

HDR, TAG = 271, 16
MIB = 1 << 20


def spread(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def make_pieces(rng, n_pages, n_src, block):
    """-> (pages [(piece_first, piece_count, len)], pieces [(src, src_off, len)])"""
    pages, pieces = [], []
    for _ in range(n_pages):
        first, room = len(pieces), block
        while room:
            ln = min(room, int(rng.integers(MIB, 3 * MIB)) | 1)
            if rng.random() < 0.3:  # holes of 64-448 KiB in front of a third of the pieces: about 5 % of the bytes
                h = min(room, int(rng.integers(MIB // 16, 7 * MIB // 16)) | 1)
                pieces.append((-1, 0, h))
                room -= h
                if not room:
                    break
                ln = min(ln, room)
            off = int(rng.integers(0, block - ln + 1))
            off = off | 1 if off + ln < block else off
            pieces.append((int(rng.integers(0, n_src)), off, ln))
            room -= ln
        pages.append((first, len(pieces) - first, block))
    return pages, pieces


def device_copy_ms(eng, nbytes, rounds):
    """hipMemcpyAsync device-to-device of nbytes between two events, ms per round."""
    hip = ctypes.CDLL("libamdhip64.so")
    P = ctypes.c_void_p
    hip.hipEventCreate.argtypes = [ctypes.POINTER(P)]
    hip.hipEventRecord.argtypes = [P, P]
    hip.hipEventSynchronize.argtypes = [P]
    hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), P, P]
    hip.hipEventDestroy.argtypes = [P]
    hip.hipMemcpyAsync.argtypes = [P, P, ctypes.c_size_t, ctypes.c_int, P]
    a, b = eng.alloc(nbytes), eng.alloc(nbytes)
    e0, e1 = P(), P()
    assert hip.hipEventCreate(ctypes.byref(e0)) == 0 and hip.hipEventCreate(ctypes.byref(e1)) == 0
    out = []
    for _ in range(rounds):
        assert hip.hipEventRecord(e0, None) == 0
        assert hip.hipMemcpyAsync(b.ptr, a.ptr, nbytes, 3, None) == 0  # hipMemcpyDeviceToDevice
        assert hip.hipEventRecord(e1, None) == 0
        assert hip.hipEventSynchronize(e1) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1) == 0
        out.append(ms.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    a.free()
    b.free()
    return out


def gather_alone_ms(eng, E, blocks, pages, pieces, rounds):
    """gather_pages_k over the pieces in device memory, ms per launch."""
    block = len(blocks[0])
    sbuf, dbuf = eng.alloc(block * len(blocks)), eng.alloc(block * len(pages))
    gs = (E.jfsx_gsrc * len(blocks))()
    for i, b in enumerate(blocks):
        sbuf.upload(b, offset=i * block)
        gs[i].data, gs[i].len = sbuf.ptr + i * block, block
    gd = (E.jfsx_gdst * len(pages))()
    for j, (first, count, n) in enumerate(pages):
        gd[j].data, gd[j].len, gd[j].piece_first, gd[j].piece_count = dbuf.ptr + j * block, n, first, count
    pa, n_piece = E.make_pieces(pieces)
    eng.set_timing(True)
    out = []
    for _ in range(rounds):
        eng.kernel_time(reset=True)
        eng.gather_batch(len(blocks), gs, len(pages), gd, n_piece, pa, E.MEM_DEVICE)
        out.append(eng.kernel_time(reset=True)[0])
    eng.set_timing(False)
    got = dbuf.download(block, offset=0)
    sbuf.free()
    dbuf.free()
    return out, got


def run_case(eng, E, dk, e, blocks, pages, pieces, codec, reps, warmup):
    algo = E.AES256GCM
    n_src, n_dst = len(blocks), len(pages)
    block = len(blocks[0])
    draw = lambda seed, i: (bytes(E.gen_key(seed, i)[0]), bytes(E.gen_key(seed + 1, i)[0]),  # noqa: E731
                            bytes(E.gen_key(seed, i)[1]))
    # the stored source objects, made once
    made = eng.store_objects(dk, e, algo, codec, [draw(0xC0A, i) + (b,) for i, b in enumerate(blocks)], crc=False)
    assert all(st == E.OK for st, _, _, _ in made)
    objs = [np.frombuffer(o, np.uint8).copy() for _, o, _, _ in made]
    expect = [int(c) for _, _, _, c in made]
    draws = [draw(0xC0C, j) for j in range(n_dst)]
    caps = [E.object_bound(codec, n) for _, _, n in pages]
    nseg = [max(1, -(-n // E.SEG)) for _, _, n in pages]

    def src_specs(dst):
        return [{"hdr": o.ctypes.data, "hdr_len": HDR, "tag": o[-TAG:].tobytes(), "src": o.ctypes.data + HDR,
                 "src_len": o.size - HDR - TAG, "dst": dst[i].ctypes.data if dst else None, "len": block,
                 "expect_crc": expect[i]} for i, o in enumerate(objs)]

    def dst_specs(obj, crc, src):
        return [{"key": k, "seed": s, "nonce": nn, "src": src[j].ctypes.data if src else None, "len": pages[j][2],
                 "obj": obj[j].ctypes.data, "obj_cap": caps[j], "crc": crc[j].ctypes.data}
                for j, (k, s, nn) in enumerate(draws)]

    # one call
    obj1 = [np.empty(c, np.uint8) for c in caps]
    crc1 = [np.empty(4 * k, np.uint8) for k in nseg]
    oarr1, _ = eng.make_oblocks(src_specs(None))
    sarr1, _ = eng.make_soblocks(dst_specs(obj1, crc1, None))
    cp = (E.jfsx_cpage * n_dst)()
    for j, (first, count, _) in enumerate(pages):
        cp[j].piece_first, cp[j].piece_count = first, count
    pa, n_piece = E.make_pieces(pieces)
    # the separate calls
    spage = [np.empty(block, np.uint8) for _ in range(n_src)]
    dpage = [np.empty(n, np.uint8) for _, _, n in pages]
    obj2 = [np.empty(c, np.uint8) for c in caps]
    crc2 = [np.empty(4 * k, np.uint8) for k in nseg]
    oarr2, _ = eng.make_oblocks(src_specs(spage))
    sarr2, _ = eng.make_soblocks(dst_specs(obj2, crc2, dpage))

    def one():
        eng.compact_objects_batch(dk, e, algo, codec, n_src, oarr1, E.CRC_CT, n_dst, sarr1, cp, E.CRC_GEN | E.CRC_CT,
                                  n_piece, pa)

    def seq():
        eng.load_objects_batch(dk, algo, codec, oarr2, n_src, E.CRC_CT, E.MEM_HOST)
        for j, (first, count, _) in enumerate(pages):
            at, page = 0, dpage[j]
            for s, off, ln in pieces[first:first + count]:
                if s < 0:
                    page[at:at + ln] = 0
                else:
                    page[at:at + ln] = spage[s][off:off + ln]
                at += ln
        eng.store_objects_batch(dk, e, algo, codec, sarr2, n_dst, E.CRC_GEN | E.CRC_CT, E.MEM_HOST)

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
    for i in range(n_src):
        assert oarr1[i].status == oarr2[i].status == E.OK and oarr1[i].obj_crc == oarr2[i].obj_crc == expect[i], i
    for j in range(n_dst):
        a, b = sarr1[j], sarr2[j]
        assert a.status == b.status == E.OK and cp[j].src_bad == -1, j
        assert (a.out_len, a.img_len, a.obj_crc) == (b.out_len, b.img_len, b.obj_crc), j
        assert obj1[j][:a.out_len].tobytes() == obj2[j][:a.out_len].tobytes(), j
        assert crc1[j].tobytes() == crc2[j].tobytes(), j
    img_in = sum(o.size - HDR - TAG for o in objs)
    out_b = sum(int(sarr1[j].out_len) for j in range(n_dst))
    pg_in, pg_out = n_src * block, sum(n for _, _, n in pages)
    crc_b = 4 * sum(nseg)
    row = {"source_image_bytes": img_in, "source_page_bytes": pg_in, "new_page_bytes": pg_out, "object_bytes": out_b,
           "one": spread(t["one"]), "seq": spread(t["seq"]),
           "one_cpu": spread(cpu["one"]), "seq_cpu": spread(cpu["seq"]),
           # over PCIe, from the shapes: wrapped keys 256 per source up, keys and seeds 64 per page up
           "one_bytes_h2d": img_in + 256 * n_src + 64 * n_dst, "one_bytes_d2h": out_b + crc_b,
           "seq_bytes_h2d": img_in + 256 * n_src + pg_out + 64 * n_dst, "seq_bytes_d2h": pg_in + out_b + crc_b}
    row["one_new_page_GBps"] = round(pg_out / (row["one"]["median_ms"] * 1e-3) / 1e9, 2)
    row["seq_new_page_GBps"] = round(pg_out / (row["seq"]["median_ms"] * 1e-3) / 1e9, 2)
    row["one_over_seq"] = round(row["one"]["median_ms"] / row["seq"]["median_ms"], 3)
    row["one_over_seq_cpu"] = round(row["one_cpu"]["median_ms"] / row["seq_cpu"]["median_ms"], 3)
    row["ranges_overlap"] = not (row["one"]["max_ms"] < row["seq"]["min_ms"] or
                                 row["seq"]["max_ms"] < row["one"]["min_ms"])
    return row, dpage[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=64)
    ap.add_argument("--sources", type=int, default=80)
    ap.add_argument("--block-mib", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codecs", default="none,lz4,zstd")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact", "compact_rate.json"))
    a = ap.parse_args()
    reps, warmup = max(a.reps, 5), max(a.warmup, 1)
    from juicefs_amd import engine as E
    from tests import lz4_data
    from tests import rsa_model as M
    block = a.block_mib * MIB
    blocks = [lz4_data.sample("text", block, seed=100 + i) for i in range(a.sources)]
    pages, pieces = make_pieces(np.random.default_rng(0xC0AC), a.pages, a.sources, block)
    hole = sum(n for s, _, n in pieces if s < 0)
    eng = E.Engine(0)
    dk = eng.rsa_key(*M.components(M.fixed_keys()["plain_p_gt_q"]))
    out = {"tool": "compact_rate", "pages": a.pages, "sources": a.sources, "block_mib": a.block_mib, "kind": "text",
           "mem": "host", "cipher": "aes256gcm", "src_crc_mode": "CT", "dst_crc_mode": "GEN|CT", "reps": reps,
           "warmup": warmup, "pieces": len(pieces), "hole_bytes": hole,
           "hole_share": round(hole / (a.pages * block), 4), "cases": {}}
    codecs = {"none": E.CODEC_NONE, "lz4": E.CODEC_LZ4, "zstd": E.CODEC_ZSTD}
    page0 = None
    for cname in a.codecs.split(","):
        out["cases"][cname], page0 = run_case(eng, E, dk, M.E, blocks, pages, pieces, codecs[cname], reps, warmup)
    g, got = gather_alone_ms(eng, E, blocks, pages, pieces, warmup + reps)
    assert page0 is None or got.tobytes() == page0.tobytes()
    cpy = device_copy_ms(eng, a.pages * block, warmup + reps)
    total = a.pages * block
    out["gather"] = dict(spread(g[warmup:]), bytes=total, tile=E.GATHER_TILE)
    out["gather"]["GBps"] = round(total / (out["gather"]["median_ms"] * 1e-3) / 1e9, 1)
    out["device_copy"] = dict(spread(cpy[warmup:]), bytes=total)
    out["device_copy"]["GBps"] = round(total / (out["device_copy"]["median_ms"] * 1e-3) / 1e9, 1)
    out["gather_over_copy"] = round(out["gather"]["median_ms"] / out["device_copy"]["median_ms"], 3)
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
