#!/usr/bin/env python3
"""Time of the ranged Open (jfsx_open_range_batch) beside what a caller had
before it: jfsx_open_batch on the same blocks, and the slice taken afterwards.
One process, one GPU, one context; one JSON line, also written to
profiles/range/range_rate.json.

Both ciphers, windows of 4 KiB, 128 KiB and len / 4 at off = 1 MiB + 5 of 4 MiB
blocks (--len), every block with its own key, nonce and valid tag (the blocks
are sealed on the device first):
  device  --blocks (1024) device-resident blocks: jfsx_open_batch into a second
          buffer against jfsx_open_range_batch into one window per block
  host    --host-blocks (64) blocks of pageable memory: jfsx_open_batch with
          MEM_HOST plus a copy of the slice, against the ranged call
  agg     the same 64 blocks one per call from --threads (20) threads:
          jfsx_agg_open plus the slice against jfsx_agg_open_range
The two sides alternate, --warmup rounds and then --reps (>= 10) timed rounds
each, a host clock around the synchronous calls; the medians with their
min-max spread, and ratio = baseline / ranged (above 1: the ranged call is
ahead).  Before anything is reported the ranged windows of the last round are
compared with the slices of jfsx_open_batch's output.

--kernels-only runs the device part alone with few rounds and writes nothing:
the run to put under a kernel trace for the auth kernels' own time."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from juicefs_amd import engine as E  # noqa: E402

MIB = 1 << 20
ALGOS = [("aes256gcm", E.AES256GCM), ("chacha20", E.CHACHA20P1305)]
SEED = 0x52414E47


def stat(ts):
    return {"median_ms": round(statistics.median(ts) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4),
            "max_ms": round(max(ts) * 1e3, 4)}


def alternate(base, ranged, warmup, reps):
    tb, tr = [], []
    for r in range(warmup + reps):
        for fn, acc in ((base, tb), (ranged, tr)):
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if r >= warmup:
                acc.append(dt)
    b, g = stat(tb), stat(tr)
    return {"open_batch": b, "open_range": g, "ratio": round(b["median_ms"] / g["median_ms"], 3)}


def device_part(eng, algo, nblk, blen, windows, off, warmup, reps):
    src, dst = eng.alloc(nblk * blen), eng.alloc(nblk * blen)
    wmax = max(windows)
    win = eng.alloc(nblk * wmax)
    keys = [E.gen_key(SEED, i) for i in range(nblk)]
    eng.gen_synthetic_batch(dst, blen, [blen] * nblk, SEED, 0)
    seal, n = eng.make_blocks([{"key": k, "nonce": nc, "src": dst.ptr + i * blen, "dst": src.ptr + i * blen,
                                "len": blen} for i, (k, nc) in enumerate(keys)])
    eng.seal_batch(algo, seal, n, E.CRC_NONE, E.MEM_DEVICE)
    tags = [bytes(seal[i].tag) for i in range(n)]
    blks, _ = eng.make_blocks([{"key": k, "nonce": nc, "tag": tags[i], "src": src.ptr + i * blen,
                                "dst": dst.ptr + i * blen, "len": blen} for i, (k, nc) in enumerate(keys)])
    out = {}
    for w in windows:
        rb, _ = eng.make_rblocks([{"key": k, "nonce": nc, "tag": tags[i], "src": src.ptr + i * blen, "len": blen,
                                   "off": off, "limit": w, "dst": win.ptr + i * wmax, "dst_cap": w}
                                  for i, (k, nc) in enumerate(keys)])
        res = alternate(lambda: eng.open_batch(algo, blks, n, E.CRC_NONE, E.MEM_DEVICE),
                        lambda: eng.open_range_batch(algo, rb, n, E.CRC_NONE, E.MEM_DEVICE), warmup, reps)
        assert all(blks[i].status == E.OK and rb[i].status == E.OK and rb[i].out_len == w for i in range(n))
        for i in (0, n // 2, n - 1):
            assert win.download(w, i * wmax).tobytes() == dst.download(w, i * blen + off).tobytes(), (w, i)
        res["bytes_authenticated"] = nblk * blen
        out[str(w)] = res
    for b in (src, dst, win):
        b.free()
    return out


def host_part(eng, algo, nblk, blen, windows, off, warmup, reps, threads):
    keys = [E.gen_key(SEED + 1, i) for i in range(nblk)]
    rng = np.random.default_rng(SEED)
    plain = [rng.integers(0, 256, blen, dtype=np.uint8) for _ in range(nblk)]
    ct = [np.empty(blen, np.uint8) for _ in range(nblk)]
    full = [np.empty(blen, np.uint8) for _ in range(nblk)]
    seal, n = eng.make_blocks([{"key": k, "nonce": nc, "src": plain[i].ctypes.data, "dst": ct[i].ctypes.data,
                                "len": blen} for i, (k, nc) in enumerate(keys)])
    eng.seal_batch(algo, seal, n, E.CRC_NONE, E.MEM_HOST)
    tags = [bytes(seal[i].tag) for i in range(n)]
    blks, _ = eng.make_blocks([{"key": k, "nonce": nc, "tag": tags[i], "src": ct[i].ctypes.data,
                                "dst": full[i].ctypes.data, "len": blen} for i, (k, nc) in enumerate(keys)])
    out = {"batch": {}, "agg": {}}
    for w in windows:
        wins = [np.empty(w, np.uint8) for _ in range(nblk)]
        rb, _ = eng.make_rblocks([{"key": k, "nonce": nc, "tag": tags[i], "src": ct[i].ctypes.data, "len": blen,
                                   "off": off, "limit": w, "dst": wins[i].ctypes.data, "dst_cap": w}
                                  for i, (k, nc) in enumerate(keys)])
        sliced = [None] * nblk

        def base():
            eng.open_batch(algo, blks, n, E.CRC_NONE, E.MEM_HOST)
            for i in range(nblk):
                sliced[i] = full[i][off:off + w].copy()

        res = alternate(base, lambda: eng.open_range_batch(algo, rb, n, E.CRC_NONE, E.MEM_HOST), warmup, reps)
        for i in range(nblk):
            assert rb[i].status == E.OK and rb[i].out_len == w
            assert wins[i].tobytes() == sliced[i].tobytes() == plain[i][off:off + w].tobytes(), (w, i)
        out["batch"][str(w)] = res

        # one block per call from `threads` threads, through the aggregator
        agg = E.Aggregator(eng, max_bytes=16 * MIB)

        def fan(work):
            def body(t):
                for i in range(t, nblk, threads):
                    work(i)
            ts = [threading.Thread(target=body, args=(t,)) for t in range(threads)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()

        def agg_base(i):
            agg.open(algo, blks[i], E.CRC_NONE, E.MEM_HOST)
            sliced[i] = full[i][off:off + w].copy()

        try:
            res = alternate(lambda: fan(agg_base),
                            lambda: fan(lambda i: agg.open_range(algo, rb[i], E.CRC_NONE, E.MEM_HOST)), warmup, reps)
        finally:
            agg.close()
        for i in range(nblk):
            assert rb[i].status == E.OK and wins[i].tobytes() == sliced[i].tobytes(), (w, i)
        out["agg"][str(w)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=1024)
    ap.add_argument("--host-blocks", type=int, default=64)
    ap.add_argument("--len", type=int, default=4 * MIB)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "range", "range_rate.json"))
    a = ap.parse_args()
    blen, off = a.len, MIB + 5
    windows = [4096, 128 << 10, blen // 4]
    reps, warmup = (2, 1) if a.kernels_only else (max(a.reps, 10), max(a.warmup, 1))
    eng = E.Engine(0)
    res = {"block_bytes": blen, "off": off, "windows": windows, "device_blocks": a.blocks,
           "host_blocks": a.host_blocks, "threads": a.threads, "reps": reps, "warmup": warmup,
           "rule": "ratio = open_batch median / open_range median", "device": {}, "host": {}, "agg": {}}
    try:
        for name, algo in ALGOS:
            res["device"][name] = device_part(eng, algo, a.blocks, blen, windows, off, warmup, reps)
            if not a.kernels_only:
                h = host_part(eng, algo, a.host_blocks, blen, windows, off, warmup, reps, a.threads)
                res["host"][name], res["agg"][name] = h["batch"], h["agg"]
    finally:
        eng.close()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if not a.kernels_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
