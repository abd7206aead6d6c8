#!/usr/bin/env python3
"""Rate of the Hadoop file checksum (jfsx_file_checksum_batch) on device-resident
synthetic data, one JSON line.

Shapes (the same buffer, generated once with gen_synthetic_batch):
  files   --files files of --file-mib MiB each      (default 128 x 128 MiB)
  one     the whole buffer as one file               (default 16 GiB)
  block   the first file alone                       (one DFS block: the MD5
          phase's latency floor)
Per shape: --warmup calls, then the median of --reps (>= 5) timed calls of
  wall_ms     the whole call (chunk CRCs, block MD5s, download, host fold)
  crc_ms      the chunk-CRC kernel alone (set_timing / kernel_time)
  rest_ms     wall_ms - crc_ms: the MD5 launch, the download and the fold
and, in the same run over the same buffers, crc32c_segments GEN (wall and
kernel) with its run-to-run spread.  `host` is the same checksum on the CPU:
--host-procs processes, each hashing one block-sized file of its own with the
oracle's hardware CRC32C called per 512-byte chunk and hashlib's MD5 (a
per-chunk loop, like the reference's Java one; the ctypes call per chunk is
part of what it measures).
"""
import argparse
import hashlib
import json
import multiprocessing
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BPC = 512


def host_file_checksum(args):
    """one file of `nbytes` synthetic bytes: seconds for the MD5 of MD5s of its chunk CRCs"""
    seed, index, nbytes, block = args
    from oracle import oracle as orc
    data = orc.gen_block(seed, index, nbytes)
    t0 = time.perf_counter()
    per = block // BPC
    digs, crcs = [], bytearray()
    for i, o in enumerate(range(0, nbytes, BPC)):
        crcs += int(orc.crc32c(data[o:o + BPC], 0, True)).to_bytes(4, "big")
        if (i + 1) % per == 0:
            digs.append(hashlib.md5(crcs).digest())
            crcs = bytearray()
    if crcs:
        digs.append(hashlib.md5(crcs).digest())
    buf = b"".join(digs)
    hashlib.md5(buf + bytes(max(32, 1 << (len(buf) - 1).bit_length()) - len(buf))).digest()
    return time.perf_counter() - t0


def measure_host(procs, nbytes, block):
    ctx = multiprocessing.get_context("spawn")
    with ctx.Pool(procs) as pool:
        pool.map(host_file_checksum, [(7, i, 1 << 20, block) for i in range(procs)])  # start-up, imports
        t0 = time.perf_counter()
        each = pool.map(host_file_checksum, [(7, i, nbytes, block) for i in range(procs)])
        wall = time.perf_counter() - t0
    total = procs * nbytes
    return {"procs": procs, "bytes": total, "wall_ms": round(wall * 1e3, 2),
            "slowest_proc_ms": round(max(each) * 1e3, 2), "GBps": round(total / wall / 1e9, 3)}


def med(xs):
    return round(statistics.median(xs), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--file-mib", type=int, default=128)
    ap.add_argument("--block-mib", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-procs", type=int, default=16)
    ap.add_argument("--host-mib", type=int, default=128, help="bytes each host process hashes")
    a = ap.parse_args()
    reps = max(a.reps, 5)
    block = a.block_mib << 20
    fbytes = a.file_mib << 20
    total = a.files * fbytes

    # the host line first: its processes start before this one opens the GPU
    host = measure_host(a.host_procs, a.host_mib << 20, block) if a.host_procs else None

    from juicefs_amd import engine as E
    eng = E.Engine(0)
    buf = eng.alloc(total)
    eng.gen_synthetic_batch(buf, fbytes, [fbytes] * a.files, 0x4A465321, 0)
    eng.sync()
    nseg = total // E.SEG
    crcbuf = eng.alloc(4 * nseg)
    eng.set_timing(True)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        eng.kernel_time(reset=True)
        wall, kern = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
            kern.append(eng.kernel_time(reset=True)[0])
        return wall, kern

    shapes = {
        "files": [(buf.ptr + i * fbytes, fbytes) for i in range(a.files)],
        "one": [(buf.ptr, total)],
        "block": [(buf.ptr, fbytes)],
    }
    out = {"tool": "filechecksum_rate", "files": a.files, "file_mib": a.file_mib, "block_mib": a.block_mib,
           "bytes": total, "reps": reps, "warmup": a.warmup, "shapes": {}, "host": host}
    for name, files in shapes.items():
        nbytes = sum(n for _, n in files)
        res = []
        wall, kern = timed(lambda: res.append(eng.file_checksum_batch(files, block, mem=E.MEM_DEVICE)))
        assert all(r == res[0] for r in res)
        R = (E.jfsx_range * len(files))()
        o = 0
        for i, (p, n) in enumerate(files):
            R[i].data, R[i].len, R[i].crc = p, n, crcbuf.ptr + o
            o += 4 * (n // E.SEG)
        swall, skern = timed(lambda: eng.crc32c_segments(R, len(files), E.CRC_GEN, E.MEM_DEVICE))
        row = {
            "bytes": nbytes, "md5_blocks": sum(-(-n // block) for _, n in files),
            "wall_ms": med(wall), "crc_ms": med(kern), "rest_ms": med([w - k for w, k in zip(wall, kern)]),
            "crc_TBps": round(nbytes / (statistics.median(kern) * 1e-3) / 1e12, 3),
            "crc_ms_min_max": [round(min(kern), 4), round(max(kern), 4)],
            "call_GBps": round(nbytes / (statistics.median(wall) * 1e-3) / 1e9, 1),
            "segments_wall_ms": med(swall), "segments_crc_ms": med(skern),
            "segments_TBps": round(nbytes / (statistics.median(skern) * 1e-3) / 1e12, 3),
            "segments_crc_ms_min_max": [round(min(skern), 4), round(max(skern), 4)],
            "md5": res[0][0][3].hex(),
        }
        if host:
            row["host_ms_at_host_rate"] = round(nbytes / (host["GBps"] * 1e9) * 1e3, 1)
        out["shapes"][name] = row
    eng.set_timing(False)
    crcbuf.free()
    buf.free()
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
