"""Where gcm_main_k's time goes between the row loops, and where a step's
time goes around the kernel: a probe build of libjfsx with JFSX_KS_PHASES

    bash scripts/build_variant.sh KSP "jfsx_gcm.hip jfsx_api.cpp" -DJFSX_KS_PHASES

makes workgroup 0 stamp the 100 MHz clock through its first eight tasks (per
wave at "rows done" and "epilogue done"), and makes enqueue_aead / run_aead
stamp the host clock and record events around the upload, keysetup, finalize
and the copy-back.  This seals three device-resident batches (bench.py's
flagship, its --ragged batch, and 64 KiB blocks), a few warm-up calls and
then `reps` measured ones each, and writes per task and per batch the means
in microseconds as JSON.

Per task: `first_row` (queue-loop top to the first row: descriptor, basis, P,
table build, barriers), `rows_min` / `rows_max` (the fastest and the slowest
wave's rows), `skew` (their difference), `epilogue` (a wave's lift, reduce
and partial stores, mean and max), `sweep` (the slowest wave's epilogue end to
the task's end: barrier and shared-segment sweep), `gap` (the task's end to
the next task's first row).  `edge_share`: each host interval and stream
interval of the step, and the step's wall time against the main kernel's.

usage: JFSX_LIB=juicefs_amd/_build/libjfsx_KSP.so python3 tools/taskedge_probe.py OUT.json [reps] [flagship blocks]
           [batches, e.g. flagship,64KiB] [k]

k = 1..3 gives a task's rows, in equal runs, to the first 4k waves only (k
waves per SIMD; jfsx_debug_edge_waves): the CU's row rate at k resident waves
per SIMD, from which gcm_task's run weights by wave age were taken
(profiles/r11/taskedge/README.md has the arithmetic).  Results stay right.
"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from juicefs_amd import engine as E  # noqa: E402

TASKS, REC = 8, 40
HOST = ["plan_batch", "descriptor fill", "slot walk + dispatch", "enqueue upload", "enqueue keysetup",
        "enqueue main", "enqueue finalize + copy-back", "wait for the stream", "finish_aead"]
DEV = ["upload", "keysetup", "keysetup end to main start", "main kernel", "finalize", "copy-back"]
MIB = 1 << 20


def batches(flagship_blocks):
    return [("flagship", [4 * MIB] * flagship_blocks),
            ("ragged", [bench.ragged_len(bench.SEED, b, 4 * MIB) for b in range(flagship_blocks)]),
            ("64KiB", [65536] * 16384)]


def task_rows(ts, waves=16):
    """Microseconds of each recorded task's parts from workgroup 0's stamps (100 MHz ticks)."""
    out = []
    for k in range(TASKS):
        r = ts[8 + k * REC:8 + (k + 1) * REC]
        if r[1] == 0:
            break
        rows = [r[8 + w] - r[1] for w in range(waves)]
        epi = [r[24 + w] - r[8 + w] for w in range(waves)]
        last = max(r[24:24 + waves])
        nxt = ts[8 + (k + 1) * REC + 1] if k + 1 < TASKS else 0
        out.append({"bytes": int(r[3]), "blk": int(r[4] >> 32), "c0": int(r[4] & 0xffffffff) << 16,
                    "first_row": (r[1] - r[0]) * 0.01, "rows_min": min(rows) * 0.01, "rows_max": max(rows) * 0.01,
                    "skew": (max(rows) - min(rows)) * 0.01, "rows_by_wave": [x * 0.01 for x in rows],
                    "epilogue_mean": sum(epi) / waves * 0.01,
                    "epilogue_max": max(epi) * 0.01, "sweep": (r[2] - last) * 0.01,
                    "task": (r[2] - r[0]) * 0.01,
                    "gap": (nxt - r[2]) * 0.01 if nxt > r[2] else None})
    return out


def mean_dicts(ds):
    keys = [k for k in ds[0] if isinstance(ds[0][k], float)]
    out = dict(ds[0])
    for k in keys:
        vals = [d[k] for d in ds if d.get(k) is not None]
        out[k] = round(sum(vals) / len(vals), 3)
    out["rows_by_wave"] = [round(sum(d["rows_by_wave"][w] for d in ds) / len(ds), 1)
                           for w in range(len(ds[0]["rows_by_wave"]))]
    return out


def main():
    path = sys.argv[1]
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    fb = int(sys.argv[3]) if len(sys.argv) > 3 else 16384
    eng = E.Engine()
    mf, hf = eng.L.jfsx_debug_main_phases, eng.L.jfsx_debug_edge_host
    mf.argtypes = hf.argtypes = [ctypes.c_void_p]
    ts = (ctypes.c_ulonglong * (8 + TASKS * REC))()
    hs = (ctypes.c_double * 15)()
    eng.set_timing(True)
    result = {"library": os.path.basename(E.LIB_PATH), "reps": reps, "unit": "us"}
    only = sys.argv[4].split(",") if len(sys.argv) > 4 else None
    if len(sys.argv) > 5:
        assert eng.L.jfsx_debug_edge_waves(int(sys.argv[5])) == 0
    result["waves_per_simd"] = int(sys.argv[5]) if len(sys.argv) > 5 else 4
    for name, lens in batches(fb):
        if only and name not in only:
            continue
        nb, L = len(lens), -(-max(lens) // 4096) * 4096  # the blocks' stride
        nseg = -(-L // E.SEG)
        src, dst, crc = eng.alloc(nb * L), eng.alloc(nb * L), eng.alloc(nb * 4 * nseg)
        eng.gen_synthetic_batch(src, L, lens, bench.SEED, 0)
        specs = []
        for b in range(nb):
            key, nonce = E.gen_key(bench.SEED, b)
            specs.append({"key": key, "nonce": nonce, "src": src.ptr + b * L, "dst": dst.ptr + b * L, "len": lens[b],
                          "crc": crc.ptr + 4 * nseg * b})
        blks, n = eng.make_blocks(specs)
        tasks, host, steps = [], [], []
        for r in range(reps + 2):
            eng.kernel_time()
            t0 = time.perf_counter()
            eng.seal_batch(E.AES256GCM, blks, n, E.CRC_GEN, E.MEM_DEVICE)
            wall = (time.perf_counter() - t0) * 1e6
            if r < 2:
                continue
            assert mf(ts) == 0 and hf(hs) == 0
            tasks.append(task_rows(list(ts)))
            host.append(list(hs))
            steps.append((wall, eng.kernel_time()[0] * 1e3))
        per_task = [mean_dicts([t[k] for t in tasks]) for k in range(min(len(t) for t in tasks))]
        hmean = [sum(h[i] for h in host) / reps for i in range(15)]
        wall, kern = sum(s[0] for s in steps) / reps, sum(s[1] for s in steps) / reps
        share = {"step_wall": round(wall, 1), "main_kernel": round(kern, 1), "outside_kernel": round(wall - kern, 1),
                 "host": {k: round(v, 1) for k, v in zip(HOST, hmean[:9])},
                 "stream": {k: round(v, 1) for k, v in zip(DEV, hmean[9:])}}
        tb, _, plan = E.debug_plan(E.PLAN_GCM, lens)
        result[name] = {"blocks": nb, "bytes": sum(lens), "task_bytes": tb, "ntasks": len(plan), "tasks": per_task,
                        "edge_share": share}
        print(name, json.dumps(result[name]), flush=True)
        for b in (src, dst, crc):
            b.free()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
    eng.close()


if __name__ == "__main__":
    main()
