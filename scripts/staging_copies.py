#!/usr/bin/env python3
"""The PCIe copies of the one-call paths' host staging, per call and layout.

  run      issues the five-block batch of tests/test_gpu_mixed_staging.py once
           per layout (all pageable, all pinned, mixed) on each of the six
           calls, every result checked as the test checks it.  Meant to run
           under a copy trace of its own (no counters in the same run):

             rocprofv3 --memory-copy-trace --output-format json -d DIR -o run \\
                 -- python3 scripts/staging_copies.py run

           A warm-up pass grows every workspace first.  In the measured pass
           each call stands between two marker copies, host to device, of
           MARK + k bytes (k counts the calls), sizes no batch has.
  table    reads DIR/**/*_results.json of such a run and prints, per call and
           layout, the number of copies and the bytes in each direction:

             python3 scripts/staging_copies.py table DIR

The tables of two builds are compared with diff: the staging is host
bookkeeping, so any difference is a difference in what the engine copies.
"""
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MARK = 7700000
P, G = "pinned", "pageable"
MIXED = [(P, G), (G, G), (P, P), (G, P), (P, P)]
LAYOUTS = [("pageable", [(G, G)] * 5), ("pinned", [(P, P)] * 5), ("mixed", MIXED)]
CALLS = ["load_batch", "load_objects", "store_batch", "store_objects", "gather_batch", "open_range_batch"]


def segments(T):
    """(call, case id, layout, kinds) of every measured call, in order."""
    return [(call, case[0] if case else "-", name, kinds) for call in CALLS for case in T.CALLS[call][1]
            for name, kinds in LAYOUTS]


def run():
    from juicefs_amd import engine as E
    from tests import rsa_model as M
    from tests import test_gpu_mixed_staging as T
    assert T.MIXED == MIXED
    eng = E.Engine(0)
    dkey = eng.rsa_key(*M.components(M.fixed_keys()[T.LO.KEY_A]))
    arenas = T.Arenas(eng)
    cases = {(call, case[0] if case else "-"): case for call in CALLS for case in T.CALLS[call][1]}
    # page-locked, so that a marker is one DMA copy and not the runtime's staged chunks
    marker, pinned = eng.alloc(MARK + 4096), eng.alloc_pinned(MARK + 4096)
    k = [0]

    def mark():
        eng._check(eng.L.jfsx_memcpy_h2d(eng.ctx, marker.ptr, pinned, MARK + k[0]), "h2d")
        k[0] += 1

    for measured in (False, True):
        for call, cid, _, kinds in segments(T):
            T.CALLS[call][0](eng, arenas, cases[(call, cid)], kinds, dkey=dkey, mark=mark if measured else lambda: None)
    marker.free()
    eng.free_pinned(pinned)
    arenas.close()
    eng.rsa_key_free(dkey)
    eng.close()
    print(json.dumps({"tool": "staging_copies", "calls": k[0] // 2}))


def copies(d):
    """(direction, bytes) of every copy of a trace, in order of its start."""
    out = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*results.json"), recursive=True)):
        for tool in json.load(open(f))["rocprofiler-sdk-tool"]:
            names = {}
            for kind in tool.get("strings", {}).get("buffer_records", []):
                if "MEMORY_COPY" in kind.get("kind", ""):
                    names = dict(enumerate(kind.get("operations", [])))
            for r in tool["buffer_records"].get("memory_copy", []):
                op = names.get(r["operation"], str(r["operation"])).replace("MEMORY_COPY_", "")
                out.append((r["start_timestamp"], op, r["bytes"]))
    return [(op, b) for _, op, b in sorted(out)]


def table(d):
    from tests import test_gpu_mixed_staging as T
    segs, seq = segments(T), copies(d)
    rows, cur, k = {}, None, 0
    for op, b in seq:
        if MARK <= b < MARK + 2 * len(segs) and b == MARK + k:
            cur = None if k % 2 else segs[k // 2][:3]
            k += 1
            if cur:
                rows[cur] = {}
            continue
        if cur:
            n, total = rows[cur].get(op, (0, 0))
            rows[cur][op] = (n + 1, total + b)
    assert k == 2 * len(segs), "markers found: %d of %d" % (k, 2 * len(segs))
    ops = sorted({op for r in rows.values() for op in r})
    print("| call | case | layout | " + " | ".join("%s copies | %s bytes" % (op, op) for op in ops) + " |")
    print("|---|---|---|" + "---:|---:|" * len(ops))
    for seg in (s[:3] for s in segs):
        print("| %s | %s | %s | " % seg + " | ".join("%d | %d" % rows[seg].get(op, (0, 0)) for op in ops) + " |")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    elif len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    else:
        sys.exit(__doc__)
