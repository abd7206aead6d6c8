"""Child process of tests/test_gpu_zstd_exec.py: decodes the corpus and the
rejects of tests/zstd_frames.py on the GPU (host-memory batches) and prints the
results as JSON, judging nothing itself.  The engine reads JFSX_ZSTD_SERIAL
once per process, so the serial kernel can only be chosen for a whole batch
from a process started with it set.

usage: python tests/zstd_serial_child.py
  out: one line "RESULT " + JSON {"serial_env": the switch as this process saw it,
       "corpus": per frame [status, sha256 of the output, reserved],
       "rejects": per reject [status, out_len], "zstd_serial": the metric after the corpus}
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from juicefs_amd import engine as E
    from tests import zstd_frames as Z
    eng = E.Engine(0)
    try:
        cs = Z.corpus()
        eng.metrics(reset=True)
        got = eng.zstd_decompress([c.frame for c in cs], [len(c.out) for c in cs])
        corpus = [[st, hashlib.sha256(d).hexdigest(), int(r)] for (st, d), r in zip(got, eng.zstd_serial_reasons)]
        serial = eng.metrics()["zstd_serial"]
        rj = Z.rejects()
        rejects = [[st, len(d)] for st, d in eng.zstd_decompress([f for _, f, _ in rj], [cap for _, _, cap in rj])]
    finally:
        eng.close()
    print("RESULT " + json.dumps({"serial_env": os.environ.get("JFSX_ZSTD_SERIAL"), "corpus": corpus,
                                  "rejects": rejects, "zstd_serial": serial}))


if __name__ == "__main__":
    main()
