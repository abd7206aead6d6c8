"""Child process of tests/test_gpu_rsa_fixed.py: unwraps the batches of a job
file on the GPU and prints the results as JSON, judging nothing itself.  The
engine reads JFSX_RSA_PAIR once per process, so the one-lane kernel can only
be reached from a process started with it set.

usage: python tests/rsa_unwrap_child.py JOBS.json
  in:  [{"comps": [5 x hex], "label": hex, "batches": [[hex ciphertext, ...], ...]}, ...]
  out: one line "RESULT " + JSON {"pair_env": the switch as this process saw it,
       "results": per job, per batch, per item the hex message or null}
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    from juicefs_amd import engine as E
    with open(sys.argv[1]) as f:
        jobs = json.load(f)
    eng = E.Engine(0)
    out = []
    try:
        for job in jobs:
            dk = eng.rsa_key(*(bytes.fromhex(c) for c in job["comps"]), label=bytes.fromhex(job["label"]))
            try:
                out.append([[None if r is None else r.hex()
                             for r in eng.oaep_decrypt_batch(dk, [bytes.fromhex(c) for c in batch])]
                            for batch in job["batches"]])
            finally:
                eng.rsa_key_free(dk)
    finally:
        eng.close()
    print("RESULT " + json.dumps({"pair_env": os.environ.get("JFSX_RSA_PAIR"), "results": out}))


if __name__ == "__main__":
    main()
