#!/usr/bin/env python3
"""Time of the batched RSA-OAEP unwrap and wrap with a 4096-bit key
(jfsx_rsa_oaep_decrypt_batch / _encrypt_batch) on one GPU, beside the same
operations through libcrypto on --threads (16) host threads, which is what a
4096-bit volume had before the engine took such keys; one JSON line, also
written to profiles/rsa4096/rsa4096_rate.json.

Workload: --keys (16384) data keys of 32 bytes with their OAEP seeds, from a
fixed stream, under one fixed RSA-4096 key of tests/golden/rsa_keys_4096.json
(e = 65537, label "keys").  In one process and on one context, alternating
wrap / unwrap: --warmup rounds, then the median of --reps (>= 5) rounds with
the min-max spread.  The GPU figures are wall times of the whole call: both
calls take and give host memory, so the copies over PCIe (8 MiB of ciphertext
one way, the messages the other) are inside.  host: RsaEncryptor.Decrypt /
Encrypt (a fresh EVP_PKEY_CTX per call, what the host path pays per object) over
all --keys items, split over the threads (libcrypto runs outside the
interpreter lock).

Before anything is reported every wrapped key of the last round has come back
through the GPU unwrap as its data key; the first items are also checked
against the model and libcrypto."""
import argparse
import concurrent.futures
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.rsa_wrap_rate import pem_of, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, default=16384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--key-name", default="plain_q_gt_p")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rsa4096", "rsa4096_rate.json"))
    a = ap.parse_args()
    reps, warmup, n, K = max(a.reps, 5), max(a.warmup, 1), a.keys, 512
    from juicefs_amd import encrypt as enc
    from juicefs_amd import engine as E
    from tests import rsa_model_wide as M
    k = M.fixed_keys()[a.key_name]
    rng = np.random.default_rng(0x4096)
    msgs = rng.integers(0, 256, n * 32, dtype=np.uint8)
    seeds = rng.integers(0, 256, n * 32, dtype=np.uint8)
    lens = np.full(n, 32, np.uint32)
    ct = np.zeros(n * K, np.uint8)
    st = np.zeros(n, np.int32)
    ctlens = np.full(n, K, np.uint32)
    back = np.zeros(n * 32, np.uint8)
    blen = np.zeros(n, np.int32)
    eng = E.Engine(0)
    dk = eng.rsa_key(*M.components(k))
    assert E.rsa_key_bytes(dk) == K

    def wrap():
        eng._check(eng.L.jfsx_rsa_oaep_encrypt_batch(eng.ctx, dk, M.E, n, msgs.ctypes.data, 32, lens.ctypes.data,
                                                     seeds.ctypes.data, ct.ctypes.data, K, st.ctypes.data),
                   "jfsx_rsa_oaep_encrypt_batch")

    def unwrap():
        eng._check(eng.L.jfsx_rsa_oaep_decrypt_batch(eng.ctx, dk, n, ct.ctypes.data, K, ctlens.ctypes.data,
                                                     back.ctypes.data, 32, blen.ctypes.data),
                   "jfsx_rsa_oaep_decrypt_batch")

    t_wrap, t_unwrap = [], []
    for r in range(warmup + reps):
        ct[:] = 0
        back[:] = 0
        for fn, acc in ((wrap, t_wrap), (unwrap, t_unwrap)):
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                acc.append(dt)
    assert not st.any() and (blen == 32).all() and (back == msgs).all()
    rsae = enc.NewRSAEncryptor(enc.ParseRsaPrivateKeyFromPem(pem_of(k, M.E)))
    for i in range(4):
        m, s = msgs[32 * i:32 * i + 32].tobytes(), seeds[32 * i:32 * i + 32].tobytes()
        c = ct[K * i:K * i + K].tobytes()
        assert c == M.encrypt(k, m, s) and rsae.Decrypt(c) == m
    eng.rsa_key_free(dk)
    eng.close()

    # the host: the same n operations on the threads, in equal shares
    cts = [ct[K * i:K * i + K].tobytes() for i in range(n)]
    plain = [msgs[32 * i:32 * i + 32].tobytes() for i in range(n)]
    shares = [range(t, n, a.threads) for t in range(a.threads)]

    def host(fn, items, check):
        def work(share):
            return all(fn(items[i]) == check[i] if check else len(fn(items[i])) == K for i in share)
        with concurrent.futures.ThreadPoolExecutor(a.threads) as pool:
            t0 = time.perf_counter()
            ok = list(pool.map(work, shares))
            dt = (time.perf_counter() - t0) * 1e3
        assert all(ok)
        return dt
    host_unwrap_ms = host(rsae.Decrypt, cts, plain)
    host_wrap_ms = host(rsae.Encrypt, plain, None)
    w, u = spread(t_wrap), spread(t_unwrap)
    out = {"tool": "rsa4096_rate", "keys": n, "key_bytes": 32, "rsa_bits": 4096, "rsa_key": a.key_name, "e": M.E,
           "reps": reps, "warmup": warmup, "mem": "host", "gpu_time": "wall time of the call, copies included",
           "gpu_unwrap_ms_per_batch": u["median_ms"], "gpu_unwrap_ms_min": u["min_ms"], "gpu_unwrap_ms_max": u["max_ms"],
           "gpu_unwraps_per_s": round(n / (u["median_ms"] * 1e-3)),
           "gpu_wrap_ms_per_batch": w["median_ms"], "gpu_wrap_ms_min": w["min_ms"], "gpu_wrap_ms_max": w["max_ms"],
           "gpu_wraps_per_s": round(n / (w["median_ms"] * 1e-3)),
           "host_threads": a.threads, "host_cpus": os.cpu_count(),
           "host_unwrap_ms_per_batch": round(host_unwrap_ms, 1), "host_wrap_ms_per_batch": round(host_wrap_ms, 1),
           "host_unwrap_ms_per_op_per_thread": round(host_unwrap_ms * a.threads / n, 4),
           "unwrap_host_over_gpu": round(host_unwrap_ms / u["median_ms"], 2),
           "wrap_host_over_gpu": round(host_wrap_ms / w["median_ms"], 2),
           "gpu_unwrap_beats_host_threads": u["median_ms"] < host_unwrap_ms,
           "gpu_wrap_beats_host_threads": w["median_ms"] < host_wrap_ms,
           "verified": "all %d wraps through the GPU unwrap; 4 against the model and libcrypto; every host result" % n}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
