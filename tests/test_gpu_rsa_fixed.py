"""The GPU RSA-OAEP key unwrap (jfsx_rsa.hip: rsa_pair_k / rsa_half_k,
rsa_finish_k) against the big-integer model of tests/rsa_model.py on the fixed
keys of tests/golden/rsa_keys.json: q > p as well as p > q, primes at both
ends of the 1024-bit range, short ciphertexts, range edges, every OAEP
failure, batch sizes around the workgroup bounds, workspace reuse, the raw
C-ABI and the key checks.

Every test here hands the key to Engine.rsa_key and the ciphertexts to
Engine.oaep_decrypt_batch or jfsx_rsa_oaep_decrypt_batch itself: there is no
host unwrap to fall back to, and no libcrypto."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from juicefs_amd import encrypt as enc
from juicefs_amd import engine as E
from tests import rsa_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FIXED = list(M.fixed_keys())
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


class DevKey:
    """A device key that frees itself and checks that the free succeeds."""

    def __init__(self, eng, k, label=b"keys"):
        self.eng, self.h = eng, eng.rsa_key(*M.components(k), label=label)
        assert self.h

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        assert self.eng.L.jfsx_rsa_key_free(self.h) == 0


def check(name, cases, got):
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == c.expect, "key %s, case %r (%d-byte ciphertext)" % (name, c.name, len(c.ct))


def mixed_batch(name, n):
    """n cases of one key, valid and invalid in turn; the last one is valid,
    and neither its ciphertext nor its message occurs anywhere else in the
    batch."""
    cs = M.case_set(name)
    good = [c for c in cs if c.name.startswith("valid len")]  # not the short forms: they share one message
    bad = [c for c in cs if c.expect is None]
    last = good.pop()
    out = [good[i % len(good)] if i % 2 == 0 else bad[(i // 2) % len(bad)] for i in range(n - 1)] + [last]
    assert last.expect and all(c.ct != last.ct and c.expect != last.expect for c in out[:-1])
    return out


# ---- 1. every fixed key, the whole ciphertext set in one batch --------------
@pytest.mark.parametrize("name", FIXED)
def test_fixed_key_matches_model(eng, name):
    assert os.environ.get("JFSX_RSA_PAIR") != "0"  # this process runs rsa_pair_k; the one-lane kernel is test 7
    M.assert_reaches_paths(name)  # from the model alone, before the engine is looked at
    k = M.fixed_keys()[name]
    with DevKey(eng, k) as dk:
        cases = M.case_set(name)
        check(name, cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))
    with DevKey(eng, k, label=b"") as dk:  # label_len 0
        cases = M.empty_label_case_set(name)
        check(name + " (empty label)", cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))


# ---- 2. batch sizes around the 32 objects per workgroup of rsa_pair_k and
#         the 64 of rsa_finish_k ---------------------------------------------
def test_batch_sizes(eng):
    name = "wide_q_gt_p"
    with DevKey(eng, M.fixed_keys()[name]) as dk:
        for n in (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129):
            cases = mixed_batch(name, n)
            check("%s, batch of %d" % (name, n), cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))


# ---- 3. the grow-only workspace, reused by a smaller batch ------------------
def test_workspace_reuse(eng):
    name = "plain_q_gt_p"
    k = M.fixed_keys()[name]
    big = mixed_batch(name, 129)
    # the other way round from big[:3], and ciphertexts that big does not hold
    em = M.oaep_encode(M.det_bytes(32, name, "reuse msg"), M.det_bytes(32, name, "reuse seed"))
    fresh = M.ct256(M.encrypt_em(k, em))
    small = [M.Case(nm, ct, M.decrypt(k, ct)) for nm, ct in
             (("c = 3", M.ct256(3)), ("fresh valid", fresh), ("c = n - 2", M.ct256(k.n - 2)))]
    assert [c.expect is None for c in big[:3]] == [False, True, False]
    assert [c.expect is None for c in small] == [True, False, True]
    assert not {c.ct for c in small} & {c.ct for c in big}
    e = E.Engine(0)  # a context of its own: its workspace has seen nothing larger
    try:
        with DevKey(e, k) as dk:
            # the 129 again, moved on by one place: valid and invalid swap slots, so results the
            # first batch left in the workspace would be wrong for every item
            again = big[1:] + big[:1]
            assert all((a.expect is None) != (b.expect is None) for a, b in zip(big[:-1], again[:-1]))
            assert big[-1].expect != again[-1].expect
            for cases in (big, small, again):
                check("%s, batch of %d" % (name, len(cases)), cases, e.oaep_decrypt_batch(dk, [c.ct for c in cases]))
    finally:
        e.close()


# ---- 4. two keys alive on one context ---------------------------------------
def test_two_keys_interleaved(eng):
    na, nb = "top", "wide_q_gt_p"
    ka, kb = M.fixed_keys()[na], M.fixed_keys()[nb]
    ca, cb = mixed_batch(na, 5), mixed_batch(nb, 6)
    # each key also sees the other's ciphertexts: whatever the model says (errors, in practice)
    xa = [M.Case("made for " + nb, c.ct, M.decrypt(ka, c.ct)) for c in cb[:2]]
    xb = [M.Case("made for " + na, c.ct, M.decrypt(kb, c.ct)) for c in ca[:2]]
    with DevKey(eng, kb) as db:
        with DevKey(eng, ka) as da:
            for _ in range(2):
                check(na, ca + xa, eng.oaep_decrypt_batch(da, [c.ct for c in ca + xa]))
                check(nb, cb + xb, eng.oaep_decrypt_batch(db, [c.ct for c in cb + xb]))
        check(nb + " after the other key was freed", cb, eng.oaep_decrypt_batch(db, [c.ct for c in cb]))


# ---- 5. the raw C-ABI --------------------------------------------------------
def raw(eng, dk, cts, ct_stride, msg_stride, msg_bytes=None, null_msg=False):
    """jfsx_rsa_oaep_decrypt_batch itself; msg is prefilled with the sentinel.
    ct_len is each item's own length even where only ct_stride bytes of it
    fit its slot (an item longer than the modulus is never read)."""
    n = len(cts)
    buf = np.full(max(1, n * ct_stride), 0x5C, np.uint8)
    lens = np.zeros(max(1, n), np.uint32)
    for i, c in enumerate(cts):
        buf[i * ct_stride:i * ct_stride + min(len(c), ct_stride)] = np.frombuffer(c[:ct_stride], np.uint8)
        lens[i] = len(c)
    msg = np.full(n * msg_stride + 64 if msg_bytes is None else msg_bytes, SENTINEL, np.uint8)
    mlen = np.full(max(1, n), -7, np.int32)
    rc = eng.L.jfsx_rsa_oaep_decrypt_batch(eng.ctx, dk, n, buf.ctypes.data, ct_stride, lens.ctypes.data,
                                           None if null_msg else msg.ctypes.data, msg_stride, mlen.ctypes.data)
    return rc, msg, mlen


def test_raw_abi_strides_and_truncation(eng):
    name = "holes"
    by = {c.name: c for c in M.case_set(name)}
    cases = [by["valid len 32 seed 0"], by["bad oaep: no separator"], by["valid len 190 seed 1"],
             by["short as 255 bytes"], by["valid len 1 seed 2"], by["empty ciphertext"], by["valid len 0 seed 3"],
             by["edge c = n"], by["short as 257 bytes"], by["valid len 33 seed 4"]]
    n = len(cases)
    want_len = [-1 if c.expect is None else len(c.expect) for c in cases]
    with DevKey(eng, M.fixed_keys()[name]) as dk:
        for ct_stride in (300, 256):
            cts = [c.ct for c in cases]  # the 257-byte item does not fit a stride of 256: declared, never read
            for msg_stride in (256, 16):
                rc, msg, mlen = raw(eng, dk, cts, ct_stride, msg_stride)
                assert rc == 0
                for i, c in enumerate(cases):
                    what = "key %s, case %r, ct_stride %d, msg_stride %d" % (name, c.name, ct_stride, msg_stride)
                    assert mlen[i] == want_len[i], what  # the full length, whatever was copied
                    slot = msg[i * msg_stride:(i + 1) * msg_stride].tobytes()
                    kept = min(max(want_len[i], 0), msg_stride)
                    assert slot[:kept] == (c.expect or b"")[:kept], what
                    assert slot[kept:] == bytes([SENTINEL]) * (msg_stride - kept), what  # error items: the whole slot
                assert msg[n * msg_stride:].tobytes() == bytes([SENTINEL]) * 64
            # lengths only
            rc, msg, mlen = raw(eng, dk, cts, ct_stride, 0, msg_bytes=64, null_msg=True)
            assert rc == 0 and list(mlen) == want_len
            rc, msg, mlen = raw(eng, dk, cts, ct_stride, 0, msg_bytes=64)
            assert rc == 0 and list(mlen) == want_len and msg.tobytes() == bytes([SENTINEL]) * 64
        # n = 0: nothing to do, nothing touched
        rc, msg, mlen = raw(eng, dk, [], 256, 256, msg_bytes=64)
        assert rc == 0 and mlen[0] == -7 and msg.tobytes() == bytes([SENTINEL]) * 64
        assert eng.L.jfsx_rsa_oaep_decrypt_batch(eng.ctx, dk, 0, None, 0, None, None, 0, None) == 0
        assert eng.oaep_decrypt_batch(dk, []) == []


# ---- 6. keys the engine refuses ----------------------------------------------
def key_new(eng, comps, prime_bytes=128, label=b"keys"):
    out = ctypes.c_void_p(0xDEAD)
    rc = eng.L.jfsx_rsa_key_new(eng.ctx, *[bytes(c) for c in comps], prime_bytes, label, len(label),
                                ctypes.byref(out))
    return rc, out.value


def test_rejected_keys(eng):
    k = M.fixed_keys()["plain_p_gt_q"]
    p, q, dp, dq, qinv = M.components(k)

    def be(v):
        return v.to_bytes(128, "big")
    rc, h = key_new(eng, (p, q, dp, dq, qinv))
    assert rc == 0 and h
    assert eng.L.jfsx_rsa_key_free(h) == 0
    bad = {"even p": (be(k.p - 1), q, dp, dq, qinv), "even q": (p, be(k.q - 1), dp, dq, qinv),
           "p with the top bit clear": (be(k.p - (1 << 1023)), q, dp, dq, qinv),
           "q with the top bit clear": (p, be(k.q - (1 << 1023)), dp, dq, qinv),
           "dp = 1": (p, q, be(1), dq, qinv), "dq = 0": (p, q, dp, be(0), qinv),
           "dp = 1 and dq = 0": (p, q, be(1), be(0), qinv)}
    for what, comps in bad.items():
        rc, h = key_new(eng, comps)
        assert rc == E.EINVAL and not h, what
    rc, h = key_new(eng, [c[64:] for c in (p, q, dp, dq, qinv)], prime_bytes=64)
    assert rc == E.EINVAL and not h, "prime_bytes 64"
    with pytest.raises(E.EngineError):
        eng.rsa_key(be(k.p - 1), q, dp, dq, qinv)


def test_rsa1024_key_unwraps_on_the_host(eng):
    """The reference's own RSA-1024 fixture key is one the engine refuses
    (512-bit primes): DecryptBatch then unwraps on the host, by design, and
    returns what Decrypt returns.  This is the only test here that is meant to
    take that path, and it says so."""
    with open(os.path.join(HERE, "golden", "pem_fixtures.json")) as f:
        pem = json.load(f)["pemWithoutPass"].encode()
    rsae = enc.NewRSAEncryptor(enc.ParseRsaPrivateKeyFromPem(pem, None))
    assert rsae.privKey.size == 128
    comps = enc.rsa_crt_components(rsae.privKey, 64)
    rc, h = key_new(eng, comps, prime_bytes=64)
    assert rc == E.EINVAL and not h
    assert rsae._device_key(eng) is None
    msgs = [M.det_bytes(n, "rsa1024", n) for n in (0, 1, 32, 62)]
    cts = [rsae.Encrypt(m) for m in msgs]
    broken = bytearray(cts[2])
    broken[9] ^= 4
    got = rsae.DecryptBatch(cts + [bytes(broken)], eng)
    assert got[:4] == msgs == [rsae.Decrypt(c) for c in cts]
    assert isinstance(got[4], enc.EncryptError) and str(got[4]) == "crypto/rsa: decryption error"
    with pytest.raises(enc.EncryptError):
        rsae.Decrypt(bytes(broken))


# ---- 7. the one-lane kernel, in a child process -------------------------------
def test_one_lane_kernel_in_a_child_process(tmp_path):
    """rsa_half_k, which launch_rsa_unwrap picks when JFSX_RSA_PAIR=0.  The
    switch is read once per process, so a fresh child process is started with
    it set (tests/rsa_unwrap_child.py); the child unwraps and prints, this
    test compares with the model.  The suite cannot observe from outside which
    kernel ran: what is pinned is that a process started with JFSX_RSA_PAIR=0
    gives the model's results, and the switch itself is three lines of
    launch_rsa_unwrap."""
    names = ("top", "bottom", "wide_q_gt_p", "plain_q_gt_p")
    sizes = (1, 33, 65)
    jobs, want = [], []
    for nm in names:
        batches = [list(M.case_set(nm))]
        if nm == "wide_q_gt_p":
            batches += [mixed_batch(nm, n) for n in sizes]
        jobs.append({"comps": [c.hex() for c in M.components(M.fixed_keys()[nm])], "label": b"keys".hex(),
                     "batches": [[c.ct.hex() for c in b] for b in batches]})
        want.append(batches)
    path = tmp_path / "jobs.json"
    path.write_text(json.dumps(jobs))
    r = subprocess.run([sys.executable, os.path.join(HERE, "rsa_unwrap_child.py"), str(path)],
                       env=dict(os.environ, JFSX_RSA_PAIR="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    assert res["pair_env"] == "0"
    assert len(res["results"]) == len(names)
    for nm, batches, got in zip(names, want, res["results"]):
        assert len(got) == len(batches)
        for cases, g in zip(batches, got):
            check("%s, one-lane kernel, batch of %d" % (nm, len(cases)), cases,
                  [None if x is None else bytes.fromhex(x) for x in g])
