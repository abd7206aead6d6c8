"""The GPU RSA-OAEP unwrap and wrap with a 4096-bit key (jfsx_rsa.hip:
rsa_words_k, rsa_quad_k, rsa_finish_w_k; rsa_encode_k, rsa_wrap_w_k, rsa_pack_k)
against the big-integer model of tests/rsa_model_wide.py on the fixed keys of
tests/golden/rsa_keys_4096.json: every fixed key's whole case set, batch sizes
around the 16 items per wave of the quad kernels and the 64 of the finish and
encode kernels, both key sizes in turn on one context, the raw C-ABI at k =
512, jfsx_rsa_key_bytes, and the keys the engine refuses.

Every test hands the key to Engine.rsa_key and the items to the engine's batch
calls: there is no host path to fall back to."""
import ctypes

import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import rsa_model as M2
from tests import rsa_model_wide as M

pytestmark = pytest.mark.gpu

FIXED = list(M.fixed_keys())
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    yield e
    e.close()


class DevKey:
    """A device key that frees itself and checks that the free succeeds."""

    def __init__(self, eng, comps, label=b"keys"):
        self.eng, self.h = eng, eng.rsa_key(*comps, label=label)
        assert self.h

    def __enter__(self):
        return self.h

    def __exit__(self, *a):
        assert self.eng.L.jfsx_rsa_key_free(self.h) == 0


def check(name, cases, got):
    assert len(got) == len(cases)
    for c, g in zip(cases, got):
        assert g == c.expect, "key %s, case %r: got %r" % (name, c.name, g if g is None else g.hex())


# ---- 1. every fixed key: the whole case set, unwrap and wrap -----------------
@pytest.mark.parametrize("name", FIXED)
def test_fixed_key_matches_model(eng, name):
    M.assert_reaches_paths(name)
    k = M.fixed_keys()[name]
    cases = M.case_set(name)
    items = M.valid_inputs(name)
    msg, seed, c = M.short_ciphertext(name)
    items.append(("short", msg, seed))
    with DevKey(eng, M.components(k)) as dk:
        assert E.rsa_key_bytes(dk) == 512
        check(name, cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))
        got = eng.oaep_encrypt_batch(dk, [m for _, m, _ in items], [s for _, _, s in items])
        assert got == [M.encrypt(k, m, s) for _, m, s in items]
        assert got[-1] == M.ct512(c) and got[-1][0] == 0  # the left padding is written
        assert eng.oaep_decrypt_batch(dk, got) == [m for _, m, _ in items]


def test_empty_label_and_exponents(eng):
    name = "plain_q_gt_p"
    k = M.fixed_keys()[name]
    items = M.valid_inputs(name)[::4]
    with DevKey(eng, M.components(k), label=b"") as dk:
        got = eng.oaep_encrypt_batch(dk, [m for _, m, _ in items], [s for _, _, s in items])
        assert got == [M.encrypt(k, m, s, label=b"") for _, m, s in items]
        assert eng.oaep_decrypt_batch(dk, got) == [m for _, m, _ in items]
        # made for "keys": the label hash check
        assert eng.oaep_decrypt_batch(dk, [M.encrypt(k, items[0][1], items[0][2])]) == [None]
    with DevKey(eng, M.components(k)) as dk:
        for e in (3, 17, 0x5A5A5A5B, (1 << 31) - 1):
            got = eng.oaep_encrypt_batch(dk, [m for _, m, _ in items], [s for _, _, s in items], e=e)
            assert got == [M.ct512(pow(int.from_bytes(M.oaep_encode(m, s), "big"), e, k.n)) for _, m, s in items], e


# ---- 2. batch sizes ----------------------------------------------------------
def mixed_cases(name, n):
    """n cases of the key's set, valid ones and every kind of failure mixed."""
    cs = M.case_set(name)
    return [cs[(5 * i + n) % len(cs)] for i in range(n)]


def test_batch_sizes(eng):
    name = "wide_q_gt_p"
    k = M.fixed_keys()[name]
    inputs = M.valid_inputs(name)
    with DevKey(eng, M.components(k)) as dk:
        for n in (1, 15, 16, 17, 33, 65):
            cases = mixed_cases(name, n)
            check(name, cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))
            batch = [inputs[(7 * i + n) % len(inputs)] for i in range(n)]
            if n >= 3:
                batch[n // 2] = ("long", bytes(447), batch[n // 2][2])
            got = eng.oaep_encrypt_batch(dk, [m for _, m, _ in batch], [s for _, _, s in batch])
            assert got == [M.encrypt(k, m, s) for _, m, s in batch], n
            assert (n >= 3) == (None in got)


# ---- 3. both widths on one context: the workspace is shared ------------------
def test_2048_then_4096_then_2048(eng):
    n2, n4 = "wide_q_gt_p", "holes"
    k2, k4 = M2.fixed_keys()[n2], M.fixed_keys()[n4]
    c2, c4 = M2.case_set(n2)[:40], M.case_set(n4)
    with DevKey(eng, M2.components(k2)) as d2, DevKey(eng, M.components(k4)) as d4:
        assert (E.rsa_key_bytes(d2), E.rsa_key_bytes(d4)) == (256, 512)
        for dk, cases, nm in ((d2, c2, n2), (d4, c4, n4), (d2, c2[::-1], n2), (d4, c4[:3], n4), (d2, c2[:70], n2)):
            check(nm, cases, eng.oaep_decrypt_batch(dk, [c.ct for c in cases]))
        m2 = [(M2.det_bytes(32, "mix", i), M2.det_bytes(32, "mix seed", i)) for i in range(20)]
        want2 = [M2.ct256(pow(int.from_bytes(M2.oaep_encode(m, s), "big"), M2.E, k2.n)) for m, s in m2]
        want4 = [M.encrypt(k4, m, s) for m, s in m2]
        for _ in range(2):
            assert eng.oaep_encrypt_batch(d2, [m for m, _ in m2], [s for _, s in m2]) == want2
            assert eng.oaep_encrypt_batch(d4, [m for m, _ in m2], [s for _, s in m2]) == want4
        # a 2048-bit key's ciphertext under the 4096-bit key: 256 bytes, taken as the number it is
        assert eng.oaep_decrypt_batch(d4, want2[:3]) == [M.decrypt(k4, c) for c in want2[:3]] == [None] * 3


# ---- 4. the raw C-ABI at k = 512 ---------------------------------------------
def raw_decrypt(eng, dk, cts, ct_stride, msg_stride):
    n = len(cts)
    buf = np.full(n * ct_stride, 0x5C, np.uint8)
    lens = np.zeros(n, np.uint32)
    for i, c in enumerate(cts):
        buf[i * ct_stride:i * ct_stride + min(len(c), ct_stride)] = np.frombuffer(c[:ct_stride], np.uint8)
        lens[i] = len(c)
    msg = np.full(n * msg_stride + 64, SENTINEL, np.uint8)
    mlen = np.full(n, -7, np.int32)
    rc = eng.L.jfsx_rsa_oaep_decrypt_batch(eng.ctx, dk, n, buf.ctypes.data, ct_stride, lens.ctypes.data,
                                           msg.ctypes.data, msg_stride, mlen.ctypes.data)
    return rc, msg, mlen


def raw_encrypt(eng, dk, batch, msg_stride, ct_stride, e=M.E):
    n = len(batch)
    buf = np.zeros(n * msg_stride, np.uint8)
    lens = np.zeros(n, np.uint32)
    for i, (m, _) in enumerate(batch):
        buf[i * msg_stride:i * msg_stride + len(m)] = np.frombuffer(m, np.uint8)
        lens[i] = len(m)
    seeds = np.frombuffer(b"".join(s for _, s in batch), np.uint8)
    ct = np.full(n * ct_stride + 64, SENTINEL, np.uint8)
    st = np.full(n, -7, np.int32)
    rc = eng.L.jfsx_rsa_oaep_encrypt_batch(eng.ctx, dk, e, n, buf.ctypes.data, msg_stride, lens.ctypes.data,
                                           seeds.ctypes.data, ct.ctypes.data, ct_stride, st.ctypes.data)
    return rc, ct, st


def test_raw_abi(eng):
    name = "holes"
    k = M.fixed_keys()[name]
    by = {c.name: c for c in M.case_set(name)}
    cases = [by["valid len 32 seed 0"], by["bad oaep: no separator"], by["valid len 446 seed 1"],
             by["short as 511 bytes"], by["empty ciphertext"], by["edge c = n"], by["513 bytes"], by["256 bytes"],
             by["1 byte"], by["valid len 33 seed 2"]]
    want_len = [-1 if c.expect is None else len(c.expect) for c in cases]
    with DevKey(eng, M.components(k)) as dk:
        # the unwrap: strides, and truncation to msg_stride
        for ct_stride in (520, 512):  # the 513-byte item does not fit 512: declared, never read
            for msg_stride in (512, 446, 16):
                rc, msg, mlen = raw_decrypt(eng, dk, [c.ct for c in cases], ct_stride, msg_stride)
                assert rc == 0
                for i, c in enumerate(cases):
                    what = "case %r, ct_stride %d, msg_stride %d" % (c.name, ct_stride, msg_stride)
                    assert mlen[i] == want_len[i], what
                    slot = msg[i * msg_stride:(i + 1) * msg_stride].tobytes()
                    kept = min(max(want_len[i], 0), msg_stride)
                    assert slot[:kept] == (c.expect or b"")[:kept], what
                    assert slot[kept:] == bytes([SENTINEL]) * (msg_stride - kept), what
                assert msg[len(cases) * msg_stride:].tobytes() == bytes([SENTINEL]) * 64
        # the wrap: strides 512 and 520, the slack untouched; 447 bytes is one too many
        batch = [(M.det_bytes(n, name, "raw msg", i), M.det_bytes(32, name, "raw seed", i))
                 for i, n in enumerate((32, 446, 447, 0, 445))]
        want = [M.encrypt(k, m, s) for m, s in batch]
        assert [w is None for w in want] == [False, False, True, False, False]
        for ct_stride in (512, 520):
            rc, ct, st = raw_encrypt(eng, dk, batch, 447, ct_stride)
            assert rc == 0 and list(st) == [0, 0, -1, 0, 0]
            for i, w in enumerate(want):
                slot = ct[i * ct_stride:(i + 1) * ct_stride].tobytes()
                assert slot[:512] == (w if w is not None else bytes(512)), (ct_stride, i)  # status -1: 512 zero bytes
                assert slot[512:] == bytes([SENTINEL]) * (ct_stride - 512)
            assert ct[len(batch) * ct_stride:].tobytes() == bytes([SENTINEL]) * 64
        rc, ct, st = raw_encrypt(eng, dk, batch, 447, 511)
        assert rc == E.EINVAL and list(st) == [-7] * 5 and ct.tobytes() == bytes([SENTINEL]) * len(ct)
        # a 2048-bit key keeps its 256: ct_stride 256 is enough there and not here
        rc, ct, st = raw_encrypt(eng, dk, batch[:1], 447, 256)
        assert rc == E.EINVAL
    with DevKey(eng, M2.components(M2.fixed_keys()["holes"])) as d2:
        rc, ct, st = raw_encrypt(eng, d2, batch[:1], 447, 256)
        assert rc == 0 and st[0] == 0
        rc, ct, st = raw_encrypt(eng, d2, batch[1:2], 447, 256)  # 446 bytes: too long for RSA-2048
        assert rc == 0 and st[0] == -1 and ct[:256].tobytes() == bytes(256)
    assert eng.L.jfsx_rsa_key_bytes(None) == E.EINVAL


# ---- 5. keys the engine refuses ----------------------------------------------
def key_new(eng, comps, prime_bytes, label=b"keys"):
    out = ctypes.c_void_p(0xDEAD)
    rc = eng.L.jfsx_rsa_key_new(eng.ctx, *[bytes(c) for c in comps], prime_bytes, label, len(label),
                                ctypes.byref(out))
    return rc, out.value


def test_rejected_keys(eng):
    k = M.fixed_keys()["plain_p_gt_q"]
    p, q, dp, dq, qinv = M.components(k)

    def be(v):
        return v.to_bytes(256, "big")
    rc, h = key_new(eng, (p, q, dp, dq, qinv), 256)
    assert rc == 0 and h and eng.L.jfsx_rsa_key_bytes(h) == 512
    assert eng.L.jfsx_rsa_key_free(h) == 0
    bad = {"even p": (be(k.p - 1), q, dp, dq, qinv), "even q": (p, be(k.q - 1), dp, dq, qinv),
           "p with the top bit clear": (be(k.p - (1 << 2047)), q, dp, dq, qinv),
           "q with the top bit clear": (p, be(k.q - (1 << 2047)), dp, dq, qinv),
           "dp = 1": (p, q, be(1), dq, qinv), "dq = 0": (p, q, dp, be(0), qinv),
           "dp = 1 and dq = 0": (p, q, be(1), be(0), qinv)}
    for what, comps in bad.items():
        rc, h = key_new(eng, comps, 256)
        assert rc == E.EINVAL and not h, what
    # other sizes: a 3072-bit key's 192-byte primes, and 512
    for nb in (192, 512, 64, 0, 255, 257):
        comps = [(bytes(512) + c)[-nb:] if nb else b"" for c in (p, q, dp, dq, qinv)]
        comps = [bytes([c[0] | 0x80]) + c[1:-1] + bytes([c[-1] | 1]) if nb else b"\x81" for c in comps]
        rc, h = key_new(eng, comps, nb)
        assert rc == E.EINVAL and not h, "prime_bytes %d" % nb
    with pytest.raises(E.EngineError):
        eng.rsa_key(be(k.p - 1), q, dp, dq, qinv)
