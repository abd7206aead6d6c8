"""CPU pin of the batched RSA-OAEP key wrap arithmetic (jfsx_rsa.h: oaep_encode,
mont_mul28_wide / mont_mul28_quad, mod_exp28_pub / mod_exp28_pub_quad,
encrypt), compiled for the host (tests/harness/rsa_wrap_host.cpp) and checked
against Python integers, the big-integer model of tests/rsa_model.py on the
fixed keys of tests/golden/rsa_keys.json, and libcrypto's RSA-OAEP -- the
rsaEncryptor.Encrypt of pkg/object/encrypt.go:128-130."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from juicefs_amd import encrypt as enc
from tests import rsa_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "rsa_wrap_host.cpp")

N28 = 74                  # 28-bit limbs of a 2048-bit number
RW = 1 << (28 * N28)      # the Montgomery radix R''
EXPONENTS = (2, 3, 17, 65537, 0x5A5A5A5B, (1 << 31) - 1)
FIXED = list(M.fixed_keys())


@pytest.fixture(scope="module")
def wrap(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rsa_wrap") / "rsa_wrap_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", out, SRC])
    lib = ctypes.CDLL(out)
    lib.wrap_exp_trace.restype = ctypes.c_uint64
    lib.wrap_exp_trace.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return lib


def be(v):
    return v.to_bytes(256, "big")


def stream_int(*tag):
    return int.from_bytes(M.det_bytes(256, "rsa wrap", *tag), "big")


def moduli():
    """(name, m): the accumulators' worst case (every limb all ones; the
    product does not care that it is no prime), the smallest 2048-bit odd
    number, the n of every fixed key, and odd numbers from a fixed stream."""
    ms = [("2^2048-1", (1 << 2048) - 1), ("2^2047+1", (1 << 2047) + 1)]
    ms += [(name, k.n) for name, k in M.fixed_keys().items()]
    ms += [("stream %d" % i, stream_int("modulus", i) | (1 << 2047) | 1) for i in range(3)]
    ms.append(("stream, 2041 bits", (stream_int("modulus", "short") >> 7) | (1 << 2040) | 1))
    return ms


def operands(name, m):
    return [0, 1, m - 1, (m - 1) * (m - 1) % m, stream_int("operand", name, 0) % m, stream_int("operand", name, 1) % m]


def mont_mul(wrap, m, a, b, quad):
    out = ctypes.create_string_buffer(256)
    assert wrap.wrap_mont_mul(be(m), be(a), be(b), out, quad) == 1, "limbs not normalized"
    return int.from_bytes(out.raw, "big")


def exp_trace(wrap, m, e, x, quad):
    out = ctypes.create_string_buffer(256)
    ops, same = ctypes.c_uint64(), ctypes.c_int()
    h = wrap.wrap_exp_trace(be(m), e, be(x), out, ctypes.byref(ops), ctypes.byref(same), quad)
    assert same.value == 1
    return int.from_bytes(out.raw, "big"), (h, ops.value)


def encrypt(wrap, comps, msg, seed, e=M.E, label=b"keys"):
    ct = ctypes.create_string_buffer(b"\xAA" * 256, 256)
    rc = wrap.wrap_encrypt(*comps, label, len(label), e, bytes(msg), len(msg), bytes(seed), ct)
    return rc, ct.raw


@pytest.mark.parametrize("label", [b"keys", b""])
def test_oaep_encode_matches_model(wrap, label):
    for n in (0, 1, 31, 32, 33, 190):
        for s in range(3):
            msg, seed = M.det_bytes(n, "encode msg", n, s), M.det_bytes(32, "encode seed", n, s)
            em = ctypes.create_string_buffer(256)
            wrap.wrap_oaep_encode(label, len(label), msg, n, seed, em)
            assert em.raw == bytes(M.oaep_encode(msg, seed, label=label)), (label, n, s)
            assert M.oaep_decode(em.raw, label=label) == msg


@pytest.mark.parametrize("quad", [0, 1], ids=["one lane", "quad"])
def test_product_mod_2048_bits(wrap, quad):
    """a b R''^-1 mod m, normalized and fully reduced, for every modulus and
    every pair of the edge operands."""
    for name, m in moduli():
        rinv = pow(RW, -1, m)
        ops = operands(name, m)
        for a in ops:
            for b in ops:
                assert mont_mul(wrap, m, a, b, quad) == a * b * rinv % m, (name, hex(a), hex(b))


@pytest.mark.parametrize("quad", [0, 1], ids=["one lane", "quad"])
def test_public_exponentiation_matches_pow_with_one_trace_per_exponent(wrap, quad):
    """x^e mod m equals pow() for every modulus, operand and exponent, and the
    recorded sequence of products depends on e alone: bit_length(e) +
    popcount(e) products (enter, a squaring per bit under the top one, a
    multiply per set bit under it, leave), the same for operand 0, 1, m - 1
    and stream values."""
    for name, m in moduli():
        for e in EXPONENTS:
            traces = set()
            for x in operands(name, m):
                got, tr = exp_trace(wrap, m, e, x, quad)
                assert got == pow(x, e, m), (name, e, hex(x))
                traces.add(tr)
            assert len(traces) == 1, (name, e, traces)
            assert next(iter(traces))[1] == e.bit_length() + bin(e).count("1"), (name, e)


def test_traces_differ_between_exponents(wrap):
    """The trace hook does record: exponents of other shape give other counts."""
    m = M.fixed_keys()["top"].n
    counts = {e: exp_trace(wrap, m, e, 5, 0)[1][1] for e in EXPONENTS}
    assert counts[2] == 3 and counts[3] == 4 and counts[65537] == 19 and counts[(1 << 31) - 1] == 62


@pytest.mark.parametrize("name", FIXED)
def test_encrypt_fixed_key_matches_model(wrap, name):
    """encrypt() on every (message, seed) the model's valid ciphertexts are
    built from: the same 256 bytes; and the pair whose ciphertext is below
    2^2040, so the left padding is written."""
    k = M.fixed_keys()[name]
    comps = M.components(k)
    items = M.valid_ints(name)
    assert len(items) == 42
    for n in M.VALID_LENGTHS:
        for s in range(M.VALID_SEEDS):
            nm, msg, c = items[M.VALID_LENGTHS.index(n) * M.VALID_SEEDS + s]
            assert nm == "valid len %d seed %d" % (n, s)
            rc, ct = encrypt(wrap, comps, msg, M.det_bytes(M.HLEN, name, "seed", n, s))
            assert rc == 0 and ct == M.ct256(c), (name, nm)
    msg, c = M.short_ciphertext(name)
    for s in range(100000):
        if M.det_bytes(32, name, "short msg", s) == msg:
            break
    rc, ct = encrypt(wrap, comps, msg, M.det_bytes(M.HLEN, name, "short seed", s))
    assert rc == 0 and ct == M.ct256(c) and ct[0] == 0


def test_encrypt_other_label_and_exponents(wrap):
    k = M.fixed_keys()["plain_q_gt_p"]
    comps = M.components(k)
    msg, seed = M.det_bytes(32, "label msg"), M.det_bytes(32, "label seed")
    for label in (b"", b"other"):
        rc, ct = encrypt(wrap, comps, msg, seed, label=label)
        assert rc == 0 and ct == M.ct256(M.encrypt_em(k, M.oaep_encode(msg, seed, label=label)))
    em = int.from_bytes(M.oaep_encode(msg, seed), "big")
    for e in EXPONENTS:
        rc, ct = encrypt(wrap, comps, msg, seed, e=e)
        assert rc == 0 and ct == M.ct256(pow(em, e, k.n)), e


def test_encrypt_message_too_long(wrap):
    comps = M.components(M.fixed_keys()["top"])
    for n in (191, 192, 255):
        rc, ct = encrypt(wrap, comps, bytes(n), bytes(32))
        assert rc == -1 and ct == bytes(256)
    assert encrypt(wrap, comps, bytes(190), bytes(32))[0] == 0


def test_encrypt_decrypts_in_libcrypto(wrap):
    """On a freshly generated libcrypto key: what encrypt() wraps, libcrypto's
    RSA-OAEP(SHA-256, "keys") unwraps."""
    priv = enc.GenerateRsaKey(2048)
    rsae = enc.NewRSAEncryptor(priv)
    comps = enc.rsa_crt_components(priv)
    for n in (0, 1, 31, 32, 33, 190):
        msg = os.urandom(n)
        rc, ct = encrypt(wrap, comps, msg, os.urandom(32))
        assert rc == 0
        assert rsae.Decrypt(ct) == msg


def test_key_carries_the_constants_of_n(wrap):
    """R''^2 mod n and -n^-1 mod 2^28 reach encrypt() through key_setup: a
    wrong constant would show above; here n itself, for both orders of p and
    q, against the model's product."""
    ks = M.fixed_keys()
    assert ks["top"].n == ks["top_swapped"].n
    msg, seed = M.det_bytes(32, "n msg"), M.det_bytes(32, "n seed")
    a = encrypt(wrap, M.components(ks["top"]), msg, seed)
    b = encrypt(wrap, M.components(ks["top_swapped"]), msg, seed)
    assert a == b and a[0] == 0
    assert hashlib.sha256(a[1]).digest() == hashlib.sha256(
        M.ct256(M.encrypt_em(ks["top"], M.oaep_encode(msg, seed)))).digest()


def test_sanitized_standalone_run(tmp_path):
    """The harness with its own main under AddressSanitizer and UBSan, as a
    stand-alone program (tests/harness/rsa_wrap_sanitize.mk builds the same): both
    product forms, both exponentiations and encrypt() on edge operands."""
    exe = str(tmp_path / "rsa_wrap_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRSA_WRAP_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "rsa_wrap_host: ok" in r.stdout, (r.stdout, r.stderr)
