"""CPU pin of the RSA-4096 arithmetic (jfsx_rsa.h: mont_mul28_wide<148> /
mont_mul28_quad<X, 148>, reduce_quad, mod_exp28_priv_wide / mod_exp28_priv_quad,
decrypt_w, encrypt_w), compiled for the host (tests/harness/rsa4096_host.cpp,
the lane exchanges emulated by four threads through the X template parameter)
and checked against Python integers, the big-integer model of
tests/rsa_model_wide.py on the fixed keys of tests/golden/rsa_keys_4096.json,
and libcrypto's RSA-OAEP."""
import ctypes
import os
import subprocess

import pytest

from juicefs_amd import encrypt as enc
from tests import rsa_model_wide as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "harness", "rsa4096_host.cpp")

N28 = 148                 # 28-bit limbs the product takes a 4096-bit number in (4 x 37)
RW = 1 << (28 * N28)      # its Montgomery radix R''
FIXED = list(M.fixed_keys())


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rsa4096") / "rsa4096_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", out, SRC])
    so = ctypes.CDLL(out)
    so.w_priv_exp_trace.restype = ctypes.c_uint64
    so.w_priv_exp_trace.argtypes = [ctypes.c_char_p] * 4 + [ctypes.POINTER(ctypes.c_uint64),
                                                            ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    return so


def be(v, n=512):
    return v.to_bytes(n, "big")


def stream_int(nbytes, *tag):
    return int.from_bytes(M.det_bytes(nbytes, "rsa4096", *tag), "big")


def mont_mul(lib, m, a, b, quad):
    out = ctypes.create_string_buffer(512)
    assert lib.w_mont_mul(be(m), be(a), be(b), out, quad) == 1, "limbs not normalized"
    return int.from_bytes(out.raw, "big")


def reduce(lib, p, c, quad):
    out = ctypes.create_string_buffer(256)
    assert lib.w_reduce(be(p, 256), be(c), out, quad) == 1, "limbs not normalized"
    return int.from_bytes(out.raw, "big")


def priv_exp(lib, p, e, x, quad):
    out = ctypes.create_string_buffer(256)
    ops, ok = ctypes.c_uint64(), ctypes.c_int()
    h = lib.w_priv_exp_trace(be(p, 256), be(e, 256), be(x, 256), out, ctypes.byref(ops), ctypes.byref(ok), quad)
    assert ok.value == 1
    return int.from_bytes(out.raw, "big"), (h, ops.value)


def decrypt(lib, comps, ct, label=b"keys"):
    msg = ctypes.create_string_buffer(512)
    n = lib.w_decrypt(*comps, label, len(label), bytes(ct), len(ct), msg)
    assert n >= -1
    return None if n < 0 else msg.raw[:n]


def encrypt(lib, comps, msg, seed, e=M.E, label=b"keys"):
    ct = ctypes.create_string_buffer(b"\xAA" * 512, 512)
    rc = lib.w_encrypt(*comps, label, len(label), e, bytes(msg), len(msg), bytes(seed), ct)
    return rc, ct.raw


# ---- products ----------------------------------------------------------------
def moduli():
    """The accumulators' worst case (every limb all ones), the smallest 4096-bit
    odd number, the n of two fixed keys, and an odd number from a fixed stream."""
    ks = M.fixed_keys()
    return [("2^4096-1", (1 << 4096) - 1), ("2^4095+1", (1 << 4095) + 1), ("top", ks["top"].n),
            ("bottom", ks["bottom"].n), ("stream", stream_int(512, "modulus") | (1 << 4095) | 1)]


def operands(name, m):
    """0, 1, m - 1, all-ones limbs (below m), a single top limb, a stream value."""
    ones = (1 << 4095) - 1
    top_limb = 1 << (28 * 146)
    return [0, 1, m - 1, ones, top_limb, stream_int(512, "operand", name) % m]


@pytest.mark.parametrize("quad", [0, 1], ids=["one lane", "quad"])
def test_product_mod_4096_bits(lib, quad):
    """a b R''^-1 mod m, normalized and fully reduced, for every modulus and
    every pair of the edge operands.  m = 2^4096 - 1 with all-ones operands is
    the case the column accumulators' bound (and the carry sweep in the middle
    of the 148 rows) is written for."""
    for name, m in moduli():
        rinv = pow(RW, -1, m)
        ops = operands(name, m)
        for i, a in enumerate(ops):
            for b in ops[i:] if quad else ops:
                assert mont_mul(lib, m, a, b, quad) == a * b * rinv % m, (name, hex(a)[:20], hex(b)[:20])
                if quad and a != b:
                    assert mont_mul(lib, m, b, a, quad) == a * b * rinv % m, (name, "swapped")


@pytest.mark.parametrize("quad", [0, 1], ids=["one lane", "quad"])
def test_input_reduction_with_0_1_and_2_corrections(lib, quad):
    """c mod p for the 4096-bit c and the 2048-bit p, on values the model says
    need no, one and both of the masked corrections, for both primes of the key
    next to 2^2047 and of the key next to 2^2048."""
    seen = set()
    for name in ("bottom", "top", "holes"):
        k = M.fixed_keys()[name]
        cs = [c for _, _, c in M.valid_ints(name)] + [0, k.n - 1, k.p, k.q * (k.p - 1), (1 << 4096) - 1, M.R - 1,
                                                       (k.p - 1) << 2048 | (M.R - 1)]
        for p in (k.p, k.q):
            for c in cs:
                assert reduce(lib, p, c, quad) == c % p, (name, hex(c)[:20])
                seen.add(M.reduce_corrections(p, c))
    assert seen == {0, 1, 2}


# ---- exponentiation ----------------------------------------------------------
def test_private_exponentiation_matches_pow_on_the_fixed_keys(lib):
    """x^dp mod p and x^dq mod q by the quad form for every fixed key, and by
    the one-lane form: pow()'s value and the same operation trace."""
    for name in FIXED:
        k = M.fixed_keys()[name]
        c = M.valid_ints(name)[0][2]
        for p, d in ((k.p, k.dp), (k.q, k.dq)):
            got, tr = priv_exp(lib, p, d, c % p, 1)
            assert got == pow(c % p, d, p), name
            one, tr1 = priv_exp(lib, p, d, c % p, 0)
            assert one == got and tr1[1] == tr[1], name


def test_trace_does_not_depend_on_the_exponent(lib):
    """The sequence of products and window-table reads is the same for two
    different exponents of one bit length, for a short exponent, and for
    operands 0, 1 and p - 1: 8 table products, 683 digits of three squarings
    and a multiply, one product to leave, and 8 masked reads per digit."""
    k = M.fixed_keys()["plain_p_gt_q"]
    p = k.p
    e1 = k.dp
    e2 = stream_int(256, "exponent") >> (2048 - e1.bit_length()) | 1 << (e1.bit_length() - 1)
    assert e1 != e2 and e1.bit_length() == e2.bit_length()
    for quad in (1, 0):
        traces = set()
        for e, x in ((e1, 5), (e2, 5), (3, 5), ((1 << 2048) - 1, p - 1), (e1, 0), (e2, 1)):
            got, tr = priv_exp(lib, p, e, x, quad)
            assert got == pow(x, e, p), (quad, hex(e)[:20])
            traces.add(tr)
        assert len(traces) == 1, (quad, traces)
        assert next(iter(traces))[1] == 8 + 4 * 683 + 1 + 8 * 683


# ---- whole operations --------------------------------------------------------
@pytest.mark.parametrize("name", FIXED)
def test_decrypt_and_encrypt_match_the_model(lib, name):
    M.assert_reaches_paths(name)
    k = M.fixed_keys()[name]
    comps = M.components(k)
    for c in M.case_set(name):
        assert decrypt(lib, comps, c.ct) == c.expect, (name, c.name)
    for nm, msg, seed in M.valid_inputs(name):
        rc, ct = encrypt(lib, comps, msg, seed)
        assert rc == 0 and ct == M.encrypt(k, msg, seed), (name, nm)
    msg, seed, c = M.short_ciphertext(name)
    rc, ct = encrypt(lib, comps, msg, seed)
    assert rc == 0 and ct == M.ct512(c) and ct[0] == 0


def test_model_lookup_is_pow(lib):
    """The model answers the ciphertexts it made itself from a table (RSADP
    inverts RSAEP); on a sample of every kind the table and pow(c, d, n) agree."""
    name = "wide_q_gt_p"
    k = M.fixed_keys()[name]
    cs = M.case_set(name)
    for c in cs[:3] + tuple(c for c in cs if c.name.startswith(("bad oaep", "edge c = n-1", "edge c = p^e", "short"))):
        assert M.decrypt(k, c.ct, lookup=False) == c.expect, c.name


def test_too_long_other_label_and_exponents(lib):
    k = M.fixed_keys()["plain_q_gt_p"]
    comps = M.components(k)
    for n in (447, 448, 511):
        rc, ct = encrypt(lib, comps, bytes(n), bytes(32))
        assert rc == -1 and ct == bytes(512)
    msg, seed = M.det_bytes(32, "label msg"), M.det_bytes(32, "label seed")
    for label in (b"", b"other"):
        rc, ct = encrypt(lib, comps, msg, seed, label=label)
        assert rc == 0 and ct == M.encrypt(k, msg, seed, label=label)
        assert decrypt(lib, comps, ct, label=label) == msg and decrypt(lib, comps, ct) is None
    em = int.from_bytes(M.oaep_encode(msg, seed), "big")
    for e in (2, 3, 17, 0x5A5A5A5B, (1 << 31) - 1):
        rc, ct = encrypt(lib, comps, msg, seed, e=e)
        assert rc == 0 and ct == M.ct512(pow(em, e, k.n)), e


def test_against_libcrypto(lib):
    """On a freshly generated libcrypto key: what encrypt_w wraps, libcrypto's
    RSA-OAEP(SHA-256, "keys") unwraps, and a libcrypto ciphertext decrypts here."""
    priv = enc.GenerateRsaKey(4096)
    rsae = enc.NewRSAEncryptor(priv)
    comps = enc.rsa_crt_components(priv, 256)
    for n in (0, 1, 32, 446):
        msg = os.urandom(n)
        rc, ct = encrypt(lib, comps, msg, os.urandom(32))
        assert rc == 0 and rsae.Decrypt(ct) == msg
        assert decrypt(lib, comps, rsae.Encrypt(msg)) == msg


def test_sanitized_standalone_run(tmp_path):
    """The harness with its own main under AddressSanitizer and UBSan, as a
    stand-alone program: both product forms, both reductions, both private
    exponentiations, encrypt_w and decrypt_w on edge operands."""
    exe = str(tmp_path / "rsa4096_sanitize")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-DRSA4096_MAIN", "-o", exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "rsa4096_host: ok" in r.stdout, (r.stdout, r.stderr)
