"""The composed CRC32C tables of the GCM kernel's two-row loop, on the CPU.

Inside that loop a lane carries B = x^8064 * A, its CRC already shifted across
the 1008-byte gap to the lane's next piece, so the shift is no lookup of its
own: B' = sum_{k<4} TT_k[byte k of (p0 ^ B)] ^ sum_{k>=4} TT_k[data byte k]
with TT_k[v] = x^8064 * U_k[v].  A B-form state comes back at a segment end
through xlB[l] = xl[l] * x^-8064, enters a following row through the slice
step's no-shift entry, or is multiplied back by x^-8064 (xlB[63]) ahead of a
ragged tail.  The tables come from the library's own host code
(jfsx_debug_crc_composed, jfsx_debug_tables); every emulated CRC is compared
with the oracle's CRC32C."""
import numpy as np
import pytest

from juicefs_amd import engine
from oracle import oracle as orc

POLY = 0x82F63B78
ROW = 1024


def mulmod(a, b):
    p = 0
    for _ in range(32):
        if a & 0x80000000:
            p ^= b
        a = (a << 1) & 0xFFFFFFFF
        b = (b >> 1) ^ POLY if b & 1 else b >> 1
    return p


def xpow8(n, x8):
    r, k = 0x80000000, 0
    while n:
        if n & 1:
            r = mulmod(int(x8[k]), r)
        n >>= 1
        k += 1
    return r


@pytest.fixture(scope="module")
def tabs():
    _, crc, crcx = engine.debug_tables()
    tt, xlb = engine.debug_crc_composed()
    return {"crc": crc.reshape(32, 256), "crcx": crcx, "tt": tt.reshape(16, 256), "xlb": xlb, "x8": crcx[64:96]}


def test_composed_tables_are_the_shifted_slice_tables(tabs):
    x1008 = xpow8(1008, tabs["x8"])
    for k in range(16):
        for v in range(256):
            assert int(tabs["tt"][k, v]) == mulmod(x1008, int(tabs["crc"][k, v])), (k, v)


def test_lane_constants_undo_the_shift(tabs):
    x1008 = xpow8(1008, tabs["x8"])
    for lane in range(64):
        assert mulmod(int(tabs["xlb"][lane]), x1008) == int(tabs["crcx"][lane]), lane
    assert mulmod(int(tabs["xlb"][63]), x1008) == 0x80000000  # x^-8064 itself


def rows_b_form(tabs, data, nrows, B=None):
    """nrows full rows of the 64-lane strided update in B form, all lanes at once"""
    tt = tabs["tt"]
    B = np.zeros(64, np.uint32) if B is None else B
    d = np.frombuffer(data, np.uint8)[:nrows * ROW].reshape(nrows, 64, 16)
    for r in range(nrows):
        p = d[r]
        q = B ^ p[:, :4].copy().view(np.uint32).reshape(64)
        n = tt[0][q & 255] ^ tt[1][(q >> 8) & 255] ^ tt[2][(q >> 16) & 255] ^ tt[3][q >> 24]
        for k in range(4, 16):
            n ^= tt[k][p[:, k]]
        B = n
    return B


def piece_a_form(tabs, s, p):
    """the slice step on an already shifted state s (the no-shift entry)"""
    T = tabs["crc"]
    q = bytearray(p)
    for k in range(4):
        q[k] ^= (s >> (8 * k)) & 255
    r = 0
    for j in range(16):
        r ^= int(T[j, q[j]])
    return r


def shift1008(tabs, a):
    T = tabs["crc"]
    return int(T[16, a & 255]) ^ int(T[17, (a >> 8) & 255]) ^ int(T[18, (a >> 16) & 255]) ^ int(T[19, a >> 24])


def partial_a_form(tabs, a, p):
    c = shift1008(tabs, a)
    for byte in p:
        c = int(tabs["crc"][15, (c ^ byte) & 255]) ^ (c >> 8)
    return c


def segment_end(tabs, L, A, lend, tail_ref, xl):
    """crc_segment_end: lanes whose last piece lies in the last full row
    (lend == 0) go from that row's end (tail_ref) with xl, the others from lend"""
    x8 = tabs["x8"]
    raw = 0
    for lane in range(64):
        if lend[lane] == 0:
            sh = int(xl[lane]) if tail_ref == L else mulmod(xpow8(L - tail_ref, x8), int(xl[lane]))
        else:
            sh = xpow8(L - lend[lane], x8)
        raw ^= mulmod(sh, int(A[lane]))
    K = int(tabs["crcx"][96]) if L == 32768 else mulmod(xpow8(L, x8), 0xFFFFFFFF)
    return (~(K ^ raw)) & 0xFFFFFFFF


def ragged_rows(tabs, seg, start, A, lend):
    """row_generic's CRC part over [start, len(seg)): A-form pieces and byte tails"""
    L = len(seg)
    for row in range(start, L, ROW):
        for lane in range(64):
            o = row + 16 * lane
            if o + 16 <= L:
                A[lane] = piece_a_form(tabs, shift1008(tabs, A[lane]), seg[o:o + 16])
                lend[lane] = o + 16
            elif o < L:
                A[lane] = partial_a_form(tabs, A[lane], seg[o:L])
                lend[lane] = L
    return A, lend


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_b_form_loop_over_whole_segments(tabs, seed):
    """32 rows in B form, brought back with xlB and reduced as crc_segment_done does"""
    seg = orc.gen_block(0xB0 + seed, seed, 32768).tobytes()
    B = rows_b_form(tabs, seg, 32)
    raw = 0
    for lane in range(64):
        raw ^= mulmod(int(tabs["xlb"][lane]), int(B[lane]))
    assert (~(int(tabs["crcx"][96]) ^ raw)) & 0xFFFFFFFF == orc.crc32c(seg)


@pytest.mark.parametrize("pairs", [1, 3, 15])
def test_stream_that_ends_in_b_form(tabs, pairs):
    """a short last segment of whole row pairs: xlB stands in for xl at the segment end"""
    L = 2 * pairs * ROW
    seg = orc.gen_block(0xB5, pairs, L).tobytes()
    B = rows_b_form(tabs, seg, 2 * pairs)
    assert segment_end(tabs, L, B, [0] * 64, L, tabs["xlb"]) == orc.crc32c(seg)


@pytest.mark.parametrize("pairs,tail", [(1, 1), (2, 1000), (3, 17), (5, 1023)])
def test_b_form_then_one_row_and_a_byte_tail(tabs, pairs, tail):
    """the loop leaves B form; one whole row enters through the no-shift entry
    and leaves A form; the ragged tail and the segment end follow in A form"""
    L = (2 * pairs + 1) * ROW + tail
    seg = orc.gen_block(0xB6, tail, L).tobytes()
    B = rows_b_form(tabs, seg, 2 * pairs)
    row = 2 * pairs * ROW
    A = [piece_a_form(tabs, int(B[lane]), seg[row + 16 * lane:row + 16 * lane + 16]) for lane in range(64)]
    tail_ref = row + ROW
    A, lend = ragged_rows(tabs, seg, tail_ref, A, [0] * 64)
    assert segment_end(tabs, L, A, lend, tail_ref, tabs["crcx"][:64]) == orc.crc32c(seg)


@pytest.mark.parametrize("pairs,tail", [(1, 5), (4, 1000), (7, 16)])
def test_b_form_then_a_ragged_tail(tabs, pairs, tail):
    """no whole row follows the loop: the state is multiplied back by x^-8064
    (xlB[63]) and the ragged tail goes on in A form"""
    L = 2 * pairs * ROW + tail
    seg = orc.gen_block(0xB7, tail, L).tobytes()
    B = rows_b_form(tabs, seg, 2 * pairs)
    inv = int(tabs["xlb"][63])
    A = [mulmod(inv, int(b)) for b in B]
    tail_ref = 2 * pairs * ROW
    A, lend = ragged_rows(tabs, seg, tail_ref, A, [0] * 64)
    assert segment_end(tabs, L, A, lend, tail_ref, tabs["crcx"][:64]) == orc.crc32c(seg)
