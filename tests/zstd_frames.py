"""Zstandard frames built sequence by sequence, a model that decodes them and a
census of what they make the block-parallel decoder do (test data and checker
only; juicefs_amd/csrc/jfsx_zstd2.h is the code under test).

Builder.  A compressed block whose three sequence tables are in RLE mode
spends no FSE state bits, and with raw or RLE literals its bitstream is only
the sequences' extra bits (RFC 8878 3.1.1.3).  Inside such a block every
sequence shares one literal-length code, one match-length code and one offset
code, so `ll`, `ml` and the offset are free inside their code's band only; the
codes change freely from block to block, and a table in repeat mode takes the
previous block's code.

Model.  Python integers and a bytearray: the repeat-offset rules of RFC 8878
3.1.1.5, literal copies, overlapping match copies, last literals.  It returns
the bytes and a trace of resolved (ll, ml, offset, repeat form) per sequence.

Census.  The stepping rule of decompress_par restated over the trace: steps of
64 sequences of a block, the step's regime by its output bytes (A byte-parallel
up to kWinBytes, B through the LDS ring up to kWinMax, C straight to dst), the
ring's F / V / W, and per step the cells REQUIRED lists.  It also restates the
kernel's dependency mask and raises if the mask misses a lane a match really
reads from, or names a lane that is not earlier (that would never finish).

Two kinds of cell need sequences of different sizes inside one block, which
one shared match-length code cannot give: a full 64-sequence regime-A step
followed by a B or C step (64 sequences in 1024 bytes leave only the
exact-value codes), and lane 63 reading from all 63 earlier matches (its match
would be 61 times longer than theirs, and a code's band is narrower than a
factor of two).  For these the match-length table may be the predefined one
(PREDEF): its FSE states are chosen from the decoding table, last sequence
first, which takes no entropy encoder either.
"""
import functools

import numpy as np

# the kernel's constants (tests/test_zstd_frames.py compares them with jfsx_zstd2.h)
kWinBytes, kWinMax, kRing, kLitStage, kMaxBlk = 1024, 4096, 8192, 512, 64

LL_BASE = list(range(16)) + [16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384,
                             32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
REP = "rep"  # a table in repeat mode: (REP, code of the table it repeats)
PREDEF = "predefined"  # the match-length table in predefined mode (free ml per sequence)


def ll_code(v):
    return max(c for c in range(36) if LL_BASE[c] <= v)


def ml_code(v):
    return max(c for c in range(53) if ML_BASE[c] <= v)


def of_code(v):
    return v.bit_length() - 1


def of_band(c):
    """Offsets (not offset values) a new-offset code c >= 2 can carry."""
    return (1 << c) - 3, (2 << c) - 4


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------
# blocks: ("raw", bytes) | ("rle", byte, n) | ("cmp", lits, seqs, codes)
#   lits: bytes (raw literals) or (byte, n) (RLE literals)
#   seqs: [(ll, ml, offset_value)]; offset_value 1..3 are the repeat codes
#   codes: (ll, of, ml), each None (RLE mode, the code of the first sequence),
#          an int (RLE mode, that code) or (REP, code); ml may also be PREDEF
# ---------------------------------------------------------------------------
def raw(data):
    return ("raw", bytes(data))


def rle(byte, n):
    return ("rle", byte, n)


def cmp_(lits, seqs, codes=(None, None, None)):
    return ("cmp", lits, list(seqs), tuple(codes))


def _codes(seqs, codes):
    out = []
    for k, (c, fn) in enumerate(zip(codes, (ll_code, of_code, ml_code))):
        v = seqs[0][(0, 2, 1)[k]]
        if c is None:
            out.append((1, fn(v)))
        elif c == PREDEF:
            assert k == 2
            out.append((0, None))
        elif isinstance(c, tuple):
            out.append((3, c[1]))
        else:
            out.append((1, c))
    return out


@functools.lru_cache(maxsize=None)
def _ml_predefined():
    """The decoding table of the predefined match-length distribution (RFC
    8878 3.1.1.3.2.2.3, accuracy log 6; table layout of 4.1.1): per state
    (symbol, bits to read, base of the next state)."""
    norm = [1, 4, 3, 2, 2, 2, 2, 2, 2] + [1] * 37 + [-1] * 7
    tab, high, pos = [0] * 64, 63, 0
    for s, p in enumerate(norm):
        if p == -1:
            tab[high] = s
            high -= 1
    for s, p in enumerate(norm):
        for _ in range(max(p, 0)):
            tab[pos] = s
            pos = (pos + 43) & 63
            while pos > high:
                pos = (pos + 43) & 63
    nxt = [1 if p == -1 else p for p in norm]
    ent = []
    for u in range(64):
        s = tab[u]
        nb = 6 - (nxt[s].bit_length() - 1)
        ent.append((s, nb, (nxt[s] << nb) - 64))
        nxt[s] += 1
    return ent


def _ml_states(mcodes):
    """FSE states that make the predefined table emit mcodes: chosen from the
    last sequence back, since the states of one symbol send their next-state
    ranges to a partition of all 64 states.  Returns per sequence (state, bits
    that lead to the next sequence's state, their count)."""
    ent = _ml_predefined()
    res, nxt = [], None
    for c in reversed(mcodes):
        for u, (s, nb, base) in enumerate(ent):
            if s == c and (nxt is None or base <= nxt < base + (1 << nb)):
                res.append((u, 0 if nxt is None else nxt - base, 0 if nxt is None else nb))
                nxt = u
                break
        else:
            raise AssertionError(("no state", c))
    return res[::-1]


def _bitstream(seqs, llc, ofc, mlc):
    out, acc, n = bytearray(), 0, 0
    st = _ml_states([ml_code(s[1]) for s in seqs]) if mlc is None else None
    for k in range(len(seqs) - 1, -1, -1):
        s = seqs[k]
        mc = ml_code(s[1]) if mlc is None else mlc
        fields = [(s[0], LL_BASE[llc], LL_BITS[llc]), (s[1], ML_BASE[mc], ML_BITS[mc]), (s[2], 1 << ofc, ofc)]
        if st:  # read after the sequence's extra bits, so written before them
            fields.insert(0, (st[k][1], 0, st[k][2]))
        for v, base, nb in fields:
            x = v - base
            assert 0 <= x < (1 << nb) or (nb == 0 and x == 0), ("value outside its code's band", s, base, nb)
            acc |= x << n
            n += nb
        while n >= 64:
            out += (acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little")
            acc >>= 64
            n -= 64
    if st:  # the initial state: the first bits read
        acc |= st[0][0] << n
        n += 6
    acc |= 1 << n
    n += 1
    return bytes(out) + acc.to_bytes((n + 7) // 8, "little")


def _lit_section(lits):
    if isinstance(lits, tuple):
        ltype, size, body = 1, lits[1], bytes([lits[0]])
    else:
        ltype, size, body = 0, len(lits), bytes(lits)
    if size < 32:
        h = bytes([ltype | size << 3])
    elif size < 4096:
        h = (ltype | 1 << 2 | size << 4).to_bytes(2, "little")
    else:
        assert size < (1 << 20)
        h = (ltype | 3 << 2 | size << 4).to_bytes(3, "little")
    return h + body


def _cmp_bytes(lits, seqs, codes):
    out = _lit_section(lits)
    n = len(seqs)
    if n == 0:
        return out + b"\x00"
    if n < 128:
        out += bytes([n])
    elif n < 0x7F00:
        out += bytes([(n >> 8) + 0x80, n & 255])
    else:
        out += b"\xff" + (n - 0x7F00).to_bytes(2, "little")
    (lm, llc), (om, ofc), (mm, mlc) = _codes(seqs, codes)
    out += bytes([lm << 6 | om << 4 | mm << 2])
    for mode, c in ((lm, llc), (om, ofc), (mm, mlc)):
        if mode == 1:
            out += bytes([c])
    return out + _bitstream(seqs, llc, ofc, mlc)


def frame(blocks, fcs=None):
    """The frame's bytes: magic, descriptor 0xA0 (single segment, 4-byte
    content size), the blocks.  fcs defaults to the model's decoded size."""
    if fcs is None:
        fcs = len(decode(blocks)[0])
    out = b"\x28\xb5\x2f\xfd\xa0" + fcs.to_bytes(4, "little")
    for i, b in enumerate(blocks):
        last = 1 if i == len(blocks) - 1 else 0
        if b[0] == "raw":
            out += (len(b[1]) << 3 | 0 << 1 | last).to_bytes(3, "little") + b[1]
        elif b[0] == "rle":
            out += (b[2] << 3 | 1 << 1 | last).to_bytes(3, "little") + bytes([b[1]])
        else:
            body = _cmp_bytes(b[1], b[2], b[3])
            assert 3 <= len(body) < (128 << 10)
            out += (len(body) << 3 | 2 << 1 | last).to_bytes(3, "little") + body
    return out


# ---------------------------------------------------------------------------
# model
# ---------------------------------------------------------------------------
class Invalid(ValueError):
    pass


def decode(blocks):
    """(bytes, trace).  trace: per block a dict with kind ('raw', 'rle', 'cmp'),
    o (output position at entry), size, and for 'cmp': ltype, litsize, seqs
    [(ll, ml, off, form)], modes (True where the table is set, False where
    repeated; None without sequences), new (new offsets in the block)."""
    out = bytearray()
    rep = [1, 4, 8]
    trace = []
    for b in blocks:
        o = len(out)
        if b[0] == "raw":
            out += b[1]
            trace.append(dict(kind="raw", o=o, size=len(b[1])))
            continue
        if b[0] == "rle":
            out += bytes([b[1]]) * b[2]
            trace.append(dict(kind="rle", o=o, size=b[2]))
            continue
        lits, seqs, codes = b[1], b[2], b[3]
        if isinstance(lits, tuple):
            ltype, lit = 1, bytes([lits[0]]) * lits[1]
        else:
            ltype, lit = 0, bytes(lits)
        lp, new, res = 0, 0, []
        for ll, ml, ov in seqs:
            if ll > len(lit) - lp:
                raise Invalid("literal length past the literals")
            out += lit[lp:lp + ll]
            lp += ll
            if ov > 3:
                off, form = ov - 3, "new"
                rep = [off, rep[0], rep[1]]
                new += 1
            else:
                idx = ov + (1 if ll == 0 else 0)
                if idx == 1:
                    off, form = rep[0], "rep1"
                elif idx == 2:
                    off, form = rep[1], "rep2_ll0" if ll == 0 else "rep2"
                    rep = [rep[1], rep[0], rep[2]]
                elif idx == 3:
                    off, form = rep[2], "rep3"
                    rep = [rep[2], rep[0], rep[1]]
                else:
                    off, form = rep[0] - 1, "rep1m1"
                    if off == 0:
                        off, form = 1, "clamp"
                    rep = [off, rep[0], rep[1]]
                if new >= 3:
                    form = "late_" + form
            if off > len(out):
                raise Invalid("offset past the output")
            if off >= ml:
                out += out[len(out) - off:len(out) - off + ml]
            else:
                seg = bytes(out[len(out) - off:])
                out += (seg * (ml // off + 1))[:ml]
            res.append((ll, ml, off, form))
        out += lit[lp:]
        modes = tuple(not isinstance(c, tuple) for c in codes) if seqs else None
        trace.append(dict(kind="cmp", o=o, size=len(out) - o, ltype=ltype, litsize=len(lit), seqs=res, modes=modes,
                          new=new))
    return bytes(out), trace


# ---------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------
FORMS = ("rep1", "rep2_ll0", "rep2", "rep3", "rep1m1", "clamp")
POSITIONS = ("frame_start", "after_ge3", "after_lt3", "via_raw", "via_rle", "via_zeroseq")
MASK_CELLS = ("mask0_literals", "one", "several", "lane63_all", "start_at_end", "start_at_end_m1", "start_at_end_p1",
              "end_at_start", "end_at_start_m1", "end_at_start_p1")

REQUIRED = (
    ["tall_1024", "tall_1025", "tall_4096", "tall_4097", "nvalid_1", "nvalid_63", "nvalid_64"] +
    ["%s_%s" % (r, t) for r in "ABC" for t in ("raw", "rle")] +
    ["A_tll_509_staged", "A_tll_510_unstaged", "A_src_dst", "A_src_ring", "A_src_step", "A_chain32", "A_no_literals",
     "A_no_step_source"] + ["A_overlap_off%d" % d for d in (1, 2, 3, 15, 16, 17)] +
    ["B_far_ml32", "B_ml33_not_far", "B_off_eq_ml", "B_straddle_lim", "B_loop_off_ge4", "B_loop_off_lt4"] +
    ["mask_%s_%s" % (r, c) for r in "BC" for c in MASK_CELLS] +
    ["C_off1", "C_off_ml_minus_1", "C_off_ge_ml"] +
    ["flush_A", "flush_B", "cross8192_A", "cross8192_B"] + ["pair_%s%s" % (x, y) for x in "ABC" for y in "ABC"] +
    ["after_raw_A", "after_raw_B", "after_rle_A", "after_rle_B"] +
    ["last_%d_after_%s" % (n, r) for n in (0, 1, 4096, 4097) for r in "ABC"] + ["last_rle"] +
    ["rep_%s_%s" % (f, p) for f in FORMS for p in POSITIONS] +
    ["tabrep_%s_%s" % (t, v) for t in ("LL", "OF", "ML") for v in ("direct", "via_raw", "via_zeroseq")] +
    ["nbseq_127", "nbseq_128", "nbseq_0x7EFF", "nbseq_0x7F00", "blocks_64", "blocks_65"] +
    ["twin_off_first", "twin_off_lane63_A", "twin_off_lane63_B", "twin_off_lane63_C"])


def lane_cells(lanes, j, off, ml, o):
    """Dependency cells of lane j's match (offset off, length ml) against the
    earlier lanes' (oj, mo, oend); and the true dependency set."""
    mo = lanes[j][1]
    ms = mo - off
    need = ms + min(off, ml)
    deps = [i for i in range(j) if lanes[i][1] < need and lanes[i][2] > ms]
    cells = set()
    if need > o:
        if not deps and ms >= o:
            cells.add("mask0_literals")
        if len(deps) == 1:
            cells.add("one")
        if len(deps) >= 2:
            cells.add("several")
        if j == 63 and len(deps) == 63:
            cells.add("lane63_all")
    for i in range(j):
        d = ms - lanes[i][2]
        if -1 <= d <= 1:
            cells.add("start_at_end" + ("_m1", "", "_p1")[d + 1])
        d = need - lanes[i][1]
        if -1 <= d <= 1:
            cells.add("end_at_start" + ("_m1", "", "_p1")[d + 1])
    return cells, deps


def _kernel_mask(lanes, j, off, ml, o, tall):
    """decompress_par's dependency mask of lane j as a set of lanes (wave_count_le
    over the 64 lanes; the kernel's invalid lanes sit at the step's end)."""
    pad = (o + tall, o + tall, o + tall)
    L = list(lanes) + [pad] * (64 - len(lanes))
    mo = L[j][1]
    ms = mo - off
    need = ms + min(off, ml)
    ks = sum(1 for x in L if x[2] <= ms)
    ke1 = sum(1 for x in L if x[0] <= need - 1)
    mks, mke = L[ks & 63][1], L[(ke1 - 1) & 63][1]
    if need > o and ke1 > 0:
        s0 = ks if need > mks else ks + 1
        e0 = ke1 - 1 if need > mke else ke1 - 2
        if s0 <= e0 and 0 <= e0 < 64:
            return set(range(s0, e0 + 1))
    return set()


def _flush_part(F, W, a):
    if W + a < 16:
        return F
    end = ((W + a) & ~15) - a
    return max(F, end)


def census(trace, a=0):
    """The set of cells a frame reaches when decoded at dst mod 16 == a."""
    cells = set()
    F = V = W = 0
    prev = None          # kind of the block before: 'raw', 'rle', 'zero', 'seq'
    hist = []            # the blocks with sequences so far: (modes, new, kinds of the blocks since the previous one)
    between = []
    nseqblk = 0
    for b in trace:
        assert b["o"] == W
        if b["kind"] != "cmp":
            F = V = W = W + b["size"]
            prev = b["kind"]
            between.append(prev)
            continue
        seqs, ltype = b["seqs"], b["ltype"]
        lt = "rle" if ltype else "raw"
        n = len(seqs)
        for v, nm in ((127, "127"), (128, "128"), (0x7EFF, "0x7EFF"), (0x7F00, "0x7F00")):
            if n == v:
                cells.add("nbseq_" + nm)
        if n:
            nseqblk += 1
            # repeat-offset forms by the block's position in the frame
            if not hist:
                pos = "frame_start"
            elif "raw" in between:
                pos = "via_raw"
            elif "rle" in between:
                pos = "via_rle"
            elif "zero" in between:
                pos = "via_zeroseq"
            else:
                pos = "after_ge3" if hist[-1][1] >= 3 else "after_lt3"
            for k, s in enumerate(seqs):
                if s[3] in FORMS:
                    if s[3] == "clamp" and pos != "frame_start" and not (k and seqs[k - 1][3] == "rep1m1"):
                        continue  # the clamp counts at the end of a run of rep1 - 1
                    cells.add("rep_%s_%s" % (s[3], pos))
            hist.append((b["modes"], b["new"], list(between)))
            between = []
            if len(hist) >= 3:
                (m0, _, _), (m1, _, b1), (m2, _, b2) = hist[-3:]
                for t, nm in enumerate(("LL", "OF", "ML")):
                    others = [x for x in range(3) if x != t]
                    if m0[t] and not m1[t] and not m2[t] and all(m1[x] and m2[x] for x in others):
                        via = b1 + b2
                        cells.add("tabrep_%s_%s" % (nm, "via_raw" if "raw" in via else
                                                    "via_zeroseq" if "zero" in via else "direct"))
        else:
            between.append("zero")
        lp, last_reg = 0, None
        for w in range(0, n, 64):
            st = seqs[w:w + 64]
            o = W
            tll = sum(s[0] for s in st)
            tall = tll + sum(s[1] for s in st)
            reg = "A" if tall <= kWinBytes else "B" if tall <= kWinMax else "C"
            cells.add("%s_%s" % (reg, lt))
            if tall in (1024, 1025, 4096, 4097):
                cells.add("tall_%d" % tall)
            if len(st) in (1, 63, 64):
                cells.add("nvalid_%d" % len(st))
            if w == 0 and prev in ("raw", "rle") and reg in "AB":
                cells.add("after_%s_%s" % (prev, reg))
            if last_reg:
                cells.add("pair_%s%s" % (last_reg, reg))
            lanes, p = [], o
            for ll, ml, off, _ in st:
                lanes.append((p, p + ll, p + ll + ml))
                p += ll + ml
            if b["o"] == 0 and w == 0 and st[0][2] == st[0][0] and trace[0] is b:
                cells.add("twin_off_first")
            if len(st) == 64 and st[63][2] == lanes[63][1]:
                cells.add("twin_off_lane63_" + reg)
            if reg == "C":
                F = V = o + tall
            else:
                if o - F >= kWinMax:
                    F = _flush_part(F, W, a)
                    cells.add("flush_" + reg)
                old = max(o + tall - kRing, 0)
                assert old <= F, "a step would read unflushed bytes from dst"
                lim = max(V, old)
                if o // kRing != (o + tall - 1) // kRing and old > 0:
                    cells.add("cross8192_" + reg)
            if reg == "A":
                if ltype == 0 and tll == 509:
                    assert tll + 3 <= kLitStage
                    cells.add("A_tll_509_staged")
                if ltype == 0 and tll == 510:
                    assert tll + 3 > kLitStage
                    cells.add("A_tll_510_unstaged")
                if tll == 0:
                    cells.add("A_no_literals")
                depth, owner, instep = [0] * tall, [0] * tall, False
                for k, ((oj, mo, oend), (ll, ml, off, _)) in enumerate(zip(lanes, st)):
                    if off < ml and off in (1, 2, 3, 15, 16, 17):
                        cells.add("A_overlap_off%d" % off)
                    for r in range(oj - o, oend - o):
                        owner[r] = k
                    for r in range(mo - o, oend - o):
                        q = o + r - off
                        if q >= o:
                            instep = True
                            cells.add("A_src_step")
                            depth[r] = depth[q - o] + (1 if owner[q - o] != k else 0)
                        else:
                            cells.add("A_src_dst" if q < lim else "A_src_ring")
                if not instep:
                    cells.add("A_no_step_source")
                if tall and max(depth) >= 32:
                    cells.add("A_chain32")
            else:
                for k, ((oj, mo, oend), (ll, ml, off, _)) in enumerate(zip(lanes, st)):
                    ms = mo - off
                    need = ms + min(off, ml)
                    lc, deps = lane_cells(lanes, k, off, ml, o)
                    km = _kernel_mask(lanes, k, off, ml, o, tall)
                    assert set(deps) <= km, ("the kernel's mask misses a lane", k, deps, km)
                    assert all(i < k for i in km), ("the kernel's mask names a lane that is not earlier", k, km)
                    cells.update("mask_%s_%s" % (reg, c) for c in lc)
                    if reg == "B":
                        far = ml <= 32 and off >= ml and ms + ml <= lim
                        if far and ml == 32:
                            cells.add("B_far_ml32")
                        if ml == 33 and off >= ml and ms + ml <= lim:
                            cells.add("B_ml33_not_far")
                        if off == ml:
                            cells.add("B_off_eq_ml")
                        if ms < lim < need:
                            cells.add("B_straddle_lim")
                        if not far:
                            cells.add("B_loop_off_ge4" if off >= 4 else "B_loop_off_lt4")
                    else:
                        if off == 1:
                            cells.add("C_off1")
                        if off == ml - 1:
                            cells.add("C_off_ml_minus_1")
                        if off >= ml:
                            cells.add("C_off_ge_ml")
            W = o + tall
            lp += tll
            last_reg = reg
        last = b["litsize"] - lp
        if last_reg and last in (0, 1, 4096, 4097):
            cells.add("last_%d_after_%s" % (last, last_reg))
        if last and ltype == 1:
            cells.add("last_rle")
        if last <= kWinMax:
            if W - F >= kWinMax:
                F = _flush_part(F, W, a)
        else:
            F = V = W + last
        W += last
        prev = "seq" if n else "zero"
    if nseqblk == len(trace) and len(trace) == 64:
        cells.add("blocks_64")
    if len(trace) == 65:
        cells.add("blocks_65")
    return cells


# ---------------------------------------------------------------------------
# corpus
# ---------------------------------------------------------------------------
def spread(total, n, lo, hi):
    q, r = divmod(total - lo * n, n)
    assert total >= lo * n and lo + q + (1 if r else 0) <= hi
    return [lo + q + (1 if i < r else 0) for i in range(n)]


def seqblock(o, lls, mls, ofc, want=None, rle_lits=None, last=0, seed=0, valid=True, ml_mode=None):
    """A compressed block of new offsets under offset code ofc at output
    position o: per sequence an offset inside the code's band that stays inside
    the output (want: {sequence index: offset}).  Returns (block, positions)."""
    lo, hi = of_band(ofc)
    seqs, pos, p = [], [], o
    for k, (ll, ml) in enumerate(zip(lls, mls)):
        mo = p + ll
        if want and k in want:
            off = want[k]
        else:
            h = min(hi, mo)
            assert lo <= h, ("no offset of this code fits here", k, mo, lo)
            off = lo + (k * 37 + seed * 11 + 5) % (h - lo + 1)
        assert lo <= off <= (min(hi, mo) if valid else hi), (k, off, lo, hi, mo)
        seqs.append((ll, ml, off + 3))
        pos.append((p, mo, mo + ml))
        p = mo + ml
    nlit = sum(lls) + last
    lits = (rle_lits, nlit) if rle_lits is not None else rnd(nlit, 1000 + seed)
    return cmp_(lits, seqs, (None, None, ml_mode)), pos


def _mask_block(o, lls, mls, ofc, reg, seed):
    """One 64-sequence step whose offsets are searched, lane by lane, for the
    dependency cells (positions do not depend on the offsets)."""
    lo, hi = of_band(ofc)
    _, pos = seqblock(o, lls, mls, ofc, seed=seed)
    want, todo = {}, [c for c in MASK_CELLS if c != "lane63_all"]
    for j in range(63, 0, -1):
        if not todo:
            break
        for off in range(lo, min(hi, pos[j][1]) + 1):
            got, _ = lane_cells(pos, j, off, mls[j], o)
            hit = [c for c in todo if c in got]
            if hit:
                want[j] = off
                todo.remove(hit[0])
                break
    return seqblock(o, lls, mls, ofc, want=want, seed=seed)[0]


def _lane63_twin(reg, bump=0):
    lls, mls = {"A": ([5] * 64, [10] * 64), "B": ([35] * 64, [16] * 64), "C": ([70] * 64, [10] * 64)}[reg]
    rel = sum(lls) + sum(mls) - mls[63]  # lane 63's match start in the step
    for c in range(4, 16):
        lo, hi = of_band(c)
        P = lo  # the prefix: lane 0 can reach back lo bytes
        if P + rel + bump <= hi:
            return [raw(rnd(P, 70 + c)), seqblock(P, lls, mls, c, want={63: P + rel + bump}, seed=c, valid=not bump)[0]]
    raise AssertionError(reg)


def _build():
    F = {}

    def add(name, blocks):
        assert name not in F
        F[name] = blocks

    P = lambda n, s=1: raw(rnd(n, s))  # noqa: E731
    # step sizes at the regime edges, raw and RLE literals
    shapes = {1024: ([13] * 64, 5), 1025: ([16 + (k % 52 >= 15) for k in range(52)], 5),
              4096: (spread(3904, 64, 48, 63), 6), 4097: (spread(3905, 64, 48, 63), 6)}
    for T, (lls, ofc) in shapes.items():
        assert sum(lls) + 3 * len(lls) == T
        for lt in (None, 0x5A):
            add("tall_%d_%s" % (T, "rle" if lt else "raw"),
                [P(200, T), seqblock(200, lls, [3] * len(lls), ofc, rle_lits=lt, seed=T)[0]])
    for T, off in ((1024, 1), (1025, 2), (4096, 3), (4097, 4), (2500, 1), (3000, 3)):
        add("one_seq_%d_off%d" % (T, off), [P(8, T), cmp_(b"", [(0, T, off + 3)])])
    add("one_seq_5000_off4999", [P(5000, 2), cmp_(b"xy", [(2, 5000, 4999 + 3)])])
    # literal staging of the byte-parallel step, at each source alignment
    for tll in (509, 510):
        for k in range(4):
            add("stage_%d_%d" % (tll, k),
                [P(64 + k, k), seqblock(64 + k, spread(tll, 14, 32, 39), [3] * 14, 5, seed=k)[0]])
    # regime A sources
    add("a_src_ring", [P(100), cmp_(rnd(300, 3), []), seqblock(400, [3] * 20, [8] * 20, 7, seed=1)[0]])
    add("a_overlap", [P(64), cmp_(rnd(14, 4), [(2, 20, 1 + 3), (2, 20, 2 + 3), (2, 20, 3 + 3), (2, 20, 4 + 3),
                                              (2, 20, 1 + 3), (2, 20, 3 + 3), (2, 20, 2 + 3)]),
                      cmp_(rnd(12, 5), [(2, 20, d + 3) for d in (15, 16, 17, 16, 15, 17)])])
    add("a_chain_5", [P(64), cmp_(b"", [(0, 5, 5 + 3)] * 40)])
    add("a_chain_7", [P(64, 2), cmp_(b"", [(0, 7, 5 + 3)] * 64 + [(0, 7, 6 + 3)] * 8)])
    add("a_far_only", [P(2000), seqblock(2000, [2] * 20, [6] * 20, 10, seed=2)[0]])
    # regime B copy loops
    for ml in (32, 33):
        add("b_ml%d" % ml, [P(600, ml), seqblock(600, [5] * 64, [ml] * 64, 8, want={7: 37 * 7 + 20}, seed=ml)[0]])
    add("b_off_eq_ml", [P(600, 3), seqblock(600, [5] * 64, [32] * 64, 5, want={k: 32 for k in range(0, 64, 3)})[0]])
    add("b_off_small", [P(64, 4), seqblock(64, [7] * 64, [39 + k % 2 for k in range(64)], 2,
                                           seed=3)[0]])
    add("b_off_small_rle", [P(64, 5), seqblock(64, [3] * 64, [40] * 64, 2, rle_lits=0x33, seed=4)[0]])
    # dependency masks
    add("mask_B1", [P(600, 6), _mask_block(600, [32 + (k * 5) % 8 for k in range(64)], [16] * 64, 8, "B", 1)])
    add("mask_B2", [P(300, 7), _mask_block(300, [0] * 64, [51 + (k * 3) % 8 for k in range(64)], 7, "B", 2)])
    add("mask_C1", [P(1100, 8), _mask_block(1100, [64 + (k * 11) % 64 for k in range(64)], [16] * 64, 9, "C", 3)])
    add("mask_C2", [P(600, 9), _mask_block(600, [0] * 64, [67 + (k * 5) % 16 for k in range(64)], 8, "C", 4)])
    add("mask_C2_rle", [rle(7, 600), _mask_block(600, [1] * 64, [67 + (k * 5) % 16 for k in range(64)], 8, "C", 5)])
    add("c_lane_match", [P(200, 10), seqblock(200, [64 + k for k in range(64)], [4] * 64, 2,
                                              want={k: (1, 3, 4, 2)[k % 4] for k in range(64)})[0]])
    # last literals after each regime; steps after raw, RLE blocks
    steps = {"A": ([3] * 10, [5] * 10, 5), "B": ([20] * 64, [10] * 64, 6), "C": ([70] * 64, [10] * 64, 7)}
    for reg, (lls, mls, ofc) in steps.items():
        for last in (0, 1, 4096, 4097):
            add("last_%d_after_%s" % (last, reg), [P(150, last), seqblock(150, lls, mls, ofc, last=last, seed=last)[0]])
        add("last_rle_after_%s" % reg, [rle(0x41, 150), seqblock(150, lls, mls, ofc, last=4097, rle_lits=0x42)[0],
                                        seqblock(150 + sum(lls) + sum(mls) + 4097, lls, mls, ofc, last=1,
                                                 rle_lits=0x43)[0]])
    add("ends_raw", [P(64, 6), seqblock(64, [3] * 10, [5] * 10, 5)[0], P(50, 7)])
    # partial flushes: 4096 bytes in the ring, then a step
    for reg in "AB":
        lls, mls, ofc = steps[reg]
        add("flush_" + reg, [cmp_(rnd(4096, 11), []), seqblock(4096, lls, mls, ofc, last=5, seed=6)[0],
                             seqblock(4101 + sum(lls) + sum(mls), lls, mls, ofc, seed=7)[0]])
    # the ring wraps: many A steps, many B steps, sources in the ring and in dst
    o, blocks = 1100, [P(1100, 12)]
    for lls, mls, ofc, nst in (([5] * 64, [10] * 64, 9, 12), ([32 + k % 8 for k in range(64)], [16] * 64, 12, 6),
                               ([4] * 64, [9] * 64, 12, 10), ([6] * 64, [8] * 64, 11, 5),
                               ([30] * 64, [33] * 64, 13, 3)):
        blk, pos = seqblock(o, lls * nst, mls * nst, ofc, last=7, seed=ofc + nst)
        blocks.append(blk)
        o = pos[-1][2] + 7
    add("ring_wrap", blocks)
    # consecutive regimes inside one block (ll code 24: 48..63, ml 3)
    seq = [48] * 64 + [63] * 64 + [48] * 64 + [50] * 5
    b1, pos = seqblock(1100, seq, [3] * len(seq), 9, seed=8)
    seq2 = [63] * 128 + [55] * 3
    b2, pos2 = seqblock(pos[-1][2], seq2, [3] * len(seq2), 10, seed=9)
    seq3 = [50] * 128
    b3, _ = seqblock(pos2[-1][2], seq3, [3] * len(seq3), 11, seed=10)
    add("pairs", [P(1100, 13), b1, b2, b3])
    # with the predefined match-length table ml is free per sequence: a full A
    # step before a B and a C step, and lane 63 reading from all 63 earlier matches
    mls = [6] * 64 + [30] * 64 + [6] * 64 + [100] * 64 + [4] * 64 + [3, 40, 200]
    add("pairs_predefined", [P(1100, 60), seqblock(1100, [2] * len(mls), mls, 9, seed=11, ml_mode=PREDEF)[0]])
    add("lane63_all_B", [P(1100, 61), seqblock(1100, [16] * 64, [3] * 63 + [1190], 10, want={63: 1200}, seed=12,
                                               ml_mode=PREDEF)[0]])
    add("lane63_all_C", [P(2100, 62), seqblock(2100, [40] * 64, [3] * 63 + [2700], 11, want={63: 2720}, seed=13,
                                               ml_mode=PREDEF)[0]])
    # repeat offsets before a block has three new offsets, by position
    new3 = cmp_(rnd(12, 14), [(4, 5, 7 + 3), (4, 5, 9 + 3), (4, 5, 11 + 3)])
    new1 = cmp_(rnd(4, 15), [(4, 5, 6 + 3)])
    pre = {"frame_start": [P(64, 16)], "after_ge3": [P(64, 17), new3], "after_lt3": [P(64, 18), new1],
           "via_raw": [P(64, 19), new3, P(9, 20)], "via_rle": [P(64, 21), new3, rle(9, 5)],
           "via_zeroseq": [P(64, 22), new3, cmp_(b"zz", [])]}
    forms = {"rep1": cmp_(rnd(10, 23), [(2, 5, 1)] * 5),
             "rep2_ll0": cmp_(b"q", [(0, 5, 1)] * 5),
             "rep23": cmp_(rnd(12, 24), [(2, 5, v) for v in (2, 3, 3, 2, 3, 2)]),
             "rep3_ll0_m1": cmp_(b"", [(0, 6, v) for v in (2, 3, 2, 2, 3, 3)]),
             "clamp": cmp_(b"w", [(0, 4, 3)] * 14)}
    for pn, pb in pre.items():
        for fn, fb in forms.items():
            add("rep_%s_%s" % (fn, pn), pb + [fb, fb])
    # each table set in block k and repeated in k + 1 and k + 2
    vals = [((2, 5, 8), (2, 6, 17), (2, 9, 5)), ((2, 5, 9), (3, 6, 10), (5, 9, 12)), ((2, 5, 8), (3, 5, 20), (4, 5, 6))]
    for t, nm in enumerate(("LL", "OF", "ML")):
        for via, vb in (("direct", []), ("via_raw", [P(5, 25)]), ("via_zeroseq", [cmp_(b"k", [])])):
            bl = [P(64, 26 + t)]
            for k, s in enumerate(vals[t]):
                codes = [None, None, None]
                if k:
                    codes[t] = (REP, (ll_code, of_code, ml_code)[t](vals[t][0][(0, 2, 1)[t]]))
                    bl += vb
                bl.append(cmp_(rnd(3 * s[0] + k, 30 + k), [s] * 3, codes))
            add("tabrep_%s_%s" % (nm, via), bl)
    # sequence-count headers
    for n in (127, 128):
        add("nbseq_%d" % n, [P(64, n), seqblock(64, [1] * n, [3] * n, 3, seed=n)[0]])
    for n in (0x7EFF, 0x7F00):
        add("nbseq_0x%X" % n, [P(64, n), seqblock(64, [0] * n, [3] * n, 2, seed=n)[0]])
    # 64 blocks with sequences (the block-parallel decoder's limit), and 65
    for nb in (64, 65):
        add("blocks_%d" % nb, [cmp_(rnd(2 + i % 3, 40 + i), [(2, 3 + i % 5, 1 + i % 2 + 3)]) for i in range(nb)])
    # the valid twins of the rejects
    add("twin_off_first", [cmp_(b"abcdef", [(4, 8, 4 + 3)])])
    for reg in "ABC":
        add("twin_off_lane63_" + reg, _lane63_twin(reg))
    add("twin_ll_exact", [P(20, 50), cmp_(b"lit", [(3, 4, 5 + 3)])])
    return F


class Case:
    def __init__(self, name, blocks):
        self.name, self.blocks = name, blocks
        self.out, self.trace = decode(blocks)
        self.frame = frame(blocks, len(self.out))
        self.serial = len(blocks) > kMaxBlk  # expected at the serial decoder


@functools.lru_cache(maxsize=None)
def corpus():
    """[Case]: every frame decodes to at most 1 MiB, the corpus to far less than 64 MiB."""
    return [Case(n, b) for n, b in _build().items()]


ALIGN_CASE = "ring_wrap"  # decoded at every dst mod 16 by the GPU test


@functools.lru_cache(maxsize=None)
def rejects():
    """[(name, frame, dst_cap)]: valid frames with one value moved by one."""
    by = {c.name: c for c in corpus()}
    P = lambda n, s=1: raw(rnd(n, s))  # noqa: E731
    R = [("off_first", frame([cmp_(b"abcdef", [(4, 8, 5 + 3)])], 14), 14)]
    for reg in "ABC":
        n = len(by["twin_off_lane63_" + reg].out)
        R.append(("off_lane63_" + reg, frame(_lane63_twin(reg, 1), n), n))
    R.append(("ll_past_literals", frame([P(20, 50), cmp_(b"lit", [(4, 4, 5 + 3)])], 28), 28))
    R.append(("repeat_mode_first_block",
              frame([cmp_(b"abcdef", [(4, 8, 4 + 3)], ((REP, 4), (REP, 2), (REP, 5)))], 14), 14))
    for nm, src in (("cap_step_A", "last_0_after_A"), ("cap_step_B", "last_0_after_B"),
                    ("cap_step_C", "last_0_after_C"), ("cap_raw", "ends_raw"), ("cap_last_literals", "last_1_after_A")):
        c = by[src]
        R.append((nm, c.frame, len(c.out) - 1))
    return R
