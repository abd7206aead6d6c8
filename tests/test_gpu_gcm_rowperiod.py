"""The four-row period of the 16-wave AES-GCM kernel against the oracle.

From a task row = 0 mod 4 (lane-0 counter low byte 2) the kernel runs four rows
per iteration: the counter-uniform terms of rounds 1-2 are read once, the
rounds-1-2 table P is read at the lane's base plus a constant (row 3's lanes
62-63 reach P[256], P[257], copies of P[0], P[1]), only row 3 can end a
segment, and the rows' data registers alternate between two sets.  A stream
that starts on a row = 2 mod 4 runs one two-row iteration first; two or three
rows left over run one more, then the single-row loop.

Modes: Seal with the plaintext CRC, GEN and VERIFY (a clean image, and one
with a wrong stored CRC that must report its segment), Seal without a CRC,
Open with the plaintext CRC, Open with JFSX_CRC_CT.  Each runs on the default
context and on a JFSX_CTX_CRC_LDS context.  Tags, outputs, CRC arrays and
reports are compared with the oracle's (tests/test_gpu_gcm_rowloop.py has the
reference class).

Batches, by what the plan makes of them:

  * "whole": the lengths behind 2 GiB of unchecked filler, so that the plan
    keeps 4 MiB tasks and every block below is one task.  32 KiB: two rows per
    stream, no period (the control).  64 KiB: one aligned period per stream,
    and a segment ends in row 3 of wave 7's and wave 15's.  96 KiB: six rows
    per stream, odd waves start on a row = 2 mod 4 (a two-row iteration, then
    a period), even waves run a period, then two rows.  98 KiB: 49 row pairs,
    streams of three and four pairs.  97 KiB: the last stream ends on a single
    row.  64 KiB + 1000 and 1 MiB + 17: ragged tails after B form, the second
    with the counter in its third byte.  4 MiB: 256 KiB per stream, 64
    periods, eight segment ends and a refill of the counter window.
  * "cut": a small batch, which the plan cuts into 64 KiB tasks, so tasks
    start inside blocks, at nonzero offsets and counters (asserted).
  * "keys": 600 blocks of 64 KiB, each with a key of its own: every workgroup
    takes several tasks and rebuilds P, its two tail entries and the period's
    scalars for each.
"""
import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import test_gpu_gcm_rowloop as RL

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
SPLIT = 192 * KIB + 1000
WHOLE = [32 * KIB, 64 * KIB, 96 * KIB, 98 * KIB, 97 * KIB, 64 * KIB + 1000, MIB + 17, 4 * MIB]
CUT = [32 * KIB, 64 * KIB, 96 * KIB, 98 * KIB, 64 * KIB + 1000, MIB + 17, SPLIT]
PATHS = (("default", 0), ("lds", E.CTX_CRC_LDS))
FILL = 8 * MIB


@pytest.fixture(scope="module")
def ref_whole():
    r = RL.Ref(0x5251, WHOLE, WHOLE.index(4 * MIB), 77, fill=[FILL] * 255)
    tb, _, tasks = E.debug_plan(E.PLAN_GCM, r.lens + r.fill)
    assert tb == 4 * MIB, "the plan keeps 4 MiB tasks"
    for i, n in enumerate(WHOLE):
        assert (i, 0, n) in tasks, "block %d (len %d) is one task" % (i, n)
    return r


@pytest.fixture(scope="module")
def ref_cut():
    r = RL.Ref(0x5252, CUT, CUT.index(MIB + 17), 20)
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    starts = sorted(c0 for b, c0, _ in tasks if b == CUT.index(SPLIT))
    assert len(starts) > 1 and starts[0] == 0 and starts[1] > 0, "the plan cuts the block: a task starts inside it"
    return r


@pytest.fixture(scope="module")
def ref_keys():
    r = RL.Ref(0x5253, [64 * KIB] * 600, 311, 1)
    assert len({k for k, _ in r.keys}) == r.n, "a key of its own per block"
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    assert sorted(tasks) == [(i, 0, 64 * KIB) for i in range(600)], "one 64 KiB task per block"
    return r


class Run(RL.Run):
    """The row-loop test's four modes, then Seal without a CRC and Open with the plaintext CRC."""

    def run(self):
        r, gcm, dev = self.ref, E.AES256GCM, E.MEM_DEVICE
        # the outputs are compared padding included, and a fresh allocation may hold anything
        self.dst.upload(np.zeros(r.bytes, np.uint8))
        super().run()
        stale = np.full(r.cbytes, 0xEE, np.uint8)
        # (the source holds the ciphertexts after open_ct)
        self.crc.upload(stale)
        self.dst.upload(np.zeros(r.bytes, np.uint8))
        arr, n = self.blocks(r.tag)
        self.eng.open_batch(gcm, arr, n, E.CRC_GEN, dev)
        self.keep("open_pt", arr)
        self.src.upload(r.pack(r.p))
        self.crc.upload(stale)
        self.dst.upload(np.zeros(r.bytes, np.uint8))
        arr, n = self.blocks()
        self.eng.seal_batch(gcm, arr, n, E.CRC_NONE, dev)
        self.keep("seal_none", arr)


def block_failures(r, out):
    """Every (mode, block, length, what differs) of a run, block by block, so that a failure names all the
    lengths it touches and not only the first."""
    stale = [b"\xee" * len(c) for c in r.crc_p]
    crc_p, crc_c = [bytes(c) for c in r.crc_p], [bytes(c) for c in r.crc_c]
    want = {"seal_gen": (r.c, crc_p), "seal_verify": (r.c, None), "seal_verify_bad": (r.c, None),
            "open_ct": (r.p, crc_c), "open_pt": (r.p, crc_p), "seal_none": (r.c, stale)}
    bad = []
    for mode, (datas, crcs) in want.items():
        o = out[mode]
        for i in range(r.n):
            a, n = r.off[i], r.lens[i]
            if o["tags"][i] != r.tag[i]:
                bad.append((mode, i, n, "tag"))
            got, ref = o["data"][a:a + n], np.frombuffer(bytes(datas[i]), np.uint8)
            if not np.array_equal(got, ref):
                bad.append((mode, i, n, "output from row %d" % (int(np.nonzero(got != ref)[0][0]) // 1024)))
            if crcs is not None:
                ca, cn = r.coff[i], 4 * RL.nseg(n)
                if o["crcs"][ca:ca + cn].tobytes() != crcs[i][:cn]:
                    seg = next(k for k in range(cn // 4)
                               if o["crcs"][ca + 4 * k:ca + 4 * k + 4].tobytes() != crcs[i][4 * k:4 * k + 4])
                    bad.append((mode, i, n, "CRC array from segment %d" % seg))
            status = o["report"][i][:2]
            if mode == "seal_verify_bad" and i == r.bad_blk:
                if status != (E.ECRC, r.bad_seg):
                    bad.append((mode, i, n, "report %r of the wrong stored CRC" % (status,)))
            elif status != (E.OK, -1):
                bad.append((mode, i, n, "status %r" % (status,)))
    return bad


def check(r, out, what):
    bad = block_failures(r, out)
    assert not bad, "%s: %d differences from the oracle: %s" % (what, len(bad), bad[:40])
    # (the whole arrays, padding included, and the values of the wrong-CRC report)
    RL.check_against_oracle(r, out, what)
    for mode, data in (("open_pt", r.pack(r.p)), ("seal_none", r.pack(r.c))):
        assert np.array_equal(out[mode]["data"], data), "%s %s output outside the blocks" % (what, mode)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_period_whole_tasks_match_oracle(ref_whole, path):
    check(ref_whole, Run(ref_whole, dict(PATHS)[path]).out, "whole/" + path)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_period_cut_tasks_match_oracle(ref_cut, path):
    check(ref_cut, Run(ref_cut, dict(PATHS)[path]).out, "cut/" + path)


@pytest.mark.parametrize("path", [name for name, _ in PATHS])
def test_row_period_rebuilds_tables_per_key(ref_keys, path):
    check(ref_keys, Run(ref_keys, dict(PATHS)[path]).out, "600 keys/" + path)
