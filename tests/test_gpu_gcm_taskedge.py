"""The task boundaries of the AES-GCM main kernel against the oracle.

A workgroup of gcm_main_k takes task after task from a queue.  Between two
row loops it hands the next task's index over in LDS, rebuilds the per-key
tables (the GHASH table from the key's basis, the rounds-1-2 table P), lifts
and stores the GHASH partials, and sums the raw CRC shares of segments that
two or more waves worked on (the sweep).  These tests put one task's edge
against another task's rows: a key of its own per block, tasks of one block in
sequence, tasks with and without shared segments in one workgroup's sequence,
and queues that end with no task, one task or a last task for a workgroup.

Every batch runs Seal and Open with the CRC modes none, GEN, VERIFY, GEN|CT
and VERIFY|CT (the stored CRCs of VERIFY are the oracle's, so a wrong computed
CRC fails the block), on three contexts: JFSX_CTX_CRC_LDS (JFSX_CRC_L1=0),
JFSX_CTX_CRC_L1 (JFSX_CRC_L1=1) and JFSX_CTX_BITSLICE.  Tags, outputs, CRC
arrays and statuses are compared with the oracle's, and every differing
(mode, block) is reported.  jfsx_debug_plan confirms each batch's geometry.

Batches:

  * "keys": 1,536 blocks of 64 KiB, one task each, a key of its own per
    block: six tasks per workgroup, each with another basis, P and descriptor.
  * "same block": blocks of 3 x task + 5 and 2 x task - 17 bytes for the
    plan's task size, so consecutive tasks in the queue are of one block: the
    same key, slot0 advancing, a nonzero first counter, a ragged last task.
  * "sweep": tasks of 1 MiB, 1 MiB - 31 KiB and 512 KiB, whose runs are
    sized by wave age and end inside segments (with equal runs the first and
    the last would be whole segments per wave, nothing shared), then tasks of
    96 KiB + 17, 64 KiB + 1 KiB and 33 KiB with equal runs, a 1-byte task
    that one wave holds alone, and a 0-byte block, which has no task, in one
    batch of 1 MiB tasks.  The queue is ordered by size, so a workgroup goes
    through the sizes in this order, its raw shares and flags reset from task
    to task; the checked blocks are the first of each size.  Unchecked
    filler, sealed in place, brings the batch to the size at which the plan
    picks 1 MiB tasks and the larger sizes to more tasks than workgroups.
  * "queue end": 255, 256, 257 and 513 tasks of 64 KiB.
  * "whole": behind 2 GiB of unchecked filler the plan keeps 4 MiB tasks: two
    4 MiB blocks (one whole task each: runs of 444, 316, 176 and 88 rows by
    wave age, every cut inside a segment), 4 MiB + 2 KiB + 5 (a second task of
    two rows and five bytes) and 3 x 4 MiB - 17 (three tasks of one block,
    slot0 advancing, the last one 17 bytes short: its cuts fall elsewhere).
"""
import numpy as np
import pytest

from juicefs_amd import engine as E
from tests import test_gpu_gcm_rowloop as RL

pytestmark = pytest.mark.gpu

KIB, MIB = 1 << 10, 1 << 20
PATHS = {"crc_lds": E.CTX_CRC_LDS, "crc_l1": E.CTX_CRC_L1, "bitslice": E.CTX_BITSLICE}
CRCS = {"none": E.CRC_NONE, "gen": E.CRC_GEN, "verify": E.CRC_VERIFY, "gen_ct": E.CRC_GEN | E.CRC_CT,
        "verify_ct": E.CRC_VERIFY | E.CRC_CT}
MODES = [(op, crc) for op in ("seal", "open") for crc in CRCS]


def shares_a_segment(nbytes):
    """Whether two of the 16 waves of a task of nbytes meet inside a 32 KiB segment.  The row split cuts the
    task's row pairs (2 KiB) into 16 runs, and a segment is 16 pairs: equal runs, at floor(w * pairs / 16),
    below 128 pairs; from there on runs of 111, 79, 44 and 22 1024ths of the task for waves 0-3, 4-7, 8-11 and
    12-15 (gcm_task)."""
    pairs = -(-nbytes // 2048)
    if pairs < 128:
        cuts = [w * pairs // 16 for w in range(1, 16)]
    else:
        front = [111 * i for i in range(4)] + [444 + 79 * i for i in range(4)] + [760 + 44 * i for i in range(4)] + \
                [936 + 22 * i for i in range(4)]
        cuts = [f * pairs >> 10 for f in front[1:]]
    return any(c % 16 for c in cuts)


class Run(RL.Run):
    """Seal and Open of the batch in all five CRC modes."""

    def run(self):
        r, dev = self.ref, E.MEM_DEVICE
        stale = np.full(r.cbytes, 0xEE, np.uint8)
        for op, crc in MODES:
            opening, mode = op == "open", CRCS[crc]
            stored = r.crc_c if mode & E.CRC_CT else r.crc_p
            self.src.upload(r.pack(r.c[:r.n] if opening else r.p[:r.n]))
            self.dst.upload(np.zeros(r.bytes, np.uint8))
            self.crc.upload(r.pack_crcs(stored[:r.n]) if mode & 3 == E.CRC_VERIFY else stale)
            arr, n = self.blocks(r.tag if opening else None)
            (self.eng.open_batch if opening else self.eng.seal_batch)(E.AES256GCM, arr, n, mode, dev)
            self.keep(op + "_" + crc, arr)


def failures(r, out):
    """Every (mode, block, length, what differs)."""
    bad = []
    for op, crc in MODES:
        o, mode = out[op + "_" + crc], CRCS[crc]
        datas = r.p if op == "open" else r.c
        stored = r.crc_c if mode & E.CRC_CT else r.crc_p
        for i in range(r.n):
            a, n = r.off[i], r.lens[i]
            where = (op + "_" + crc, i, n)
            if o["report"][i][:2] != (E.OK, -1):
                bad.append(where + ("status %r" % (o["report"][i][:2],),))
            if o["tags"][i] != r.tag[i]:
                bad.append(where + ("tag",))
            got, ref = o["data"][a:a + n], np.frombuffer(bytes(datas[i]), np.uint8)
            if not np.array_equal(got, ref):
                bad.append(where + ("output from row %d" % (int(np.nonzero(got != ref)[0][0]) // 1024),))
            ca, cn = r.coff[i], 4 * RL.nseg(n)
            want = bytes(stored[i])[:cn] if mode & 3 else b"\xee" * cn
            if o["crcs"][ca:ca + cn].tobytes() != want:
                bad.append(where + ("CRC array",))
    return bad


def check(r, path, what):
    out = Run(r, PATHS[path]).out
    bad = failures(r, out)
    assert not bad, "%s/%s: %d differences from the oracle: %s" % (what, path, len(bad), bad[:40])
    for op, crc in MODES:  # nothing written outside the blocks
        data = r.pack(r.p[:r.n] if op == "open" else r.c[:r.n])
        assert np.array_equal(out[op + "_" + crc]["data"], data), "%s/%s %s_%s output outside the blocks" % (
            what, path, op, crc)


@pytest.fixture(scope="module")
def ref_keys():
    r = RL.Ref(0x5261, [64 * KIB] * 1536, 0, 0)
    assert len({k for k, _ in r.keys}) == r.n, "a key of its own per block"
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    assert sorted(tasks) == [(i, 0, 64 * KIB) for i in range(r.n)], "one 64 KiB task per block, six per workgroup"
    return r


@pytest.fixture(scope="module")
def ref_same_block():
    tb = 64 * KIB
    lens = [3 * tb + 5, 2 * tb - 17] * 100
    r = RL.Ref(0x5262, lens, 0, 0)
    tb2, _, tasks = E.debug_plan(E.PLAN_GCM, lens)
    assert tb2 == tb, "the plan's task size"
    assert len(tasks) == 100 * (4 + 2), "four and two tasks per block: more than twice the compute units"
    order = {t: k for k, t in enumerate(tasks)}
    for b in (0, 1, 198):
        ks = [order[(b, c0, min(c0 + tb, lens[b]))] for c0 in range(0, lens[b] - tb, tb)]
        assert ks == list(range(ks[0], ks[0] + len(ks))), "the whole tasks of block %d follow each other" % b
    return r


SWEEP_SIZES = [(MIB, 16, 100), (MIB - 31 * KIB, 16, 240), (512 * KIB, 16, 240), (96 * KIB + 17, 16, 0),
               (64 * KIB + KIB, 16, 0), (33 * KIB, 16, 0), (1, 4, 0), (0, 4, 0)]  # (length, checked, filler)


@pytest.fixture(scope="module")
def ref_sweep():
    lens = [n for n, k, _ in SWEEP_SIZES for _ in range(k)]
    fill = [n for n, _, k in SWEEP_SIZES for _ in range(k)]
    r = RL.Ref(0x5263, lens, 0, 0, fill=fill)
    tb, _, tasks = E.debug_plan(E.PLAN_GCM, lens + fill)
    assert tb == MIB, "the plan picks 1 MiB tasks"
    assert [c1 - c0 for _, c0, c1 in tasks] == sorted((n for n in lens + fill if n), reverse=True), \
        "one task per block, by size"
    assert [shares_a_segment(n) for n, _, _ in SWEEP_SIZES[:7]] == [True, True, True, True, True, True, False]
    assert [-(-n // 2048) >= 128 for n, _, _ in SWEEP_SIZES[:7]] == [True, True, True, False, False, False, False], \
        "runs by wave age in the first three sizes, equal runs in the others"
    for n, _, _ in SWEEP_SIZES[:3]:  # each more tasks than workgroups, the checked blocks first
        mine = [b for b, c0, c1 in tasks if c1 - c0 == n]
        assert len(mine) >= 256 or n == MIB
        assert mine[:16] == [i for i, x in enumerate(lens) if x == n]
    return r


@pytest.fixture(scope="module")
def refs_queue():
    return {n: RL.Ref(0x5264, [64 * KIB] * n, 0, 0) for n in (255, 256, 257, 513)}


WHOLE = [4 * MIB, 4 * MIB + 2 * KIB + 5, 3 * 4 * MIB - 17, 4 * MIB]


@pytest.fixture(scope="module")
def ref_whole():
    r = RL.Ref(0x5265, WHOLE, 0, 0, fill=[8 * MIB] * 255)
    tb, _, tasks = E.debug_plan(E.PLAN_GCM, r.lens + r.fill)
    assert tb == 4 * MIB, "the plan keeps 4 MiB tasks"
    mine = sorted(t for t in tasks if t[0] < len(WHOLE))
    assert mine == [(0, 0, 4 * MIB), (1, 0, 4 * MIB), (1, 4 * MIB, WHOLE[1]), (2, 0, 4 * MIB),
                    (2, 4 * MIB, 8 * MIB), (2, 8 * MIB, WHOLE[2]), (3, 0, 4 * MIB)], \
        "whole 4 MiB tasks, blocks of two and three tasks, ragged last tasks"
    return r


@pytest.mark.parametrize("path", list(PATHS))
def test_back_to_back_tasks_with_different_keys(ref_keys, path):
    check(ref_keys, path, "1536 keys")


@pytest.mark.parametrize("path", list(PATHS))
def test_consecutive_tasks_of_one_block(ref_same_block, path):
    check(ref_same_block, path, "same block")


@pytest.mark.parametrize("path", list(PATHS))
def test_shared_segment_sweep_on_and_off_in_one_batch(ref_sweep, path):
    check(ref_sweep, path, "sweep")


@pytest.mark.parametrize("path", list(PATHS))
def test_whole_4mib_tasks_with_runs_by_wave_age(ref_whole, path):
    check(ref_whole, path, "whole 4 MiB tasks")


@pytest.mark.parametrize("ntasks", [255, 256, 257, 513])
@pytest.mark.parametrize("path", list(PATHS))
def test_queue_end(refs_queue, path, ntasks):
    r = refs_queue[ntasks]
    tasks = E.debug_plan(E.PLAN_GCM, r.lens)[2]
    assert sorted(tasks) == [(i, 0, 64 * KIB) for i in range(ntasks)], "one 64 KiB task per block"
    check(r, path, "%d tasks" % ntasks)
