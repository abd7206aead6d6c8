"""The task planner (plan_batch, jfsx_api.cpp) through its host-only view
engine.debug_plan: what the AEAD and CRC kernels assume of the tasks they are
given, over seeded random and edge length lists.  No device.

The invariants are the ones the sources state, not observed output:
  Task.c0 % kSeg == 0                                (jfsx_internal.h, struct Task)
  each block is split into tasks of at most task_bytes, whole segments, one
  workgroup each; `slots` partial slots per task     (plan_tasks)
  GCM: 64 KiB (kGcmMinTask) .. 4 MiB (kMaxTaskBytes) in 64 KiB steps, 16 slots
  ChaCha: one segment per wave (4 x 32 KiB) .. 1 MiB (kCpTaskBytes), 4 slots
  CRC: whole 16-segment rounds up to 4 MiB (crc_task_bytes), no slots
  small batches are cut into about 512 (GCM, CRC: ~2 per CU) or 2048 (ChaCha)
  tasks, large ones keep the largest task
  the persistent transform kernels get the tasks largest first in 4 KiB
  units, stable within a unit (order_largest_first); crc_segments_k is one
  workgroup per task and gets them in plan order
"""
import numpy as np
import pytest

from juicefs_amd import engine as E

KIB, MIB, GIB = 1 << 10, 1 << 20, 1 << 30
SEG = 32 * KIB
# kind: (unit, largest task, slots per task, tasks wanted of a small batch, largest-first dispatch)
KINDS = {
    E.PLAN_GCM: (64 * KIB, 4 * MIB, 16, 512, True),
    E.PLAN_CHACHA: (128 * KIB, 1 * MIB, 4, 2048, True),
    E.PLAN_CRC: (512 * KIB, 4 * MIB, 0, 512, False),
}
IDS = {E.PLAN_GCM: "gcm", E.PLAN_CHACHA: "chacha", E.PLAN_CRC: "crc"}


def check_plan(kind, lens):
    unit, top, slots, want, sorted_ = KINDS[kind]
    lens = [int(x) for x in lens]
    total = sum(lens)
    tb, nslots, tasks = E.debug_plan(kind, lens)
    ctx = (IDS[kind], total, lens[:6])
    # the task size: whole units within [unit, top], about total / want
    assert tb % unit == 0 and unit <= tb <= top, ctx
    assert tb == top or tb * want >= total - want, ctx        # not finer than `want` tasks need
    assert tb == unit or (tb - unit) * want < total, ctx      # and not a whole unit coarser
    assert nslots == len(tasks) * slots, ctx
    # per block: the tasks tile [0, len) with full tasks and one last, possibly short
    per_blk = {}
    for blk, c0, c1 in tasks:
        assert 0 <= blk < len(lens), ctx
        assert c0 % SEG == 0 and c0 < c1, ctx + (blk, c0, c1)
        per_blk.setdefault(blk, []).append((c0, c1))
    plan = []  # the plan order, rebuilt
    for b, n in enumerate(lens):
        ts = sorted(per_blk.get(b, []))
        if n == 0:
            assert not ts, ctx + (b,)
            continue
        assert ts[0][0] == 0 and ts[-1][1] == n, ctx + (b,)
        for (a0, a1), (b0, _) in zip(ts, ts[1:]):
            assert a1 == b0 and a1 - a0 == tb, ctx + (b, a0, a1, b0)
        assert ts[-1][1] - ts[-1][0] <= tb, ctx + (b,)
        assert len(ts) == -(-n // tb), ctx + (b,)
        plan += [(b, c0, c1) for c0, c1 in ts]
    # dispatch order: a permutation of the plan ...
    assert sorted(tasks) == plan, ctx
    if sorted_:
        # ... largest first in 4 KiB units, plan order kept within a unit
        units = [(c1 - c0) >> 12 for _, c0, c1 in tasks]
        assert all(a >= b for a, b in zip(units, units[1:])), ctx
        assert tasks == sorted(plan, key=lambda t: -((t[2] - t[1]) >> 12)), ctx
    else:
        assert tasks == plan, ctx
    return tb


def _steps(kind):
    """Totals around every point where the task size may step up: one unit more
    per want * unit bytes, up to the largest task."""
    unit, top, _, want, _ = KINDS[kind]
    out = []
    for k in range(1, top // unit + 2):
        edge = k * unit * want
        out += [edge - want - 1, edge - want, edge - 1, edge, edge + 1, edge + want - 1, edge + want, edge + want + 1]
    return out


@pytest.mark.parametrize("kind", sorted(KINDS), ids=lambda k: IDS[k])
def test_edge_batches(kind):
    for lens in ([], [0], [0, 0, 0], [1], [0, 1, 0], [SEG - 1], [SEG], [SEG + 1], [0, 5, 0, SEG + 7, 0]):
        tb = check_plan(kind, lens)
        assert tb == KINDS[kind][0]  # the smallest task for the smallest batches
    # the empty batch and the all-empty batch have no task at all
    assert E.debug_plan(kind, [])[1:] == (0, [])
    assert E.debug_plan(kind, [0, 0])[1:] == (0, [])


@pytest.mark.parametrize("kind", sorted(KINDS), ids=lambda k: IDS[k])
def test_totals_around_every_rounding_step(kind):
    unit, top, _, want, _ = KINDS[kind]
    seen = set()
    prev = 0
    for total in _steps(kind):
        # as one block, and as ragged blocks of the same total
        tb = check_plan(kind, [total])
        third = total // 3
        assert check_plan(kind, [third + 5, 0, total - 2 * third - 12, third + 7]) == tb
        assert tb >= prev  # a larger batch never gets smaller tasks
        prev = tb
        seen.add(tb)
    # the sweep went through every task size there is
    assert seen == set(range(unit, top + 1, unit))


@pytest.mark.parametrize("kind", sorted(KINDS), ids=lambda k: IDS[k])
def test_totals_from_2_gib(kind):
    top = KINDS[kind][1]
    for lens in ([2 * GIB - 1], [2 * GIB], [2 * GIB + 1], [4 * GIB - 1, 1, 1], [4 * GIB + SEG + 1],
                 [3 * GIB + 5, 0, 5 * GIB + 7, 13], [GIB] * 64, [GIB + 12345] * 3 + [17] * 50):
        assert check_plan(kind, lens) == top


# the longest block each cipher's kernels take (jfsx.h, struct jfsx_blk): GCM's 32-bit counter runs from 2;
# the ChaCha kernels count a block's 16-byte Poly1305 blocks in 32 bits
MAX_LEN = {E.PLAN_GCM: ((1 << 32) - 2) * 16, E.PLAN_CHACHA: ((1 << 32) - 1) * 16}


@pytest.mark.parametrize("kind", sorted(MAX_LEN), ids=lambda k: IDS[k])
def test_length_limit_and_one_past_it(kind):
    """The plan applies the batch validation's per-cipher limits: the longest
    block plans (its last task's exponents fit the kernels' 32 bits), one byte
    more is JFSX_EINVAL wherever it stands in the batch.  No buffer exists."""
    top, limit = KINDS[kind][1], MAX_LEN[kind]
    assert check_plan(kind, [limit]) == top
    tasks = E.debug_plan(kind, [limit])[2]
    assert max(c1 for _, _, c1 in tasks) == limit and -(-limit // 16) < 1 << 32
    assert check_plan(kind, [5, limit, 0]) == top
    for lens in ([limit + 1], [1, limit + 1], [limit + 1, 0], [limit + 16], [1 << 38], [(1 << 64) - 1]):
        with pytest.raises(E.EngineError) as ei:
            E.debug_plan(kind, lens)
        assert ei.value.code == E.EINVAL, lens
    # the CRC-only plan has no cipher's limit
    assert E.debug_plan(E.PLAN_CRC, [limit + 1])[0] == KINDS[E.PLAN_CRC][1]


@pytest.mark.parametrize("kind", sorted(KINDS), ids=lambda k: IDS[k])
def test_seeded_random_batches(kind):
    rng = np.random.default_rng(20261019 + kind)
    sizes = set()
    for case in range(250):
        n = int(rng.integers(0, 40))
        scale = int(rng.choice([1, 100, SEG, MIB, 8 * MIB, 64 * MIB, 300 * MIB]))
        lens = rng.integers(0, 2 * scale + 1, n)
        # sprinkle empty blocks, whole segments and whole tasks among them
        for i in range(n):
            r = int(rng.integers(0, 8))
            if r == 0:
                lens[i] = 0
            elif r == 1:
                lens[i] = int(lens[i]) // SEG * SEG
            elif r == 2:
                lens[i] = int(lens[i]) // MIB * MIB
        sizes.add(check_plan(kind, lens))
    unit, top = KINDS[kind][:2]
    assert unit in sizes and top in sizes and len(sizes) > 3
