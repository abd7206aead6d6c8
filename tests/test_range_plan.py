"""CPU pin of the ranged Open's contract: jfsx_rblk's layout, the window rule
and the task plan of jfsx_open_range_batch through engine.debug_range_plan, and
the argument errors the call rejects before it touches a context."""
import ctypes
import itertools

import numpy as np
import pytest

from juicefs_amd import engine as E

SEG = E.SEG
KINDS = [E.PLAN_GCM, E.PLAN_CHACHA]
NAME = {E.PLAN_GCM: "gcm", E.PLAN_CHACHA: "chacha"}
LENS = [0, 1, 16, 32768, 32769]
CT = E.CRC_GEN | E.CRC_CT


def window(length, off, limit):
    """encrypt.go:246-253"""
    o = min(off, length)
    n = length - o if limit == -1 or limit > length - o else limit
    return o, n


def cases(length):
    offs = [0, 1, length - 1, length, length + 1, 1 << 63]
    limits = [-1, 0, 1, length, length + 1, 1 << 62]
    return [(length, o, l) for o, l in itertools.product(offs, limits) if o >= 0]


def check_plan(kind, lens, offs, limits):
    pl = E.debug_range_plan(kind, lens, offs, limits)
    assert len(pl["blocks"]) == len(lens)
    slot = 0
    tasks = iter(pl["tasks"])
    seen = 0
    for i, (n_, off, limit) in enumerate(zip(lens, offs, limits)):
        b = pl["blocks"][i]
        o, n = window(n_, off, limit)
        assert (b["o"], b["n"]) == (o, n), (n_, off, limit)
        # the widened window: whole segments (but for the block's tail), around [o, o + n), empty with n = 0
        w0, w1 = b["w0"], b["w1"]
        if n == 0:
            assert w0 == w1
        else:
            assert w0 % SEG == 0 and (w1 % SEG == 0 or w1 == n_)
            assert w0 <= o < w0 + SEG and o + n <= w1 < o + n + SEG and w1 <= n_
        # the block's tasks, in plan order: its main tasks, then its auth tasks
        mine = [next(tasks) for _ in range(b["n_main"] + b["n_auth"])]
        seen += len(mine)
        assert all(t[0] == i for t in mine)
        assert [t[1] for t in mine] == [0] * b["n_main"] + [1] * b["n_auth"]
        # slots: contiguous over the block, the block's first slot first
        assert b["slot0"] == slot
        for t in mine:
            assert t[4] == slot
            slot += pl["main_slots"] if t[1] == 0 else pl["auth_slots"]
        assert b["nslots"] == slot - b["slot0"]
        # main and auth tasks partition the block's segments exactly once
        cover = sorted((t[2], t[3], t[1]) for t in mine)
        at = 0
        for c0, c1, kern in cover:
            assert c0 == at and c0 < c1 and c0 % SEG == 0
            assert (w0 <= c0 and c1 <= w1) if kern == 0 else (c1 <= w0 or c0 >= w1)
            assert c1 - c0 <= (pl["main_bytes"] if kern == 0 else pl["auth_bytes"])
            at = c1
        assert at == n_
    assert seen == len(pl["tasks"])
    return pl


@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_window_rule_and_plan(kind):
    every = []
    for length in LENS:
        cs = cases(length)
        every += cs
        for c in cs:  # alone
            check_plan(kind, [c[0]], [c[1]], [c[2]])
        check_plan(kind, *zip(*cs))  # and as one batch
    check_plan(kind, *zip(*every))
    assert E.debug_range_plan(kind, [], [], [])["tasks"] == []


@pytest.mark.parametrize("kind", KINDS, ids=NAME.get)
def test_plan_of_larger_blocks(kind):
    big = 4 << 20
    lens = [big, big - 5, 384 * 1024 + 1000, big]
    pl = check_plan(kind, lens, [(1 << 20) + 5, 0, 65531, big - 1], [4096, -1, 32778, 1])
    b = pl["blocks"]
    assert (b[0]["w0"], b[0]["w1"]) == (1 << 20, (1 << 20) + SEG)
    assert b[1]["n_auth"] == 0 and b[1]["n_main"] >= 1
    assert (b[2]["w0"], b[2]["w1"]) == (32768, 131072)
    assert (b[3]["w0"], b[3]["w1"]) == (big - SEG, big)
    # the auth planner's ladder: a power of two of segments between the kernel's minimum and 1 MiB
    lo = 65536 if kind == E.PLAN_GCM else 32768
    assert pl["auth_bytes"] in [lo << k for k in range(6)] and pl["auth_bytes"] <= 1 << 20
    with pytest.raises(E.EngineError):
        E.debug_range_plan(kind, [10], [0], [-2])


def test_rblk_layout_and_exports():
    assert ctypes.sizeof(E.jfsx_rblk) == 136
    f = E.jfsx_rblk
    assert (f.tag.offset, f.src.offset, f.len.offset, f.off.offset, f.limit.offset, f.dst.offset, f.dst_cap.offset,
            f.crc.offset, f.out_len.offset, f.status.offset, f.reserved2.offset) == \
        (48, 64, 72, 80, 88, 96, 104, 112, 120, 128, 132)
    L = E.load_library()
    for name in ("jfsx_open_range_batch", "jfsx_agg_open_range", "jfsx_data_decrypt_range"):
        assert name in E.EXPORTS and getattr(L, name)
    assert L.jfsx_abi_version() == 9
    assert ctypes.sizeof(E.jfsx_metrics) == 28 * 8


def test_argument_errors_touch_no_context():
    """Every argument error of the table, with a context that is not one (it
    would fault if it were used): JFSX_EINVAL, the record and the buffers
    unchanged."""
    L = E.load_library()
    src = np.full(256, 0x5A, np.uint8)
    dst = np.full(256, 0xA5, np.uint8)
    crc = np.full(48, 0xA5, np.uint8)
    fake = ctypes.c_void_p(16)
    sp = src.ctypes.data + (-src.ctypes.data) % 16  # 16-byte aligned, for the device rules
    dp = dst.ctypes.data + (-dst.ctypes.data) % 16
    cp = crc.ctypes.data + (-crc.ctypes.data) % 16

    def blk(**kw):
        spec = {"key": bytes(32), "nonce": bytes(12), "tag": bytes(16), "src": sp, "len": 100, "off": 10, "limit": 20,
                "dst": dp, "dst_cap": 20, "crc": cp}
        spec.update(kw)
        arr, _ = E.Engine.make_rblocks([spec])
        arr[0].status, arr[0].out_len = 77, 78
        return arr

    def rejected(arr, algo=E.AES256GCM, mode=E.CRC_NONE, mem=E.MEM_HOST, n=1, ctx=fake):
        rc = L.jfsx_open_range_batch(ctx, algo, n, arr, mode, mem)
        return rc == E.EINVAL and (arr is None or (arr[0].status, arr[0].out_len) == (77, 78)) and \
            (src == 0x5A).all() and (dst == 0xA5).all() and (crc == 0xA5).all()

    assert rejected(blk(), ctx=None)
    assert rejected(None)
    assert rejected(blk(), n=-1)
    for algo in (2, -1):
        assert rejected(blk(), algo=algo)
    for mode in (E.CRC_GEN, E.CRC_VERIFY, E.CRC_CT, E.CRC_VERIFY | E.CRC_CT, E.CRC_GEN | E.CRC_BOTH, 16, -1):
        assert rejected(blk(), mode=mode), mode
    for mem in (2, -1):
        assert rejected(blk(), mem=mem)
    r = blk()
    r[0].reserved = 1
    assert rejected(r)
    r = blk()
    r[0].reserved2 = 1
    assert rejected(r)
    assert rejected(blk(limit=-2))
    assert rejected(blk(len=((1 << 32) - 2) * 16 + 1), algo=E.AES256GCM)
    assert rejected(blk(len=((1 << 32) - 1) * 16 + 1), algo=E.CHACHA20P1305)
    assert rejected(blk(dst_cap=19))
    assert rejected(blk(limit=-1, dst_cap=89))        # n = len - o = 90
    assert rejected(blk(dst=None))
    assert rejected(blk(crc=None), mode=CT)
    assert rejected(blk(src=None))
    for mem in (E.MEM_HOST, E.MEM_DEVICE):
        assert rejected(blk(dst=None, dst_cap=0), mem=mem)  # n = 20 still needs a dst
    # device memory: alignment of what is used, and dst against src
    D = E.MEM_DEVICE
    assert rejected(blk(src=sp + 1), mem=D)
    assert rejected(blk(dst=dp + 8), mem=D)
    assert rejected(blk(crc=cp + 4), mode=CT, mem=D)
    assert rejected(blk(dst=sp + 96, dst_cap=32), mem=D)      # dst[0, dst_cap) reaches into src[0, len)
    assert rejected(blk(dst=sp - 16, dst_cap=32, src=sp), mem=D)
    # legal: no blocks at all (nothing runs, the context is not touched)
    assert L.jfsx_open_range_batch(fake, E.AES256GCM, 0, None, E.CRC_NONE, E.MEM_HOST) == 0
    assert L.jfsx_open_range_batch(fake, E.CHACHA20P1305, 0, blk(), CT, E.MEM_DEVICE) == 0
    # jfsx_data_decrypt_range: its own argument errors, before the context is touched
    obj = np.zeros(3 + 12 + 16 + 5, np.uint8)
    obj[2] = 12
    out = np.full(8, 0xA5, np.uint8)
    n = ctypes.c_uint64(99)
    dr = L.jfsx_data_decrypt_range
    assert dr(None, E.AES256GCM, bytes(32), obj.ctypes.data, obj.size, 0, -1, out.ctypes.data, 8, ctypes.byref(n),
              None, None) == E.EINVAL
    assert dr(fake, 7, bytes(32), obj.ctypes.data, obj.size, 0, -1, out.ctypes.data, 8, ctypes.byref(n), None,
              None) == E.EINVAL
    assert dr(fake, E.AES256GCM, bytes(32), obj.ctypes.data, obj.size, 0, -2, out.ctypes.data, 8, ctypes.byref(n),
              None, None) == E.EINVAL
    assert dr(fake, E.AES256GCM, bytes(32), obj.ctypes.data, obj.size, 1, -1, out.ctypes.data, 3, ctypes.byref(n),
              None, None) == E.EINVAL  # out_cap one byte short of n = 4
    bad = obj.copy()
    bad[0] = 0xFF
    assert dr(fake, E.AES256GCM, bytes(32), bad.ctypes.data, bad.size, 0, -1, out.ctypes.data, 8, ctypes.byref(n),
              None, None) == E.EMISFORMED
    assert n.value == 99 and (out == 0xA5).all()
