"""The crafted ChaCha20-Poly1305 ciphertexts that tests/test_poly1305.py (CPU:
the host emulation and the oracle) and tests/test_gpu_poly_edges.py (the
kernels) share.  Crafted once per process; fixed seeds, so every run sees the
same bytes.  What a case was built for (`want`) is checked on the CPU against
the emulation of the kernels' own functions, so a GPU case is never vacuous."""
import functools
import hashlib

from juicefs_amd import engine as E
from tests import poly_model as M

P = M.P
KIB = 1 << 10
# one full row (p_mul_add only); the guarded tail row with a partial block; the r^253 hop
SHAPES = [4096, 4096 + 40, 8192]
SPLIT = "split"  # stands for split_length() in a spec


def tasks_of(n):
    """The planner's tasks (c0, c1) of a single block of n bytes."""
    return sorted((c0, c1) for _, c0, c1 in E.debug_plan(E.PLAN_CHACHA, [n])[2])


def split_length():
    """The smallest block the planner cuts into two tasks."""
    return E.debug_plan(E.PLAN_CHACHA, [1])[0] + 1


class Case:
    def __init__(self, name, n, build, want):
        self.name, self.want = name, want
        self.n = n = split_length() if n == SPLIT else n
        self.key = hashlib.sha256(("poly-edge/" + name).encode()).digest()
        self.nonce = hashlib.sha256(("poly-edge-nonce/" + name).encode()).digest()[:12]
        self.c = build(self)
        assert len(self.c) == n
        self.tag = M.tag(self.key, self.nonce, self.c)


FINAL_TARGETS = [
    ("0", 0), ("1", 1), ("4", 4), ("p-1", P - 1), ("p-5", P - 5), ("2^128-1", (1 << 128) - 1), ("2^128", 1 << 128),
    ("-s", lambda s: (-s) & M.M128),            # tag all zero: h + s carries out of every word
    ("-1-s", lambda s: (M.M128 - s) & M.M128),  # tag all ones: no word carries
]
# lane targets: (lane, value); None leaves the lane seeded, ("p-", l) is p minus lane l's value.  Two lanes are the
# partners l, l ^ 32 of the wave sum's first step.
LANE_TARGETS = [("lane=0", [(5, 0)]), ("lane=p-1", [(63, P - 1)]), ("pair=p", [(9, None), (41, ("p-", 9))]),
                ("pair=2p-2", [(0, P - 1), (32, P - 1)])]


def _lanes(cs, lanes):
    (task,) = tasks_of(cs.n)
    assert M.wave_range(task[0], task[1], 3) == (0, cs.n)  # a one-segment task is wave 3's
    return M.craft_lanes(cs.key, cs.nonce, cs.n, task, 3, lanes, cs.name)


def _wave(cs, t, wave):
    ts = tasks_of(cs.n)
    if cs.n == 128 * KIB:  # one segment per wave
        assert len(ts) == 1 and M.wave_range(ts[0][0], ts[0][1], wave) == (wave * M.SEG, (wave + 1) * M.SEG)
    else:
        assert len(ts) == 2 and len(tasks_of(cs.n - 1)) == 1
    return M.craft_wave(cs.key, cs.nonce, cs.n, ts[t], wave, 0, cs.name)


def _specs():
    """(name, length, builder, what it is built for); needs no library"""
    out = []
    # -- the final accumulator
    for n in SHAPES:
        for tname, t in FINAL_TARGETS:
            out.append(("final[%s]-%d" % (tname, n), n,
                        lambda cs, t=t: M.craft_final(cs.key, cs.nonce, cs.n, t, cs.name), ("final", t)))
    # -- one lane's lifted partial, and two lanes the wave sum pairs in its first step
    for n in (4096, 8192):
        for tname, lanes in LANE_TARGETS:
            out.append(("%s-%d" % (tname, n), n, lambda cs, lanes=lanes: _lanes(cs, lanes), ("lanes", 0, 3, lanes)))
    # -- a whole wave's sum = 0: the zero-partial skip of finalize, on a wave that is not empty
    for wave in range(4):
        out.append(("wave%d=0-%d" % (wave, 128 * KIB), 128 * KIB, lambda cs, wave=wave: _wave(cs, 0, wave),
                    ("wave", 0, wave)))
    out.append(("wave1=0-split", SPLIT, lambda cs: _wave(cs, 0, 1), ("wave", 0, 1)))
    # -- saturated data: the largest and the smallest message limbs
    for n in (16, 64, 4096, 4112, 32768, 131072):
        for byte in (0xFF, 0x00):
            out.append(("all%02x-%d" % (byte, n), n, lambda cs, byte=byte: bytes([byte]) * cs.n, ("none",)))
    return out


SPECS = {s[0]: s for s in _specs()}
NAMES = list(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(*SPECS[name])


def cases():
    return [case(n) for n in NAMES]
