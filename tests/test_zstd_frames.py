"""The gate of tests/zstd_frames.py, on the CPU: every built frame decodes
under the system zstd library and under the host build of the serial decoder
(juicefs_amd/csrc/jfsx_zstd.h) to the model's bytes, every reject is rejected
by both, the census of the corpus has every cell the block-parallel decoder's
execution phase (jfsx_zstd2.h) is to be pinned on, and the census's constants
are the kernel's.  tests/test_gpu_zstd_exec.py sends the same frames to the GPU."""
import os
import re

import pytest

from tests import zstd_frames as Z, zstd_lib
from tests.test_zstd_host import host  # noqa: F401  (the fixture: the host build of jfsx_zstd.h)

HDR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "juicefs_amd", "csrc", "jfsx_zstd2.h")


def test_constants_are_the_kernels():
    src = open(HDR).read()
    for name in ("kWinBytes", "kWinMax", "kRing", "kLitStage", "kMaxBlk"):
        m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % name, src)
        assert m, name
        assert int(m.group(1)) == getattr(Z, name), name


def test_corpus_limits():
    cs = Z.corpus()
    assert len({c.name for c in cs}) == len(cs)
    assert max(len(c.out) for c in cs) <= 1 << 20
    assert sum(len(c.out) for c in cs) <= 64 << 20
    assert [c.name for c in cs if c.serial] == ["blocks_65"]
    assert any(c.name == Z.ALIGN_CASE and len(c.out) > 2 * Z.kRing for c in cs)


def test_library_decodes_every_frame_to_the_models_bytes():
    for c in Z.corpus():
        assert zstd_lib.decompress(c.frame, len(c.out)) == (len(c.out), c.out), c.name


def test_host_decoder_decodes_every_frame_to_the_models_bytes(host):  # noqa: F811
    for c in Z.corpus():
        assert host(c.frame, len(c.out)) == (len(c.out), c.out), c.name


def test_rejects_are_rejected_by_library_and_host_decoder(host):  # noqa: F811
    names = [n for n, _, _ in Z.rejects()]
    assert len(names) == 11 and len(set(names)) == 11
    for name, fr, cap in Z.rejects():
        assert zstd_lib.decompress(fr, cap)[0] < 0, name
        assert host(fr, cap)[0] < 0, name
    # the dst_cap rejects are corpus frames one byte short: accepted at dst_cap = n
    by = {c.frame: c for c in Z.corpus()}
    assert sum(1 for _, fr, cap in Z.rejects() if fr in by and cap == len(by[fr].out) - 1) == 5


def test_census_is_complete():
    """Every cell of REQUIRED is reached by some corpus frame (a condition on
    the inputs, from the model alone)."""
    got = set()
    for c in Z.corpus():
        got |= Z.census(c.trace)
    assert not got - set(Z.REQUIRED), sorted(got - set(Z.REQUIRED))
    assert [x for x in Z.REQUIRED if x not in got] == []


def test_model_rejects_what_it_should():
    with pytest.raises(Z.Invalid):
        Z.decode([Z.cmp_(b"abcdef", [(4, 8, 5 + 3)])])
    with pytest.raises(Z.Invalid):
        Z.decode([Z.raw(b"0123456789"), Z.cmp_(b"lit", [(4, 4, 5 + 3)])])


def test_census_notices_a_wrong_dependency_mask(monkeypatch):
    """The census restates the kernel's mask and checks it against the lanes
    a match really reads: with the mask's first lane dropped, the frames built
    for the mask's edges must trip it."""
    real = Z._kernel_mask
    monkeypatch.setattr(Z, "_kernel_mask", lambda *a: {i for i in real(*a) if i != min(real(*a))})
    tripped = 0
    for c in Z.corpus():
        if c.name.startswith("mask_"):
            try:
                Z.census(c.trace)
            except AssertionError:
                tripped += 1
    assert tripped >= 4
