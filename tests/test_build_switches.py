"""Every build or run-time switch under juicefs_amd/csrc is on the list below.

The names that appear in a #if / #ifdef / #ifndef / #elif line or in a
getenv("JFSX_...") there must equal SWITCHES exactly.  An experiment adds its
switch here, in the open, with who selects it; once the experiment is decided
the losing side is deleted and the entry goes with it ("Build
switches")."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SWITCHES = {
    # --- instrumentation builds (results stay correct)
    "JFSX_ABLATE_TRACE": "scripts/wgtrace.py, the Makefile's variant target: per-workgroup time stamps",
    "JFSX_KS_PHASES": "tools/ks_phase_probe.py: phase stamps of keysetup and the main kernel",
    "JFSX_LZ4_STAMP": "scripts/lz4_stamps.py: section stamps of the LZ4 kernels",
    "JFSX_ZSTD_STAMP": "scripts/zstd_stamps.py: section stamps of the zstd decoder",
    "JFSX_ZC_STAMP": "instrumentation build (scripts/GPU_CALLS_r1-r4.md): parse / entropy stamps of the zstd compressor",
    # --- kernel variants a test or the API selects
    "JFSX_CRC_L1": "juicefs_amd/engine.py and the crc_l1 tests: a context's fused-CRC path (LDS or vector L1)",
    "JFSX_CRC_L1K": "round 7: lookups per CRC step through the L1 (DESIGN 4.1)",
    "JFSX_CRC_L1LG": "round 7: gathers per AES round group",
    "JFSX_CRC_L1LAG": "round 7: round groups between a gather's issue and its fold",
    "JFSX_CRC_L1_DEFAULT": "round 7: whether a context takes the L1 path unless told otherwise",
    "JFSX_LZ4_TABLE": "tests/test_gpu_lz4.py, bench.py: the LZ4 hash table in LDS or global memory",
    "JFSX_RSA_PAIR": "tests/test_gpu_rsa_fixed.py: lane-pair or single-lane exponentiation",
    "JFSX_ZSTD_SERIAL": "bench.py, scripts/zstd_stamps.py: the serial zstd decoder, also the fallback",
    # --- variants kept because no measured verdict is on record ("Build switches")
    "JFSX_GH8": "GHASH table walk in quarters / halves / at once: verdict only in a source comment",
    "JFSX_ABLATE_GHBUILD": "timing ablation (wrong tags): no numbers recorded",
    "JFSX_ABLATE_LIFT": "timing ablation (wrong tags): no numbers recorded",
    "JFSX_ABLATE_NEAR": "LZ4 decoder timing ablation (wrong output): no numbers recorded",
    "JFSX_LZ4_FLUSH": "LZ4 decoder flush threshold: no A/B recorded",
    "JFSX_SBOX_PAIR": "bitsliced S-boxes in pairs or singly: no A/B recorded",
    "JFSX_ZC_LANE0_ENTROPY": "zstd compressor's entropy stage on lane 0: no A/B recorded",
    "JFSX_ZC_SCALAR": "zstd compressor on one lane (the library's serial code): no A/B recorded",
    # --- host-side run-time knobs (jfsx_api.cpp, jfsx_agg.cpp)
    "JFSX_AGG_ARENA_MB": "aggregator: staging arena size",
    "JFSX_AGG_DISPATCHERS": "aggregator: dispatcher threads",
    "JFSX_AGG_FILL_MB": "aggregator: batch fill target",
    "JFSX_AGG_INFLIGHT": "aggregator: batches in flight",
    "JFSX_MCTX_WORKERS": "multi-device context: worker threads",
    "JFSX_BOUNCE_RETAIN_MB": "host pipeline: bounce buffer kept between calls",
    "JFSX_COPY_THREADS": "host pipeline: staging copy threads",
    "JFSX_HOST_STAGE": "host pipeline: staging policy",
    "JFSX_KS_STREAM": "host pipeline: keysetup on its own stream",
    "JFSX_PIPE": "host pipeline: staging slots (compile time)",
    "JFSX_PIPE_META": "host pipeline: descriptors pulled by a kernel",
    "JFSX_PIPE_STATS": "host pipeline: statistics at context destruction",
    "JFSX_WAIT_POLL_US": "host pipeline: poll interval of waits",
    "JFSX_ZC_QUEUE": "zstd compressor: ticket-queue object assignment",
    "JFSX_ZC_WAVES": "zstd compressor: persistent waves per CU",
    "JFSX_ZSTD_ARENA_MB": "zstd decoder: arena budget",
    # --- host / device portability guards and macro hooks the host builds override
    "__HIPCC__": "headers shared with the host harness",
    "__HIP_DEVICE_COMPILE__": "device-only intrinsics in shared headers",
    "__gfx950__": "gfx950-only instructions in jfsx_md5.h",
    "__has_builtin": "jfsx_gf.h: bit reverse builtin or a portable loop",
    "__builtin_bitreverse32": "the builtin __has_builtin asks for",
    "JFSX_HD": "jfsx_load.h: function qualifiers (tests/harness overrides)",
    "JFSX_GF_HD": "jfsx_gf.h: function qualifiers",
    "JFSX_GF_BREAK": "jfsx_gf.h: scheduling fence hook",
    "JFSX_MD5_HD": "jfsx_md5.h: function qualifiers",
    "JFSX_P5_HD": "jfsx_poly.h: function qualifiers",
    "JFSX_RSA_OPAQUE": "jfsx_rsa.h: value barrier hook",
    "JFSX_RSA_TRACE": "jfsx_rsa.h: operation trace hook of tests/harness/rsa_host.cpp",
}

_COND = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$")


def _names_in_tree():
    found = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "juicefs_amd", "csrc", "*"))):
        base = os.path.basename(path)
        for line in open(path, encoding="utf-8"):
            m = _COND.match(line)
            if m:
                expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(1))
                for name in re.findall(r"[A-Za-z_]\w*", expr):
                    if name != "defined":
                        found.setdefault(name, set()).add(base)
            for name in re.findall(r'getenv\("(JFSX_\w+)"\)', line):
                found.setdefault(name, set()).add(base)
    return found


def test_switches_are_exactly_the_listed_ones():
    found = _names_in_tree()
    unlisted = {n: sorted(f) for n, f in found.items() if n not in SWITCHES}
    stale = sorted(set(SWITCHES) - set(found))
    assert not unlisted, "switches not on the list (add them with a reason, or delete them): %r" % unlisted
    assert not stale, "listed switches the source no longer has (remove them): %r" % stale


def test_every_entry_has_a_reason():
    assert all(isinstance(r, str) and len(r) > 10 for r in SWITCHES.values())
