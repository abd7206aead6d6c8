#!/usr/bin/env python3
"""Compare two builds' device assembly, function by function.

usage: python3 scripts/isa_compare.py <dirA> <dirB> [--map FILE]

dirA and dirB hold the output of `hipcc ... --cuda-device-only -S` for the
same sources (one .s per .hip file, same file names).  For every kernel and
every out-of-line device function the script says whether the instruction
streams are equal, after replacing the function's own symbol and its local
labels by neutral names and dropping comments and the per-file __hip_cuid_*
symbol.  For kernels it also prints the resource metadata (.vgpr_count,
.sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size, the
spill counts and .kernarg_segment_size) and flags any that differ (META: the
stream is equal and only metadata differs).

--map FILE: lines "old-symbol new-symbol"; a function of dirA is compared
with the function of dirB its name maps to (for a change that renames
kernels).  "old-symbol -" says the function is retired on purpose.  Exit
status 1 if anything differs, or disappears or appears unannounced.

The script compares and counts only; it looks for no particular instruction.
"""
import argparse
import os
import re
import sys

META = ['.vgpr_count', '.sgpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
        '.vgpr_spill_count', '.sgpr_spill_count', '.kernarg_segment_size']
LOCAL = re.compile(r'\.L(BB|func_begin|func_end|tmp|JTI)(\d+)(?:_(\d+))?')


def local_label(m, seen):
    """a local label without its function number; .Ltmp labels in order of appearance"""
    kind, sub = m.group(1), m.group(3)
    if sub is not None:
        return '.L%s_%s' % (kind, sub)
    if kind == 'tmp':
        return '.Ltmp%d' % seen.setdefault(m.group(0), len(seen))
    return '.L' + kind


def parse(path, rename):
    """-> {symbol: {'kernel': bool, 'ins': [str], 'meta': {key: int}}}, symbols already renamed"""
    text = open(path).read()
    for old, new in rename.items():
        text = text.replace(old, new)
    lines = text.split('\n')
    funcs = {}
    types = re.findall(r'^\s*\.type\s+(\S+),@function', text, re.M)
    i = 0
    for sym in types:
        while i < len(lines) and lines[i].split(';')[0].strip() != sym + ':':
            i += 1
        body = []
        i += 1
        while i < len(lines) and not re.match(r'\s*\.size\s+' + re.escape(sym) + ',', lines[i]):
            body.append(lines[i])
            i += 1
        ins, labels = [], {}
        for ln in body:
            ln = ln.split(';')[0].rstrip()
            s = ln.strip()
            if not s or '__hip_cuid_' in s:
                continue
            if s.startswith('.') and not s.endswith(':'):
                continue  # directives (sections, alignment, the .amdhsa_ block)
            s = s.replace(sym, '<self>')
            s = LOCAL.sub(lambda m: local_label(m, labels), s)
            ins.append(re.sub(r'\s+', ' ', s))
        funcs[sym] = {'kernel': False, 'ins': ins, 'meta': {}}
    # kernel metadata: the YAML note at the end of the file, one list item per kernel
    note = text[text.find('amdhsa.kernels:'):]
    for item in re.split(r'^  - ', note, flags=re.M)[1:]:
        kv = dict(re.findall(r'^\s+(\.[a-z_]+):\s*(\S+)\s*$', '    ' + item, re.M))
        name = kv.get('.symbol', '')[:-3]
        if name in funcs:
            funcs[name]['kernel'] = True
            funcs[name]['meta'] = {k: int(kv[k]) for k in META if k in kv}
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('dir_a')
    ap.add_argument('dir_b')
    ap.add_argument('--map', help='file of "old new" symbol pairs')
    a = ap.parse_args()
    rename, retired = {}, set()
    if a.map:
        for ln in open(a.map):
            if ln.strip() and not ln.startswith('#'):
                old, new = ln.split()
                if new == '-':
                    retired.add(old)
                else:
                    rename[old] = new
    bad = 0
    files = sorted(f for f in os.listdir(a.dir_a) if f.endswith('.s'))
    for f in files:
        if not os.path.exists(os.path.join(a.dir_b, f)):
            print('%s: missing in %s' % (f, a.dir_b))
            bad += 1
            continue
        fa = parse(os.path.join(a.dir_a, f), rename)
        fb = parse(os.path.join(a.dir_b, f), {})
        print('== %s: %d functions (%d kernels) -> %d (%d kernels)' % (
            f, len(fa), sum(x['kernel'] for x in fa.values()), len(fb), sum(x['kernel'] for x in fb.values())))
        for sym in fa:
            kind = 'kernel' if fa[sym]['kernel'] else 'func  '
            if sym not in fb:
                print('  %s %s %s' % ('retired' if sym in retired else 'GONE  ', kind, sym))
                bad += sym not in retired
                continue
            x, y = fa[sym], fb[sym]
            same = x['ins'] == y['ins']
            dm = [k for k in META if x['meta'].get(k) != y['meta'].get(k)]
            first = ''
            if not same:
                n = next((i for i, (p, q) in enumerate(zip(x['ins'], y['ins'])) if p != q), min(len(x['ins']), len(y['ins'])))
                first = '  first difference at instruction %d of %d / %d' % (n, len(x['ins']), len(y['ins']))
            bad += (not same) or bool(dm)
            verdict = 'same  ' if same and not dm else 'META  ' if same else 'DIFFER'  # META: same stream, other metadata
            print('  %s %s %s  %d instr%s' % (verdict, kind, sym, len(y['ins']), first))
            if x['kernel']:
                print('         ' + ' '.join('%s=%s' % (k[1:], y['meta'].get(k)) for k in META))
                for k in dm:
                    print('         %s: %s -> %s' % (k, x['meta'].get(k), y['meta'].get(k)))
        for sym in fb:
            if sym not in fa:
                print('  NEW    %s %s' % ('kernel' if fb[sym]['kernel'] else 'func  ', sym))
                bad += 1
    print('%s' % ('all equal' if not bad else '%d differences' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
