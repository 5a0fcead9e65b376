#!/usr/bin/env python3
"""Do two source trees compile to the same gfx950 device code?  tools/kernel_isa_diff.py <tree A> <tree B> [-j N]

Compiles every .hip of <tree>/deeptables_amd/csrc (or of <tree> itself when it has no such directory) to assembly, device
side only, splits the output per function symbol and compares, symbol by symbol across all files of a tree: the
.amdhsa_* kernel descriptor (VGPRs, SGPRs, scratch, LDS, wavefront size, ...) and the instruction text with comments
dropped and the unit-local label numbers (.LBB<n>_<m>, .Lfunc_end<n>, ...) normalised.  Which file a kernel lives in is
not compared: a kernel may move between translation units.  CPU only; exit status 1 when anything is missing, added or
different."""
import argparse
import difflib
import glob
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-x', 'hip', '--cuda-device-only', '-S']
MAX_JOBS = 16


def sources(tree):
    csrc = os.path.join(tree, 'deeptables_amd', 'csrc')
    return sorted(glob.glob(os.path.join(csrc if os.path.isdir(csrc) else tree, '*.hip')))


def compile_asm(job):
    src, out = job
    r = subprocess.run([HIPCC] + FLAGS + [src, '-o', out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode:
        raise RuntimeError(f'{src}: hipcc failed\n{r.stdout.decode()}')
    return open(out).read()


def normalise(lines):
    """instruction text of one function: no comments, no blank lines; .LBB<n>_<m> loses the function number n, every
    other numbered local label is renumbered in its order of appearance"""
    seen = {}

    def label(m):
        t = m.group(0)
        u = re.match(r'^(\.L[A-Za-z]+)\d+_(\d+)$', t)
        if u:
            return f'{u.group(1)}_{u.group(2)}'
        u = re.match(r'^(\.L\w*[A-Za-z_])\d+$', t)
        return seen.setdefault(t, f'{u.group(1)}#{len(seen)}') if u else t

    out = []
    for ln in lines:
        ln = ln.split(';', 1)[0].strip()
        if not ln:
            continue
        ln = re.sub(r'\.L\w+', label, ln)
        out.append(re.sub(r'\s+', ' ', ln))
    return out


def functions(asm):
    """{symbol: (descriptor lines, instruction lines)} of one assembly file; the descriptor is empty for a device
    function that is not a kernel"""
    s = asm.split('\n')
    funcs = set(re.findall(r'^\s*\.type\s+(\S+),@function', asm, re.M))
    out = {}
    i = 0
    while i < len(s):
        m = re.match(r'^([A-Za-z_$][\w$.]*):', s[i])
        if m and m.group(1) in funcs:
            j = i + 1
            while j < len(s) and not s[j].startswith('.Lfunc_end'):
                j += 1
            # the kernel descriptor is emitted inside the function's range, after its last instruction
            lines = s[i + 1:j]
            k0 = next((k for k, x in enumerate(lines) if x.strip().startswith('.amdhsa_kernel')), len(lines))
            k1 = next((k for k, x in enumerate(lines) if x.strip().startswith('.end_amdhsa_kernel')), len(lines))
            desc = [re.sub(r'\s+', ' ', x.strip()) for x in lines[k0 + 1:k1]]
            out[m.group(1)] = (desc, normalise(lines[:k0] + lines[k1 + 1:]))
            i = j
        i += 1
    return out


def tree_functions(tree, jobs, tmp, tag):
    srcs = sources(tree)
    if not srcs:
        sys.exit(f'{tree}: no .hip sources')
    todo = [(p, os.path.join(tmp, f'{tag}_{os.path.basename(p)}.s')) for p in srcs]
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        asms = list(ex.map(compile_asm, todo))
    found = {}      # symbol -> [(file, descriptor, text)]: a template may be instantiated by more than one unit
    for p, asm in zip(srcs, asms):
        for sym, (d, t) in functions(asm).items():
            found.setdefault(sym, []).append((os.path.basename(p), d, t))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('-j', type=int, default=min(MAX_JOBS, os.cpu_count() or 4), help=f'parallel compiles (at most {MAX_JOBS})')
    ap.add_argument('--lines', type=int, default=12, help='diff lines shown per differing kernel')
    a = ap.parse_args()
    jobs = max(1, min(a.j, MAX_JOBS))
    with tempfile.TemporaryDirectory() as tmp:
        fa = tree_functions(a.tree_a, jobs, tmp, 'a')
        fb = tree_functions(a.tree_b, jobs, tmp, 'b')
    missing = sorted(set(fa) - set(fb))
    added = sorted(set(fb) - set(fa))
    differing, moved = [], 0
    for sym in sorted(set(fa) & set(fb)):
        va = sorted((d, t) for _, d, t in fa[sym])
        vb = sorted((d, t) for _, d, t in fb[sym])
        if va != vb:
            differing.append(sym)
        moved += sorted(f for f, _, _ in fa[sym]) != sorted(f for f, _, _ in fb[sym])
    for sym in missing:
        print(f'missing  {sym}  ({", ".join(f for f, _, _ in fa[sym])})')
    for sym in added:
        print(f'added    {sym}  ({", ".join(f for f, _, _ in fb[sym])})')
    for sym in differing:
        (fa_, da, ta), (fb_, db, tb) = fa[sym][0], fb[sym][0]
        what = ' + '.join(w for w, x, y in (('descriptor', da, db), ('instructions', ta, tb)) if x != y)
        print(f'differs  {sym}  ({fa_} -> {fb_}): {what}')
        shown = list(difflib.unified_diff(da + ta, db + tb, 'a', 'b', lineterm='', n=1))[2:2 + a.lines]
        print('\n'.join('    ' + x for x in shown))
    nk = lambda f: sum(1 for v in f.values() if v[0][1])
    per_file = lambda f: Counter(x[0] for v in f.values() for x in v)
    ca, cb = per_file(fa), per_file(fb)
    for name in sorted(set(ca) | set(cb)):
        if ca[name] != cb[name]:
            print(f'functions in {name}: {ca[name]} -> {cb[name]}')
    print(f'kernel_isa_diff: {len(fa)} functions ({nk(fa)} kernels) in A, {len(fb)} ({nk(fb)} kernels) in B: '
          f'{len(missing)} missing, {len(added)} added, {len(differing)} differing; {moved} in another file')
    return 1 if missing or added or differing else 0


if __name__ == '__main__':
    sys.exit(main())
