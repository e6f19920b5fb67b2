#!/usr/bin/env python3
"""Instruction ledger of one kernel of mpcb_split.hip (host only: the compile cross-targets
gfx950, nothing runs on a GPU).

Compiles mpc_blaster_amd/csrc/mpcb_split.hip device-only with the flags of mpc_blaster_amd/build.py
and prints, for every depth-1 loop of the named kernel and for the straight-line rest, the
instruction count by broad class, then the kernel's registers, scratch and LDS.  Loops are the
strongly connected components of the kernel's control-flow graph (labels and branch targets of the
assembly), so a block the compiler placed outside its loop's annotated range is still counted.
The classes are taken from mnemonic prefixes:

    fp64    vector fp64 arithmetic (v_*_f64*, not moves / compares / conversions)
    dpp     DPP moves (v_mov_*_dpp)
    valu    every other vector ALU instruction
    salu    scalar ALU and branches
    wait    s_waitcnt / s_nop / s_sleep
    lds     ds_*
    vmem    global_* / buffer_* / flat_* / scratch_*

    tools/isa_ledger.py [--kernel MANGLED] [--csrc DIR] [--json]
    tools/isa_ledger.py --update profiles/isa_c2.json --entry result [--commit ID]

The two loops with the most instructions are named, in program order, ``rollout`` (the RK4
interval of row_body, with its slow-path redo) and ``riccati`` (the stage of riccati_body).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from mpc_blaster_amd import build as _b  # noqa: E402

KERNEL = '_ZN4mpcb18row_riccati_kernelILb0ELb1EEEvNS_9SplitArgsIdEE'   # row_riccati_kernel<false, true>
CLASSES = ('fp64', 'dpp', 'valu', 'salu', 'wait', 'lds', 'vmem')


def have_hipcc() -> bool:
    return os.path.exists(_b.HIPCC) or shutil.which(_b.HIPCC) is not None


def classify(m: str) -> str:
    if m in ('s_waitcnt', 's_nop', 's_sleep') or m.startswith('s_waitcnt'):
        return 'wait'
    if m.startswith('s_'):
        return 'salu'
    if m.startswith('ds_'):
        return 'lds'
    if m.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    if m.startswith('v_mov') and m.endswith('_dpp'):
        return 'dpp'
    if '_f64' in m and not m.startswith(('v_mov', 'v_cmp', 'v_cvt', 'v_cndmask')):
        return 'fp64'
    return 'valu'


def assembly(csrc: str | None = None, defines=()) -> str:
    src = os.path.join(csrc or _b.CSRC, 'mpcb_split.hip')
    flags = [f for f in _b.FLAGS if f not in ('-shared', '-fPIC')]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'split.s')
        cmd = [_b.HIPCC, *flags, *defines, '--cuda-device-only', '-S', src, '-o', out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise SystemExit(f'{" ".join(cmd)}\n{r.stderr}')
        return open(out).read()


def blocks_of(s: str, kernel: str):
    """[(label, [mnemonic...], [branch targets], falls_through)] of the kernel, in program order."""
    i = s.index('\n' + kernel + ':')
    j = s.index('.Lfunc_end', i)
    blocks = [['<entry>', [], [], True]]
    for line in s[i:j].split('\n')[2:]:
        ls = line.strip()
        m = re.match(r'(\.LBB\d+_\d+):', ls) or re.match(r'; %bb\.(\d+):', ls)
        if m:
            blocks.append([m.group(1), [], [], True])
            continue
        if not ls or ls.startswith((';', '.')):
            continue
        op = ls.split()[0]
        cur = blocks[-1]
        cur[1].append(op)
        if op.startswith('s_cbranch') or op == 's_branch':
            cur[2].append(ls.split()[1])
            if op == 's_branch':
                cur[3] = False
        elif op in ('s_endpgm', 's_setpc_b64'):
            cur[3] = False
    return blocks


def loops_of(blocks):
    """Strongly connected components with a cycle, as sorted lists of block indices."""
    idx = {b[0]: n for n, b in enumerate(blocks)}
    succ = []
    for n, b in enumerate(blocks):
        e = [idx[t] for t in b[2] if t in idx]
        if b[3] and n + 1 < len(blocks):
            e.append(n + 1)
        succ.append(e)
    # Tarjan, iterative
    index, low, on, stack, comps, counter = {}, {}, set(), [], [], [0]
    for root in range(len(blocks)):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, pi = work.pop()
            if pi == 0:
                index[v] = low[v] = counter[0]
                counter[0] += 1
                stack.append(v)
                on.add(v)
            recurse = False
            for k in range(pi, len(succ[v])):
                w = succ[v][k]
                if w not in index:
                    work.append((v, k + 1))
                    work.append((w, 0))
                    recurse = True
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            if recurse:
                continue
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(sorted(comp))
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return sorted(comps)


def count(blocks, which):
    c = dict.fromkeys(CLASSES, 0)
    for n in which:
        for op in blocks[n][1]:
            c[classify(op)] += 1
    c['total'] = sum(c[k] for k in CLASSES)
    return c


def meta_of(s: str, kernel: str) -> dict:
    j = s.index('.Lfunc_end', s.index('\n' + kernel + ':'))
    tail = s[j:j + 4000]
    out = {}
    for key, pat in (('vgpr', r'; NumVgprs: (\d+)'), ('agpr', r'; NumAgprs: (\d+)'),
                     ('scratch', r'; ScratchSize: (\d+)'), ('lds', r'; LDSByteSize: (\d+)')):
        out[key] = int(re.search(pat, tail).group(1))
    md = s[s.index('amdhsa.kernels:'):]
    for block in re.split(r'\n  - ', md)[1:]:
        if re.search(r'^\s*\.name:\s+' + re.escape(kernel) + r'\s*$', block, re.M):
            out['vgpr_spill'] = int(re.search(r'\.vgpr_spill_count:\s+(\d+)', block).group(1))
            out['sgpr_spill'] = int(re.search(r'\.sgpr_spill_count:\s+(\d+)', block).group(1))
    return out


def ledger(kernel: str = KERNEL, csrc: str | None = None, defines=()) -> dict:
    s = assembly(csrc, defines)
    blocks = blocks_of(s, kernel)
    comps = loops_of(blocks)
    inside = {n for c in comps for n in c}
    loops = []
    for c in comps:
        e = count(blocks, c)
        e['header'] = blocks[c[0]][0]
        e['blocks'] = len(c)
        e['largest_block'] = max(len(blocks[n][1]) for n in c)
        loops.append(e)
    for name, e in zip(('rollout', 'riccati'),
                       sorted(sorted(loops, key=lambda e: -e['total'])[:2], key=loops.index)):
        e['role'] = name
    return {'kernel': kernel, 'loops': loops,
            'straight_line': count(blocks, [n for n in range(len(blocks)) if n not in inside]),
            'meta': meta_of(s, kernel)}


def role(entry: dict, name: str) -> dict:
    return next(e for e in entry['loops'] if e.get('role') == name)


def show(entry: dict) -> None:
    print(entry['kernel'])
    hdr = f'{"part":28s}' + ''.join(f'{k:>7s}' for k in CLASSES + ('total',))
    print(hdr)
    for e in entry['loops']:
        name = f'loop {e["header"]} {e.get("role", "")} ({e["blocks"]} blocks, largest {e["largest_block"]})'
        print(f'{name:28s}')
        print(' ' * 28 + ''.join(f'{e[k]:7d}' for k in CLASSES + ('total',)))
    e = entry['straight_line']
    print(f'{"straight-line rest":28s}' + ''.join(f'{e[k]:7d}' for k in CLASSES + ('total',)))
    print('meta', ' '.join(f'{k}={v}' for k, v in entry['meta'].items()))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument('--kernel', default=KERNEL)
    ap.add_argument('--csrc', default=None, help='directory of the sources (default: this tree)')
    ap.add_argument('-D', dest='defines', action='append', default=[])
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--update', metavar='FILE', help='write the ledger into FILE under --entry')
    ap.add_argument('--entry', choices=('parent', 'result'), default='result')
    ap.add_argument('--commit', default='')
    args = ap.parse_args()
    entry = ledger(args.kernel, args.csrc, [f'-D{d}' for d in args.defines])
    if args.update:
        doc = json.load(open(args.update)) if os.path.exists(args.update) else {}
        if args.commit:
            entry['commit'] = args.commit
        doc[args.entry] = entry
        with open(args.update, 'w') as f:
            json.dump(doc, f, indent=1)
            f.write('\n')
    if args.json:
        print(json.dumps(entry, indent=1))
    else:
        show(entry)
    return 0


if __name__ == '__main__':
    sys.exit(main())
