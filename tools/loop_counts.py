#!/usr/bin/env python3
"""Instruction counts per loop of one kernel of the built engine, from the gfx950 disassembly: basic blocks, control-flow graph, strongly
connected components, nested by removing the edges back to each loop's entry blocks.  Per loop: VALU / SALU / scratch / global-memory / LDS
instructions, the v_mad_u64_u32 among the VALU ones and the calls (counted, not followed).  The figures of docs/kernels.md for the window loop
of k_ac17_enc_rows come from here.
usage: python tools/loop_counts.py k_ac17_enc_rows [path/to/librabe_hip.so]"""
import os
import re
import subprocess
import sys
import tempfile

sys.setrecursionlimit(100000)
LLVM = "/opt/rocm/lib/llvm/bin/"
kname = sys.argv[1]
lib = sys.argv[2] if len(sys.argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "rabe_amd", "librabe_hip.so")


def listing():
    """the disassembly of the code object that holds the kernel (the library's .hip_fatbin has one offload bundle per translation unit)"""
    with tempfile.TemporaryDirectory() as t:
        fat = os.path.join(t, "fat.bin")
        subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
        d = open(fat, "rb").read()
        magic, starts, i = b"__CLANG_OFFLOAD_BUNDLE__", [], d.find(b"__CLANG_OFFLOAD_BUNDLE__")
        while i >= 0:
            starts.append(i)
            i = d.find(magic, i + 1)
        for k, s in enumerate(starts):
            b = os.path.join(t, "bundle%02d" % k)
            open(b, "wb").write(d[s:starts[k + 1] if k + 1 < len(starts) else len(d)])
            subprocess.run([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + b,
                            "--output=" + b + ".o"], check=True)
            syms = subprocess.run([LLVM + "llvm-readelf", "-s", b + ".o"], check=True, capture_output=True, text=True).stdout
            if re.search(r"\b_Z\d+%s[A-Z]" % kname, syms):
                return subprocess.run([LLVM + "llvm-objdump", "-d", "--no-show-raw-insn", "--symbolize-operands", b + ".o"], check=True,
                                      capture_output=True, text=True).stdout
    raise SystemExit("no kernel %s in %s" % (kname, lib))


lines = listing().split('\n')
start = next(i for i, l in enumerate(lines) if re.match(r'^[0-9a-f]+ <_Z\d+%s[A-Z]\S*>:' % kname, l))
end = next((i for i in range(start + 1, len(lines)) if re.match(r'^[0-9a-f]+ <[^L]\S*>:', lines[i])), len(lines))   # the unit's last kernel
ins, labels = [], {}
for l in lines[start + 1:end]:
    l = l.split('//')[0].strip()
    m = re.match(r'^(?:[0-9a-f]+ )?<?(L\d+)>?:$', l)
    if m:
        labels[m.group(1)] = len(ins); continue
    if l: ins.append(l)
n = len(ins)
leaders = {0} | set(labels.values())
tgt = {}
for i, l in enumerate(ins):
    m = re.match(r'^(s_cbranch_\w+|s_branch)\s+(L\d+)', l)
    if m:
        tgt[i] = (labels[m.group(2)], m.group(1) != 's_branch'); leaders.add(i + 1)
    if l.startswith('s_endpgm') or l.startswith('s_setpc'): leaders.add(i + 1)
leaders = sorted(x for x in leaders if x < n)
bid = {}
blocks = []
for k, a in enumerate(leaders):
    b = leaders[k + 1] if k + 1 < len(leaders) else n
    blocks.append((a, b))
    for i in range(a, b): bid[i] = k
succ = []
for a, b in blocks:
    last = b - 1; s = []
    if last in tgt:
        s.append(bid[tgt[last][0]])
        if tgt[last][1] and b < n: s.append(bid[b])
    elif not (ins[last].startswith('s_endpgm') or ins[last].startswith('s_setpc')) and b < n:
        s.append(bid[b])
    succ.append(s)
def find_sccs(nodes, succ_of):
    index, low, on, st, out, cnt = {}, {}, set(), [], [], [0]
    def sc(v):
        index[v] = low[v] = cnt[0]; cnt[0] += 1; st.append(v); on.add(v)
        for w in succ_of(v):
            if w not in index: sc(w); low[v] = min(low[v], low[w])
            elif w in on: low[v] = min(low[v], index[w])
        if low[v] == index[v]:
            comp = []
            while True:
                w = st.pop(); on.discard(w); comp.append(w)
                if w == v: break
            if len(comp) > 1 or v in succ_of(v): out.append(sorted(comp))
    for v in nodes:
        if v not in index: sc(v)
    return out
pred = [[] for _ in blocks]
for v, ss in enumerate(succ):
    for w in ss: pred[w].append(v)
def cls(op):
    for p, c in (('v_', 'valu'), ('s_', 'salu'), ('scratch_', 'scratch'), ('global_', 'vmem'), ('buffer_', 'vmem'), ('flat_', 'vmem'), ('ds_', 'lds')):
        if op.startswith(p): return c
    return 'other'
def count(idx):
    c = {'valu': 0, 'salu': 0, 'scratch': 0, 'vmem': 0, 'lds': 0, 'mad_u64': 0, 'calls': 0}
    for i in idx:
        op = ins[i].split()[0]
        k = cls(op)
        if k in c: c[k] += 1
        if op.startswith('v_mad_u64_u32'): c['mad_u64'] += 1
        if op.startswith('s_swappc'): c['calls'] += 1
    return c
print(kname, 'instructions', n, count(range(n)))
def walk(nodes, removed, depth):
    ns = set(nodes)
    so = lambda v: [w for w in succ[v] if w in ns and (v, w) not in removed]
    for comp in sorted(find_sccs(sorted(ns), so), key=lambda c: blocks[c[0]][0]):
        idx = [i for b in comp for i in range(*blocks[b])]
        if len(idx) < 200: continue
        print('  ' * depth + 'loop depth %d: %d blocks, first instr %d, %d instructions:' % (depth, len(comp), blocks[comp[0]][0], len(idx)), count(idx))
        cs = set(comp)
        heads = [b for b in comp if any(p not in cs for p in pred[b])] or [comp[0]]
        rem = set(removed) | {(p, h) for h in heads for p in pred[h] if p in cs}
        walk(comp, rem, depth + 1)
walk(range(len(blocks)), set(), 0)
