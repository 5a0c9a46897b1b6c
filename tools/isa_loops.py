#!/usr/bin/env python
"""Instruction counts of one kernel of a device-side assembly listing by SOURCE LINE RANGE and by LOOP (CPU only).  Compile with line
tables, which do not change the code:

    hipcc $(python -m vid2player3d_amd.build --print-flags physics_ll.hip) -gline-tables-only --cuda-device-only -S physics_ll.hip -o k.s

usage: tools/isa_loops.py k.s <template flags, e.g. 10000100> [--loops] [--range name=first-last ...] [--dump first-last]
  --loops   every innermost loop (a backward branch): its label, the source lines of its body, its counts
  --range   counts of all instructions whose .loc line lies in first..last, per occurrence (an inlined lambda appears once per call site:
            consecutive runs of instructions separated by more than GAP other instructions are listed apart)
  --dump    the instructions of that line range, in listing order, with their source lines
Classes: float VALU (v_fma / v_fmac / v_mul / v_add / v_sub / v_mac / v_dot _f32, packed too), select (v_cndmask), move (v_mov, DPP moves
included), lane read (v_readlane / v_readfirstlane / v_writelane), other VALU, LDS (ds_*), wait (s_waitcnt / s_nop), branch, other scalar."""
import re
import sys

GAP = 400
FLOAT = re.compile(r"^v_(pk_)?(fma|fmac|mul|add|sub|subrev|mac|mad|max|min|rcp|rsq|sqrt|dot\w*)_(legacy_)?f32")


def klass(op):
    if FLOAT.match(op):
        return "float"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith("v_mov") or op.startswith("v_accvgpr"):
        return "move"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
        return "lane"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("s_waitcnt", "s_nop")):
        return "wait"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_"):
        return "scalar"
    return "mem"  # global / scratch / buffer / flat


ORDER = ("float", "select", "move", "lane", "valu", "lds", "wait", "branch", "scalar", "mem")


def kernel(path, flags):
    want = "physics_ll_kernelI" + "".join("Lb%sE" % c for c in flags)
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN\w*" + want + r"\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith(".amdhsa_kernel"))
    insts, labels, line = [], {}, 0
    for l in lines[start + 1:end]:
        s = l.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"\.loc\s+\d+\s+(\d+)", s)
        if m:
            line = int(m.group(1))
            continue
        if s.endswith(":"):
            labels[s[:-1]] = len(insts)
            continue
        if s.startswith("."):
            continue
        insts.append((line, s))
    return insts, labels


def counts(sub):
    c = dict.fromkeys(ORDER, 0)
    for _, s in sub:
        c[klass(s.split()[0])] += 1
    return c


def fmt(c):
    return "  ".join("%s %d" % (k, c[k]) for k in ORDER if c[k]) + "  | total %d" % sum(c.values())


def main():
    path, flags = sys.argv[1], sys.argv[2]
    insts, labels = kernel(path, flags)
    print("%d instructions; %s" % (len(insts), fmt(counts(insts))))
    args = sys.argv[3:]
    if "--loops" in args:
        loops = []
        for i, (_, s) in enumerate(insts):
            p = s.split()
            if p[0].startswith(("s_cbranch", "s_branch")) and p[-1] in labels and labels[p[-1]] <= i:
                loops.append((labels[p[-1]], i, p[-1]))
        inner = [l for l in loops if not any(o is not l and l[0] <= o[0] and o[1] <= l[1] and (o[0], o[1]) != (l[0], l[1]) for o in loops)]
        for a, b, name in sorted(inner):
            src = sorted({ln for ln, _ in insts[a:b + 1]})
            print("loop %-12s inst %6d..%6d lines %d..%d  %s" % (name, a, b, src[0], src[-1], fmt(counts(insts[a:b + 1]))))
    for k, arg in enumerate(args):
        if arg == "--range":
            name, rng = args[k + 1].split("=")
            lo, hi = map(int, rng.split("-"))
            idx = [i for i, (ln, _) in enumerate(insts) if lo <= ln <= hi]
            runs, cur = [], []
            for i in idx:
                if cur and i - cur[-1] > GAP:
                    runs.append(cur)
                    cur = []
                cur.append(i)
            if cur:
                runs.append(cur)
            for r in runs:
                print("%-14s lines %d-%d at inst %6d..%6d: %s" % (name, lo, hi, r[0], r[-1], fmt(counts([insts[i] for i in r]))))
        if arg == "--dump":
            lo, hi = map(int, args[k + 1].split("-"))
            inv = {}
            for n, i in labels.items():
                inv.setdefault(i, []).append(n)
            for i, (ln, s) in enumerate(insts):
                if lo <= ln <= hi:
                    for n in inv.get(i, []):
                        print("%s:" % n)
                    print("%6d  L%-5d %s" % (i, ln, s))


main()
