#!/usr/bin/env python
"""Are the kernels of two device-side assembly listings the same machine code?  For refactors that must not touch the kernels: compile
the old and the new tree with the shipped flags,

    hipcc $(python -m vid2player3d_amd.build --print-flags physics_ll.hip[:regs]) --cuda-device-only -S physics_ll.hip -o new.s

and compare.  Per kernel (every physics_ll_kernel instantiation, env_pre_kernel, pair_scatter_kernel): instruction count, whether the
instruction streams are equal after normalising symbol names (enclosing namespaces, basic-block label numbers) and dropping comments and
.file / .loc directives, whether the kernel descriptors (.amdhsa_*) are equal, and the resource line.  Two streams in which only immediates of `s_movk_i32 s, N` / `s_cmpk_* s, N` differ
count as equal, and are reported as such, if EVERY such immediate of the kernel inside the range of values that moved (a handful of
consecutive numbers) moves by the same amount: these are the block numbers through which the compiler dispatches the exits of the rows'
unrolled loop, and they move when source lines that compile to nothing in a kernel (the cycle counters of the diagnostic
instantiation) add blocks in front of it.  (A constant of another meaning inside that range that moved by the same amount would pass
too; the range is a few numbers wide.)
The kernels of tennis_task.hip are known too (tennis_task_kernel<STEP, DUAL>, tennis_handover_kernel), and those of mvae_player.hip
(mvae_step_kernel, mvae_reset_kernel and their mvae_dual_* forms; they live in an anonymous namespace, which the symbol pattern allows),
and those of mvae_target.hip (mvae_target_kernel<RESET>, mvae_target_actions_kernel), tennis_reset.hip (tennis_reset_kernel) and
controller_actions.hip (controller_actions_kernel), and the reset by flags (mvae_reset_flagged_kernel of mvae_player_flagged.hip;
mvae_target_reset_flagged_kernel, env_push_state_flagged_kernel, ctl_reset_begin_kernel / _end_kernel of flag_reset.hip, next to
env_push_state_kernel of task_ops.hip), and the pair reset by flags (mvae_dual_reset_flagged_kernel of mvae_player_dual_flagged.hip;
ctl_pair_reset_begin_kernel / _end_kernel, tennis_dual_serve_flagged_kernel of pair_reset.hip), and the evaluation step
(tennis_eval_kernel of tennis_eval.hip), and the match record (match_record_frame_kernel, match_record_select_kernel,
match_record_copy_kernel of match_record.hip), and the two-hand backhand fix (two_hand_fix_kernel of two_hand_fix.hip).  A kernel that only the new listing has is
reported and does not count as a difference; one that only the old listing has does.
usage: tools/kernel_identity.py <old.s>[,<old2.s>...] <new.s>[,<new2.s>...]   (a kernel is looked up in every listing of its side)"""
import re
import sys

KERNELS = re.compile(r"^(_ZN\w*?(physics_ll_kernelI\w+?EEv|env_pre_kernelE|pair_scatter_kernelE|tennis_task_kernelI\w+?EEv|tennis_handover_kernelE|mvae_(?:dual_)?(?:step|reset)_kernelE|mvae_target_kernelI\w+?EEv|mvae_target_actions_kernelE|tennis_reset_kernelE|controller_actions_kernelE|mvae_reset_flagged_kernelE|mvae_target_reset_flagged_kernelE|env_push_state(?:_flagged)?_kernelE|ctl_reset_(?:begin|end)_kernelE|mvae_dual_reset_flagged_kernelE|ctl_pair_reset_(?:begin|end)_kernelE|tennis_dual_serve_flagged_kernelE|tennis_eval_kernelE|match_record_(?:frame|select|copy)_kernelE|two_hand_fix_kernelE)\w*):")
# the enclosing namespaces: v2p, v2p::ll_lds, v2p::ll_regs, or v2p itself renamed with a suffix (how the register object was built
# before the kernel had a namespace per build): _ZN3v2p17..., _ZN3v2p6ll_lds17..., _ZN3v2p7ll_regs17... -> _ZN@17...
NAMESPACES = re.compile(r"_ZN\d+v2p(?:_[a-z]+)?(?:\d+ll_[a-z]+)?")
RESOURCES = ("NumVgprs", "NumAgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def norm(line):
    line = line.split(";")[0].strip()
    line = NAMESPACES.sub("_ZN@", line)
    return re.sub(r"\.LBB\d+_", ".LBB_", line)


def kernels(paths):
    out = {}
    for path in paths.split(","):
        lines = open(path).read().split("\n")
        i = 0
        while i < len(lines):
            m = KERNELS.match(lines[i])
            if not m:
                i += 1
                continue
            name = m.group(2)
            if name.startswith("physics_ll_kernel"):  # template flags CONTACT MULTI TGS DIAG BALL JOBS LIMITS VFRIC
                name = "physics_ll_kernel<" + "".join(re.findall(r"Lb([01])E", name)) + ">"
            elif name.startswith("tennis_task_kernel"):  # template flags STEP DUAL (DUAL came later: a listing without it is DUAL = 0)
                name = "tennis_task_kernel<" + "".join(re.findall(r"Lb([01])E", name)).ljust(2, "0") + ">"
            elif name.startswith("mvae_target_kernel"):  # template flag RESET
                name = "mvae_target_kernel<" + "".join(re.findall(r"Lb([01])E", name)) + ">"
            else:
                name = name[:-1]
            # the code runs up to the kernel descriptor; the resource comments follow the function
            end = next(k for k in range(i, len(lines)) if lines[k].lstrip().startswith(".amdhsa_kernel"))
            body = [n for n in map(norm, lines[i + 1:end]) if n and not n.startswith((".file", ".loc", ".cfi"))]
            insts = [n for n in body if not n.endswith(":") and not n.startswith(".")]
            k = next(k for k in range(end, len(lines)) if lines[k].lstrip().startswith(".end_amdhsa_kernel"))
            desc = [norm(n.replace(m.group(1), "@KERNEL")) for n in lines[end:k]]  # (the symbol carries the template's parameter list)
            res = {}
            while len(res) < len(RESOURCES):
                k += 1
                m2 = re.match(r"; (\w+): (\S+)", lines[k])
                if m2 and m2.group(1) in RESOURCES:
                    res[m2.group(1)] = m2.group(2)
            kernarg = next(d.split()[-1] for d in desc if d.startswith(".amdhsa_kernarg_size"))
            out[name] = (body, len(insts), desc, " ".join("%s %s" % (r, res[r]) for r in RESOURCES) + " kernarg " + kernarg)
            i = end
    return out


DISPATCH = re.compile(r"^(s_movk_i32|s_cmpk_\w+) (s\d+), (0x[0-9a-f]+|\d+)$")


def dispatch_shift(b0, b1):
    """The one amount by which EVERY dispatch block number of two otherwise equal streams differs, or None.  Only `s_movk_i32` /
    `s_cmpk_*` immediates may differ; the differing ones span a range of values in the old stream (the block numbers: a handful of
    consecutive numbers), and every `s_movk_i32` / `s_cmpk_*` immediate of the kernel inside that range must move by the same amount -
    one that keeps its value, or moves otherwise, makes the streams unequal."""
    if len(b0) != len(b1):
        return None
    pairs = []
    for x, y in zip(b0, b1):
        mx, my = DISPATCH.match(x), DISPATCH.match(y)
        if mx and my and mx.group(1, 2) == my.group(1, 2):
            pairs.append((int(mx.group(3), 0), int(my.group(3), 0)))
        elif x != y:
            return None
    moved = [a for a, b in pairs if a != b]
    if not moved:
        return None
    lo, hi = min(moved), max(moved)
    if hi - lo > 16:
        return None
    shifts = {b - a for a, b in pairs if lo <= a <= hi}
    return shifts.pop() if len(shifts) == 1 and all(a == b for a, b in pairs if not lo <= a <= hi) else None


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print("%-40s only in the %s listing" % (name, "old" if name in old else "new"))
        bad += name in old
        continue
    (b0, n0, d0, r0), (b1, n1, d1, r1) = old[name], new[name]
    shift = None if b0 == b1 else dispatch_shift(b0, b1)
    same = (b0 == b1 or shift is not None) and d0 == d1
    bad += not same
    code = "equal" if b0 == b1 else ("equal but for dispatch block numbers (%+d)" % shift if shift is not None else "NOT equal (old %d)" % n0)
    print("%-40s %6d instructions  code %s  descriptor %s  %s%s" % (name, n1, code,
                                                                   "equal" if d0 == d1 else "NOT equal", r1, "" if r0 == r1 else "  (old: %s)" % r0))
print("%d kernels, %d differ" % (len(set(old) | set(new)), bad))
sys.exit(1 if bad else 0)
