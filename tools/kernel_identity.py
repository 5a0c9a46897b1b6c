#!/usr/bin/env python
"""Are the kernels of two device-side assembly listings the same machine code?  For refactors that must not touch the kernels: compile
the old and the new tree with the shipped flags,

    hipcc $(python -m vid2player3d_amd.build --print-flags physics_ll.hip[:regs]) --cuda-device-only -S physics_ll.hip -o new.s

and compare.  Per kernel (every physics_ll_kernel instantiation, env_pre_kernel, pair_scatter_kernel): instruction count, whether the
instruction streams are equal after normalising symbol names (enclosing namespaces, basic-block label numbers) and dropping comments and
.file / .loc directives, whether the kernel descriptors (.amdhsa_*) are equal, and the resource line.
usage: tools/kernel_identity.py <old.s>[,<old2.s>...] <new.s>[,<new2.s>...]   (a kernel is looked up in every listing of its side)"""
import re
import sys

KERNELS = re.compile(r"^(_ZN\w*?(physics_ll_kernelI\w+?EEv|env_pre_kernelE|pair_scatter_kernelE)\w*):")
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
            else:
                name = name[:-1]
            # the code runs up to the kernel descriptor; the resource comments follow the function
            end = next(k for k in range(i, len(lines)) if lines[k].lstrip().startswith(".amdhsa_kernel"))
            body = [n for n in map(norm, lines[i + 1:end]) if n and not n.startswith((".file", ".loc", ".cfi"))]
            insts = [n for n in body if not n.endswith(":") and not n.startswith(".")]
            k = next(k for k in range(end, len(lines)) if lines[k].lstrip().startswith(".end_amdhsa_kernel"))
            desc = [norm(n) for n in lines[end:k]]
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


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
bad = 0
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        print("%-40s only in the %s listing" % (name, "old" if name in old else "new"))
        bad += 1
        continue
    (b0, n0, d0, r0), (b1, n1, d1, r1) = old[name], new[name]
    same = b0 == b1 and d0 == d1
    bad += not same
    print("%-40s %6d instructions  code %s  descriptor %s  %s%s" % (name, n1, "equal" if b0 == b1 else "NOT equal (old %d)" % n0,
                                                                   "equal" if d0 == d1 else "NOT equal", r1, "" if r0 == r1 else "  (old: %s)" % r0))
print("%d kernels, %d differ" % (len(set(old) | set(new)), bad))
sys.exit(1 if bad else 0)
