"""Build libv2p_rollout.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU, so this runs in the build container; the resulting .so
travels to the GPU box with the repo snapshot.  `python -m vid2player3d_amd.build`
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libv2p_rollout.so")
SOURCES = ["capi.hip", "device_owner.hip", "model_compile.hip", "env.hip", "motion_state.hip", "task_ops.hip", "shape_compile.hip", "motion_build.hip", "physics.hip", "physics_ll.hip", "physics_ll_host.hip", "ball_rollout.hip", "tennis_task.hip", "tennis_eval.hip", "tennis_reset.hip", "controller_actions.hip", "mvae_player.hip", "mvae_player_dual.hip", "mvae_target.hip", "policy_io.hip", "ctl_ppo.hip", "mvae_player_flagged.hip", "flag_reset.hip", "mvae_player_dual_flagged.hip", "pair_reset.hip", "match_record.hip", "two_hand_fix.hip"]
HEADERS = ["v2p_internal.hpp", "device_guards.hpp", "ll_schedule.hpp", "ll_forms.hpp", "ll_contact_setup.inc", "v2p_dev.hpp", "v2p_math.inc", "phys_math.hpp", "phys_common.hpp", "motion_sample.inc", "hull_gjk.hpp", "post_ops.inc", "strict_ops.inc", "tennis_task.hpp", "tennis_task_dev.hpp", "tennis_eval.hpp", "tennis_pose_dev.hpp", "match_record.hpp", "two_hand_fix.hpp", "tennis_row.inc", "tennis_reset.hpp", "controller_actions.hpp", "philox.hpp", "mvae_player.hpp", "mvae_player_dev.hpp", "mvae_rows.inc", "mvae_target.hpp", "mvae_target_dev.hpp", "mvae_target_row.inc", "flag_reset.hpp", "pair_reset.hpp", "policy_io.hpp", "ctl_ppo.hpp", "obs_imitation_row.inc", "ref_rotations.hpp", os.path.join("..", "..", "include", "v2p_rollout.h")]
ARCH = "gfx950"


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the HIP extension cannot be built")


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build_info():
    """What the bench line records about the build."""
    return {"arch": ARCH, "kernel_source_sha16": kernel_source_hash(), "physics_ll_math": "precise" if os.environ.get("V2P_LL_STRICT_MATH") else "relaxed (" + " ".join(LL_MATH_FLAGS) + "; precise device libraries, strict pre-physics prologue)",
            "hipcc": _hipcc()}


LL_CODEGEN_FLAGS = ["-mllvm", "-sink-insts-to-avoid-spills=1"]
LL_MATH_FLAGS = ["-fassociative-math", "-freciprocal-math", "-fno-signed-zeros", "-fno-trapping-math", "-fno-honor-nans"]
# what the physics kernel is compiled from: the counters kept under profiles/ (VALU instructions, HBM bytes per launch) describe ONE
# kernel; they carry this hash, and bench.py drops them from its line when the sources have moved on
KERNEL_SOURCES = ["physics_ll.hip", "phys_common.hpp", "phys_math.hpp", "hull_gjk.hpp", "strict_ops.inc", "post_ops.inc", "v2p_math.inc", "motion_sample.inc", "v2p_internal.hpp", "device_guards.hpp", "ll_schedule.hpp", "ll_forms.hpp", "ll_contact_setup.inc", "v2p_dev.hpp"]


def kernel_source_hash():
    """sha256 (16 hex digits) of the sources of physics_ll_kernel and of the flags it is built with."""
    import hashlib

    h = hashlib.sha256()
    for s in KERNEL_SOURCES:
        with open(os.path.join(CSRC, s), "rb") as f:
            h.update(s.encode() + b"\0" + f.read() + b"\0")
    h.update(" ".join(LL_MATH_FLAGS + LL_CODEGEN_FLAGS + [os.environ.get("V2P_LL_STRICT_MATH", ""), os.environ.get("V2P_FLAGS_PHYSICS_LL", "")]).encode())
    return h.hexdigest()[:16]


# -fno-slp-vectorize: the SLP vectoriser packs adjacent fp32 ops into v_pk_* on 64-bit register pairs, which costs the
# physics kernels ~160 registers of pressure (1 instead of 2 waves/SIMD) and is slower next to dependent chains anyway
BASE_FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-fno-vectorize", "-fno-slp-vectorize", "-Wall",
              "-Wno-unused-function"]
# physics_ll.hip is compiled twice: the default object and the register build, whose kernel and launcher carry their own names (see the
# head of the file).  (the ILP scheduler: this build runs where a launch is as long as its heaviest wave's chain, +1.6 % at 4096 envs,
# +2.1 % at 1024; for the default build, bound by instruction issue at three waves per SIMD, the same switch costs 0.3 %:
# profiles/r04e_dual_build.txt)
LL_REGS_FLAGS = ["-DV2P_LL_REGS_BUILD", "-DV2P_LL_WPS=2", "-DV2P_LL_WPS_BALL=2", "-DV2P_LL_WPS_LIMITS=2", "-DV2P_LL_PARK2=0", "-DV2P_LL_PARK3=0",
                 "-mllvm", "-amdgpu-sched-strategy=iterative-ilp"]


def compile_flags(source, regs=False):
    """The hipcc flags of one object of the library (everything but `-c <source> -o <object>`): what build() compiles with, and what the
    tools that look at a kernel's registers and spills (tools/kres.sh, ...) compile with.  regs: the register build of physics_ll.hip."""
    fl = list(BASE_FLAGS)
    if regs:
        fl += LL_REGS_FLAGS
    if source in ("motion_state.hip", "task_ops.hip", "shape_compile.hip", "motion_build.hip", "tennis_task.hip", "tennis_eval.hip", "tennis_reset.hip", "controller_actions.hip", "mvae_player.hip", "mvae_player_dual.hip", "mvae_target.hip", "policy_io.hip", "ctl_ppo.hip", "mvae_player_flagged.hip", "flag_reset.hip", "mvae_player_dual_flagged.hip", "pair_reset.hip", "match_record.hip", "two_hand_fix.hip"):
        # the task-side kernels restate torch elementwise code: no FMA contraction, so that ill-conditioned spots of the
        # reference itself (acos of a dot product next to 1 in slerp / angle-axis) round the way torch rounds them
        fl = [f if f != "-ffp-contract=fast" else "-ffp-contract=off" for f in fl]
    if source in ("physics_ll.hip", "physics_ll_host.hip", "ball_rollout.hip"):
        # the link-per-lane physics kernel (and the stand-alone pre-physics kernel that shares namespace strict with it; and the free-ball
        # kernel, which restates the ball lane of the former and is meant to round like it): relaxed fp32
        # arithmetic for the code of this file, precise device libraries (see the head of physics_ll.hip for why the flags are spelled
        # out instead of -ffast-math); V2P_LL_STRICT_MATH=1 builds it precise (A/B, bisecting)
        fl = [f if f != "-ffp-contract=fast" else "-ffp-contract=fast-honor-pragmas" for f in fl]
        fl = fl + (["-DV2P_LL_STRICT_MATH"] if os.environ.get("V2P_LL_STRICT_MATH") else LL_MATH_FLAGS)
        # MachineLICM hoists every loop-invariant address / uniform expression in front of the substep loop and the register allocator then
        # spills them across it; this switch lets it sink them back instead (round 6: racket + ball + limits 328 -> 184 B of scratch per
        # lane, 12.89 -> 13.64 M env-steps/s; limits alone 84 -> 0 B; the headline instantiation 20 -> 0 B, unchanged speed:
        # profiles/r06d_variants_spill.log)
        fl = fl + LL_CODEGEN_FLAGS
    extra = os.environ.get("V2P_FLAGS_" + source.split(".")[0].upper() + ("_REGS" if regs else ""))  # experiments: per-object flag override, e.g. V2P_FLAGS_PHYSICS_LL="-O1" (V2P_FLAGS_PHYSICS_LL_REGS: the register build)
    if extra:
        fl = [f for f in fl if f != "-O3"] + extra.split()
    return fl


def build(force=False, verbose=False, lib_out=None, tag=""):
    """out / tag: build a variant library next to the default one (A/B experiments: tools/variants.sh)."""
    if lib_out is None and not force and not needs_build():
        return LIB
    objs = []
    procs = []
    for s in SOURCES + ["physics_ll.hip:regs"]:
        regs = s.endswith(":regs")
        s = s.split(":")[0]
        obj = os.path.join(CSRC, s.replace(".hip", ("_regs" if regs else "") + tag + ".o"))
        cmd = [_hipcc()] + compile_flags(s, regs) + ["-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for cmd, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            sys.stderr.write(out.decode())
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
        if verbose and out:
            print(out.decode())
    cmd = [_hipcc(), "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib_out or LIB] + objs
    subprocess.check_call(cmd)
    return lib_out or LIB


if __name__ == "__main__":
    if "--print-flags" in sys.argv:  # --print-flags <source>[:regs], e.g. physics_ll.hip:regs
        src, _, variant = sys.argv[sys.argv.index("--print-flags") + 1].partition(":")
        print(" ".join(compile_flags(src, variant == "regs")))
    else:
        print(build(force="--force" in sys.argv, verbose=True))
