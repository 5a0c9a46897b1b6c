// Which FORM of each phase an instantiation of physics_ll_kernel runs, in one place.  Several phases of the link-per-lane kernel exist in
// two forms: a later, faster one for the headline instantiation, and the earlier one, kept for the instantiations where the later one
// spilled or missed a bound (TGS, joint limits, racket + ball, the diagnostic kernel, parts of the register build).  The switches are
// pure functions of the build and of the kernel's template flags - no HIP, no globals: a host-only C++ program can include this header
// alone (tests/test_ll_forms.py pins every value).  physics_ll.hip names the struct once (`using F = LlForms<...>`) and reads F::VTAB
// and so on.
#pragma once

namespace v2p {

// the two objects physics_ll.hip is compiled into (build.py)
enum class LlBuild { Lds, Regs };  // default build: 168 VGPRs, three waves per SIMD, LDS parking | register build: 256 VGPRs, two waves per SIMD

template <LlBuild BUILD, bool TGS, bool DIAG, bool BALL, bool LIMITS>
struct LlForms {
    static constexpr bool REGS = BUILD == LlBuild::Regs;

    // (the substep length behind an opaque scalar move, see the head of the substep loop)
    static constexpr bool OPAQUE_H = BALL || LIMITS;  // (the headline instantiation keeps its 0 - 12 B of scratch either way: measured no difference, profiles/r06d_variants_spill.log)

    // FASTARG: the (value, index) reductions of contact generation in two reductions of one value each (grp_arg in physics_ll.hip, FAST).
    // It needs two registers more while it runs, which the racket + ball and joint-limit instantiations do not have (their scratch grew
    // by 8 - 20 B per lane with it): those keep the pairwise form.
    static constexpr bool FASTARG = REGS ? !BALL && !LIMITS && !TGS && !DIAG  // (see grp_arg; the register build spills in its TGS kernels with it)
                                         : !BALL && !LIMITS;

    // VTAB (the kernels without joint limits and TGS): the moves of the sweep's walk filed by VISIT instead of by link (the table is
    // described where it is built, physics_ll.hip).
    // The joint-limit kernels carry moves of their own inside a visit (the one-joint bounce) and keep the earlier form, the TGS
    // kernels with them (as UPMASK below); with the table the ball kernels of the register build need 16 B more scratch per
    // lane and its diagnostic kernel 20 B: they keep the earlier form too (docs/NOTES.md B, 2026-10-19, the sweep's visits).
    static constexpr bool VTAB = REGS ? !LIMITS && !TGS && !BALL && !DIAG
                                      : !LIMITS && !TGS && !BALL;

    // SETUPX (the kernels with the visit table, see VTAB): the depth of each env's deepest touched link is a reduction of the
    // lanes' own depths on the DPP network, and the visit table is formed by the stops' own lanes (where it is built).  The other kernels
    // walk the touched links with a load of the model's depth table per link, and fill the table stop by stop: with the reduction
    // alone, nine of the racket + ball, joint-limit and TGS kernels of the default build need 4 - 16 B more scratch per lane and
    // four of the register build 4 - 8 B (profiles/r21a_kres_*_reduction_in_every_kernel.txt against r21a_kres_*_all_kernels.txt).
    static constexpr bool SETUPX = REGS ? !LIMITS && !TGS && !BALL && !DIAG
                                        : !LIMITS && !TGS && !BALL;

    // LIVEM (with the visit table): whether an env has applied an impulse yet is bit h of ONE scalar word (`livem`), fed by the two
    // halves of the change ballot as two scalars.  As two bools (the earlier form, which the other kernels keep with their visits)
    // the compiler holds `live` in two lane masks, and every visit turns them into a scalar through a VGPR again
    // (docs/NOTES.md B, 2026-10-19, the way down and the rest of the sweep).
    static constexpr bool LIVEM = VTAB;

    // ROWX: the rows of a visit's stops, point by point, without selects and without a dispatch between the points: a point's
    // three rows run as a divergent region of the lanes whose point is active.  ROWCNT (with the visit table): whether point c
    // exists for either stop is a scalar test on the stops' numbers of points, which the visit words carry in bits 25 - 27;
    // without the table it stays a vote.  The register build's kernels without the table keep the earlier form, a vote per point
    // and `dl` selected per row: with the regions its TGS + joint-limit kernel needs 12 B more scratch per lane
    // (docs/NOTES.md B, 2026-10-19, the rows).
    static constexpr bool ROWX = REGS ? VTAB : true;
    static constexpr bool ROWCNT = ROWX && VTAB;

    // UPMASK: whether walk_to runs the way up in its masked form.  The joint-limit and TGS kernels keep the earlier form: with the masked
    // one the joint-limit kernels of the register build need 4 .. 16 B more scratch per lane, and two TGS tests of the racket + ball
    // kernels missed their bounds by 1 % and 5 % - cause not found, see docs/NOTES.md B 2026-10-19
    static constexpr bool UPMASK = !LIMITS && !TGS;

    // LAMX: a level of the Lambda recursion by blocks - Lam.B = P Gb - E Gc, M1 = P Ga - E Gb^T, Lam.A = Di + M1 P - Lam.B E^T with
    // P = aug Di - every entry once, as aug (Di . G) - E . G in seven fused multiply-adds, of the symmetric Lam.A the upper triangle, and
    // the parent's blocks shifted to the link's origin in fused chains as well.  The earlier form went through H1, H2 = Lam.B^T (the
    // same nine entries a second time) and all nine entries of t, averaged: 308 float instructions per level against 210.  It does
    // not keep the earlier form's float32 rounding; every instantiation of both builds runs it: none gains scratch or loses a wave
    // per SIMD with it (docs/NOTES.md B, 2026-10-20, the arithmetic of the level loops).
    static constexpr bool LAMX = true;

    // P2SHIFT: pass 2 shifts cA to the parent's origin through the cB it has just formed, two crosses per entry of the upper triangle
    // instead of t1, t1^T and t2 (274 -> 261 float instructions per level; float32 rounding moves).  The TGS kernels with a ball keep the
    // earlier form: with BOTH new forms one TGS test of the mixed racket + ball batches missed its position bound by 5 % (each form
    // alone stays inside it) - cause not found, docs/NOTES.md B, 2026-10-20, the arithmetic of the level loops
    static constexpr bool P2SHIFT = !(TGS && BALL);

    // CGEN_EARLY (with the visit table): contact generation - the cull, the scan rounds, the records, the touched masks, the depth of each
    // env's deepest stop, sweep_on - runs right behind the kinematics, where the pose is still in registers, instead of between the root
    // solve and the Lambda recursion.  It reads only the pose and constants, so its results are the same bits; what goes is what its
    // earlier place cost: the root's Lambda parked in LDS around it (21 writes, 21 reads), the placeholder fill of the other lanes' Lambda
    // (21 moves) and the re-read of the pose (7 reads).  The joint-limit kernels activate their rows with v*, which exists only after pass
    // 3: they, and with them the TGS and ball kernels, keep the earlier order (docs/NOTES.md B, 2026-10-20, contact generation first).
    static constexpr bool CGEN_EARLY = VTAB;

    // DIAGX: the split of the sweep's remainder (counters CLOSE_MOVE .. SWEEP_SETUP: closing move, closing pass, head and tail of a visit,
    // set-up) is timed in the default build's diagnostic kernel only: in the register build's it costs 12 B of scratch per lane
    static constexpr bool DIAGX = REGS ? false : DIAG;

    // the waves per SIMD that __launch_bounds__ takes (the register budget), from the build's three figures (V2P_LL_WPS*)
    static constexpr int waves_per_simd(int wps, int wps_ball, int wps_limits) { return DIAG ? 2 : (BALL ? wps_ball : (LIMITS ? wps_limits : wps)); }

    static_assert(SETUPX == VTAB, "the set-up in front of the sweep and the table go together");
    static_assert(LIVEM == VTAB, "the scalar live word belongs to the visit table");
    static_assert(ROWCNT == (ROWX && VTAB), "the points are counted from the visit words: no table, no count");
    static_assert(!VTAB || UPMASK, "every kernel with the visit table runs the masked way up");
};

}  // namespace v2p
