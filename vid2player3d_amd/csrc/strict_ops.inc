// namespace strict: what the link-per-lane physics step restates of the reference's torch arithmetic, compiled with precise semantics
// and without contraction inside a translation unit that is otherwise built relaxed (-ffp-contract=fast-honor-pragmas and the
// -fassociative-math set, build.py).  Included inside namespace v2p by physics_ll.hip (fused prologue / epilogue of physics_ll_kernel)
// and by physics_ll_host.hip (the stand-alone env_pre_kernel); no include guard.
//
// Pre-physics (humanoid_smpl_im.py:125-157, 391-396): PD-target clamp, residual root wrench rotated into the heading frame.  ONE
// implementation serves both the stand-alone env_pre_kernel and the prologue of the physics kernel, so the fused step equals the
// staged step bit for bit (tests).
namespace strict {
#pragma clang fp reassociate(off) reciprocal(off) contract(off)
#include "v2p_math.inc"
#include "motion_sample.inc"
#include "post_ops.inc"
// sum of 24 consecutive floats, ascending (the order env_post_kernel adds the bodies' reward terms in)
__device__ __forceinline__ float sum_bodies(const float* p) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NB; ++i) s += p[i];
    return s;
}
__device__ __forceinline__ float pd_clamp(float act, float q, float lim) { return fmaxf(fminf(act, q + lim), q - lim); }
// root_rot: rigid-body rotation of the root (xyzw); a3: the three action components of the force (or torque) part
__device__ __forceinline__ V3 residual_wrench(const float* root_rot, float a0, float a1, float a2, float scale) {
    const Q4 hq = ref_heading_quat(ref_calc_heading(ref_remove_base_rot(Q4{root_rot[0], root_rot[1], root_rot[2], root_rot[3]})));
    return ref_quat_rotate(hq, V3{a0 * scale, a1 * scale, a2 * scale});
}
// force and torque at once: one heading quaternion (the same functions of the same arguments: the same bits as two calls)
__device__ __forceinline__ void residual_wrench2(const float* root_rot, const float* a6, float fscale, float tscale, V3& F, V3& T) {
    const Q4 hq = ref_heading_quat(ref_calc_heading(ref_remove_base_rot(Q4{root_rot[0], root_rot[1], root_rot[2], root_rot[3]})));
    F = ref_quat_rotate(hq, V3{a6[0] * fscale, a6[1] * fscale, a6[2] * fscale});
    T = ref_quat_rotate(hq, V3{a6[3] * tscale, a6[4] * tscale, a6[5] * tscale});
}
}  // namespace strict
#if !defined(V2P_LL_STRICT_MATH)
#pragma clang fp reassociate(on) reciprocal(on) contract(fast)  // (a file-scope fp pragma stays in force past the namespace: switch back)
#endif
