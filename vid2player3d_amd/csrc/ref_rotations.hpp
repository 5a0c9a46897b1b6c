// The rotation conversions of the reference's utils/konia_transform.py as the task-side kernels restate them: torch elementwise float32
// code, the same operations in the same order (the including files are built without FMA contraction).  The one statement on the device;
// vid2player3d_amd/ref_rotations.py is the numpy one.  The eps rules - 1e-6 shifted into a denominator, theta + 1e-6, a NaN that survives
// clamp_min - are what parity with the reference rests on: change them here or nowhere.
// Included by mvae_player_dev.hpp (mvae_player.hip, mvae_player_dual.hip), mvae_target.hip and, for clamp_min, tennis_task.hip.
//
// Two statements of rotation_matrix_to_quaternion's branch table remain: the one here, which writes the quaternion into an array, and
// mv_rotmat_to_angle_axis of mvae_player_dev.hpp, which keeps it in four locals (and hands it to ref_quat_to_angle_axis like this one).
// The compiler orders x*x + y*y of the sum of squares by which of the two forms it inlined: with this form the four MotionVAE kernels
// differ from what they were in the exchanged sources of one or two v_add_f32, with the locals the two mvae_target kernels do
// (tools/kernel_identity.py; no order of the three squares and no scalar copies of q[] gave both).  The exchanged adds give the same
// bits on the fixtures, but the step's time did not stay inside the bound set for kernels that are not the same machine code
// (docs/NOTES.md, 2026-10-20, rotation conversions), so each file keeps the form its kernels were compiled from.  The third "clamp_min
// as torch evaluates it", tennis_task.hip's, is this one now; its three-argument tt_clamp has one user and stays there.
#pragma once
#include <hip/hip_runtime.h>

namespace v2p {

namespace {

// x.clamp_min(lo) as torch evaluates it: a NaN stays a NaN (fmaxf would drop it)
__device__ inline float ref_clamp_min(float x, float lo) { return x < lo ? lo : x; }
// safe_zero_division (utils/konia_transform.py:336-344)
__device__ inline float ref_szd(float num, float den) {
    if (fabsf(den) < 1e-6f) den += 1e-6f;
    return num / den;
}
// torch_safe_atan2 (:41-49)
__device__ inline float ref_safe_atan2(float y, float x) {
    if (fabsf(y) < 1e-6f && fabsf(x) < 1e-6f) y += 1e-6f;
    return atan2f(y, x);
}

// rotation_matrix_to_quaternion (:347-438): m row-major -> (w, x, y, z), the branch torch.where selects
__device__ inline void ref_rotmat_to_quat(const float* m, float* q) {
    const float m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[3], m11 = m[4], m12 = m[5], m20 = m[6], m21 = m[7], m22 = m[8];
    const float trace = m00 + m11 + m22;
    if (trace > 0.f) {
        const float sq = sqrtf(ref_clamp_min(trace + 1.f, 1e-6f)) * 2.f;
        q[0] = 0.25f * sq; q[1] = ref_szd(m21 - m12, sq); q[2] = ref_szd(m02 - m20, sq); q[3] = ref_szd(m10 - m01, sq);
    } else if (m00 > m11 && m00 > m22) {
        const float sq = sqrtf(ref_clamp_min(1.f + m00 - m11 - m22, 1e-6f)) * 2.f;
        q[0] = ref_szd(m21 - m12, sq); q[1] = 0.25f * sq; q[2] = ref_szd(m01 + m10, sq); q[3] = ref_szd(m02 + m20, sq);
    } else if (m11 > m22) {
        const float sq = sqrtf(ref_clamp_min(1.f + m11 - m00 - m22, 1e-6f)) * 2.f;
        q[0] = ref_szd(m02 - m20, sq); q[1] = ref_szd(m01 + m10, sq); q[2] = 0.25f * sq; q[3] = ref_szd(m12 + m21, sq);
    } else {
        const float sq = sqrtf(ref_clamp_min(1.f + m22 - m00 - m11, 1e-6f)) * 2.f;
        q[0] = ref_szd(m10 - m01, sq); q[1] = ref_szd(m02 + m20, sq); q[2] = ref_szd(m12 + m21, sq); q[3] = 0.25f * sq;
    }
}

// quaternion_to_angle_axis (:557-628) of (w, x, y, z)
__device__ inline void ref_quat_to_angle_axis(const float* q, float* aa) {
    const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const float s = sqrtf(ref_clamp_min(s2, 1e-6f));
    const float two_theta = 2.f * (q[0] < 0.f ? ref_safe_atan2(-s, -q[0]) : ref_safe_atan2(s, q[0]));
    const float k = s2 > 0.f ? ref_szd(two_theta, s) : 2.f;
    aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
}

// rotation_matrix_to_angle_axis (:631-655)
__device__ inline void ref_rotmat_to_angle_axis(const float* m, float* aa) {
    float q[4];
    ref_rotmat_to_quat(m, q);
    ref_quat_to_angle_axis(q, aa);
}

// angle_axis_to_rotation_matrix (:282-333): the Rodrigues form above theta^2 = 1e-6, the first-order form below
__device__ inline void ref_angle_axis_to_rotmat(const float* aa, float* m) {
    const float rx = aa[0], ry = aa[1], rz = aa[2];
    const float theta2 = rx * rx + ry * ry + rz * rz;
    if (theta2 > 1e-6f) {
        const float theta = sqrtf(ref_clamp_min(theta2, 1e-6f));
        const float wx = rx / (theta + 1e-6f), wy = ry / (theta + 1e-6f), wz = rz / (theta + 1e-6f);
        const float c = cosf(theta), s = sinf(theta), t = 1.f - c;
        m[0] = c + wx * wx * t;        m[1] = wx * wy * t - wz * s;   m[2] = wy * s + wx * wz * t;
        m[3] = wz * s + wx * wy * t;   m[4] = c + wy * wy * t;        m[5] = -wx * s + wy * wz * t;
        m[6] = -wy * s + wx * wz * t;  m[7] = wx * s + wy * wz * t;   m[8] = c + wz * wz * t;
    } else {
        m[0] = 1.f; m[1] = -rz; m[2] = ry;
        m[3] = rz;  m[4] = 1.f; m[5] = -rx;
        m[6] = -ry; m[7] = rx;  m[8] = 1.f;
    }
}

}  // namespace

}  // namespace v2p
