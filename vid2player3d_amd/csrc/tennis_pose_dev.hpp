// What the evaluation step (tennis_eval.hip) and the match record (match_record.hip) share: the env's row of `_joint_rot` as
// `_update_state_from_sim` forms it with `_is_train` false (humanoid_smpl_im_mvae.py:813-820).  Moved here from tennis_eval.hip as the
// lines stood - the text of that file's kernel is the same as before (tools/kernel_identity.py).
#pragma once
#include "ref_rotations.hpp"
#include "v2p_internal.hpp"

namespace v2p {

namespace {

constexpr int TE_JOINTS = 24;
constexpr int TE_PACK = 12;  // joints per 64-bit word of the packed joint table, 5 bits each

// quaternion_to_angle_axis of (w, x, y, z) as ref_quat_to_angle_axis states it, with its one arctangent evaluated in double and rounded
// once.  atan2f is correctly rounded in no library, and the device's and a host's differ in the last bits of one result in six; the
// double's rounding is the correctly rounded float for all but one argument in some 2^29, so the record's joint 0 is the same bits
// here and in the numpy statement (ref_rotations.py, wide_atan2).  One value per env and step.  (torch_safe_atan2's shift never
// applies: s >= 1e-3.)
__device__ inline void te_quat_to_angle_axis(const float* q, float* aa) {
    const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    const float s = sqrtf(ref_clamp_min(s2, 1e-6f));
    const float at = q[0] < 0.f ? (float)atan2(-(double)s, -(double)q[0]) : (float)atan2((double)s, (double)q[0]);
    const float two_theta = 2.f * at;
    const float k = s2 > 0.f ? ref_szd(two_theta, s) : 2.f;
    aa[0] = q[1] * k; aa[1] = q[2] * k; aa[2] = q[3] * k;
}

// The 72 floats of env e's `_joint_rot`, written by the lanes of its wave to joint_rot[at * 72 ..]: joint 0 from the root link's
// quaternion, joints 1..23 the DoF positions of body_of_smpl[j] (packed, 5 bits per joint).  `lanes`: the lanes of the wave.
__device__ inline void te_pose_row(const float* rb, const float* dof_state, int64_t e, const uint64_t* body_of_smpl, int lane, int lanes, float* joint_rot, int64_t at) {
    const float q[4] = {rb[6], rb[3], rb[4], rb[5]};  // the root link's (x, y, z, w) read as (w, x, y, z)
    float aa[3];
    te_quat_to_angle_axis(q, aa);
    for (int i = lane; i < TE_JOINTS * 3; i += lanes) {
        const int j = i / 3, ax = i % 3;
        const int body = (int)((j < TE_PACK ? body_of_smpl[0] : body_of_smpl[1]) >> (5 * (j % TE_PACK))) & 31;
        float v = ax == 0 ? aa[0] : (ax == 1 ? aa[1] : aa[2]);
        if (body > 0) v = dof_state[(e * (3 * (TE_JOINTS - 1)) + (body - 1) * 3 + ax) * 2];
        joint_rot[at * (TE_JOINTS * 3) + i] = v;
    }
}

}  // namespace

// (host) `_mujoco_2_smpl` [24] packed for the kernel arguments: a table indexed by the lane would be copied to scratch
inline void te_pack_body_of_smpl(const int32_t* body_of_smpl, uint64_t* packed) {
    for (int w = 0; w < TE_JOINTS / TE_PACK; ++w) {
        packed[w] = 0;
        for (int j = 0; j < TE_PACK; ++j) packed[w] |= (uint64_t)(body_of_smpl[w * TE_PACK + j] & 31) << (5 * j);
    }
}

// (host) is body_of_smpl a permutation of 0..23 with the root first?  Returns the offending joint, -1 when it is.
inline int te_body_of_smpl_fault(const int32_t* body_of_smpl) {
    uint32_t seen = 0;
    for (int s = 0; s < TE_JOINTS; ++s) {
        const int body = body_of_smpl[s];
        if (body < 0 || body >= TE_JOINTS || (seen >> body & 1u) || (s == 0 && body != 0)) return s;
        seen |= 1u << body;
    }
    return -1;
}

}  // namespace v2p
