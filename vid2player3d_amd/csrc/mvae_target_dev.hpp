// What the kernels of the imitation target share: sizes, the launch's argument struct, the quaternion-difference velocity and the levels
// of the chain of transforms.  Included by mvae_target.hip (step, reset by id list, actions) and flag_reset.hip (reset by flags); the
// body of the row kernel itself is text, mvae_target_row.inc.  Two translation units on purpose, as for the motion generator
// (mvae_player_dev.hpp): the kernels of mvae_target.hip must stay the machine code they were (tools/kernel_identity.py).
#pragma once
#include "mvae_target.hpp"
#include "ref_rotations.hpp"

namespace v2p {

namespace {

constexpr int MT_JOINTS = 24;
constexpr int MT_LANES = 32;                      // lanes of an env
constexpr int MT_THREADS = 256;
constexpr int MT_ENVS = MT_THREADS / MT_LANES;    // envs of a workgroup
constexpr int MT_ROW = MSD + 1;                   // floats of a staged row in LDS (odd: the slots' rows start in different banks)
constexpr float MT_PI = 3.14159265358979323846f;

struct MtArgs {
    v2p_mvae_target_cfg c;
    v2p_mvae_target_buffers b;
    const int64_t* env_ids;  // reset only (the reset by flags: the flags [num_envs])
    int64_t n, num_envs;
    int32_t depth[MT_JOINTS];         // level of SMPL joint s (root 0)
    int32_t body_of_smpl[MT_JOINTS];  // the engine's body of SMPL joint s (inverse of smpl_of_body)
    int32_t max_depth;
    int32_t fix_lo, fix_hi;           // the levels that hold a descendant (or self) of Neck or Head: what the head rule's second pass redoes
};

// dof_vel of one body (:915-917): quat_mul_norm(quat_inverse(prev), cur) -> quat_to_angle_axis -> axis * angle / dt; quaternions
// (x, y, z, w), utils/torch_utils.py:14-103 with isaacgym's quat_mul
__device__ inline void mt_quat_diff_velocity(const float* prev, const float* cur, float dt, float* v) {
    const float x1 = -prev[0], y1 = -prev[1], z1 = -prev[2], w1 = prev[3];
    const float x2 = cur[0], y2 = cur[1], z2 = cur[2], w2 = cur[3];
    const float ww = (z1 + x1) * (x2 + y2);
    const float yy = (w1 - y1) * (w2 + z2);
    const float zz = (w1 + y1) * (w2 - z2);
    const float xx = ww + yy + zz;
    const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
    float w = qq - ww + (z1 - y1) * (y2 - z2);
    float x = qq - xx + (x1 + w1) * (x2 + w2);
    float y = qq - yy + (w1 - x1) * (y2 + z2);
    float z = qq - zz + (z1 + y1) * (w2 - x2);
    const float sign = 1.f - 2.f * (w < 0.f ? 1.f : 0.f);  // quat_pos
    x = sign * x; y = sign * y; z = sign * z; w = sign * w;
    const float nrm = ref_clamp_min(sqrtf(x * x + y * y + z * z + w * w), 1e-9f);  // quat_unit
    x = x / nrm; y = y / nrm; z = z / nrm; w = w / nrm;
    // quat_to_angle_axis (:82-103): a NaN of sqrt / acos (w a rounding above 1) fails the mask like the reference's
    const float sin_theta = sqrtf(1.f - w * w);
    float angle = 2.f * acosf(w);
    angle = atan2f(sinf(angle), cosf(angle));  // normalize_angle
    float ax = x / sin_theta, ay = y / sin_theta, az = z / sin_theta;
    if (!(fabsf(sin_theta) > 1e-5f)) { angle = 0.f; ax = 0.f; ay = 0.f; az = 1.f; }
    v[0] = ax * angle / dt; v[1] = ay * angle / dt; v[2] = az * angle / dt;
}

// the levels lo .. hi of batch_rigid_transform (utils/hybrik.py:630-637): a lane of level d multiplies its parent's global transform
// (pulled from the parent's lane `src`) with its own local one, the parent first; R, p: the lane's global transform, in and out
__device__ __forceinline__ void mt_chain(int lo, int hi, int depth, int src, const float* m, const float* rel, float* R, float* p) {
    for (int d = lo; d <= hi; ++d) {
        float PR[9], pp[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) PR[k] = __shfl(R[k], src, MT_LANES);
#pragma unroll
        for (int k = 0; k < 3; ++k) pp[k] = __shfl(p[k], src, MT_LANES);
        if (depth == d) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int q = 0; q < 3; ++q) R[r * 3 + q] = PR[r * 3] * m[q] + PR[r * 3 + 1] * m[3 + q] + PR[r * 3 + 2] * m[6 + q];
                p[r] = PR[r * 3] * rel[0] + PR[r * 3 + 1] * rel[1] + PR[r * 3 + 2] * rel[2] + pp[r];
            }
        }
    }
}

// the levels and the inverse body order of a checked cfg
void fill_args(MtArgs& a, const v2p_mvae_target_cfg& c, const v2p_mvae_target_buffers& b) {
    a = {};
    a.c = c;
    a.b = b;
    bool dirty[MT_JOINTS];
    for (int s = 0; s < MT_JOINTS; ++s) {
        const int par = c.smpl_parents[s];
        a.depth[s] = par < 0 ? 0 : a.depth[par] + 1;  // (parents precede their children)
        a.max_depth = a.depth[s] > a.max_depth ? a.depth[s] : a.max_depth;
        a.body_of_smpl[c.smpl_of_body[s]] = s;
        dirty[s] = s == c.smpl_head || s == c.smpl_neck || (par >= 0 && dirty[par]);
    }
    a.fix_lo = MT_JOINTS;
    a.fix_hi = 0;
    for (int s = 0; s < MT_JOINTS; ++s)
        if (dirty[s] && a.depth[s] > 0) {
            a.fix_lo = a.depth[s] < a.fix_lo ? a.depth[s] : a.fix_lo;
            a.fix_hi = a.depth[s] > a.fix_hi ? a.depth[s] : a.fix_hi;
        }
}

}  // namespace

}  // namespace v2p
