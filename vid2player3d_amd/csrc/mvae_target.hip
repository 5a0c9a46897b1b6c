// The imitation target from the motion generator's pose (vid2player/env/tasks/humanoid_smpl_im_mvae.py): v2p_mvae_target_step is
// `_set_target_motion_state` (:600-661) with the head rule (:605-634) around `_smpl_to_sim` / `_forward_kinematics` (:897-946,
// utils/hybrik.py:598-652), v2p_mvae_target_reset is `_reset_actors` + `_set_env_state` (:463-501) for a list of env ids,
// v2p_mvae_target_actions is `_action_to_pd_targets` (:693-703) before its clamp.
//
// The work of an env is small and tree-shaped: 24 local matrices -> angle-axis, a chain of 3x3 products eight levels deep, 24 global
// matrices -> quaternions, 24 quaternion differences against the previous target.  32 lanes share an env, lane = SMPL joint (lanes
// 24..31 only help with the stores), two envs per wave64, eight per workgroup.  A level of the chain pulls the parent's global
// transform out of the parent's lane with width-32 shuffles; nothing of the chain goes through memory.  The head rule needs the head's
// global transform of a first pass: every lane evaluates the rule on its own transform and the head's result is broadcast; the second
// pass recomputes only the levels that hold a descendant of Neck or Head (two for SMPL).  The packed row (331 floats, rows 4-byte
// aligned) is staged in LDS and written by the env's 32 lanes striding it, as tennis_task.hip writes its observation row.
//
// The arithmetic restates torch elementwise float32 code (built without FMA contraction like tennis_task.hip and mvae_player.hip): the
// same operations in the same order.  The tree and the order of the engine's bodies are the caller's (v2p_mvae_target_cfg); the
// launcher derives the level of every joint and the inverse body order from them.
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
    const int64_t* env_ids;  // reset only
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

// RESET: row i of the launch is env env_ids[i], no head rule, no previous pose; otherwise env i
template <bool RESET>
__global__ __launch_bounds__(MT_THREADS) void mvae_target_kernel(const MtArgs a) {
    __shared__ float s_row[MT_ENVS][MT_ROW];
    const int j = threadIdx.x & (MT_LANES - 1), slot = threadIdx.x / MT_LANES;
    const int64_t i = (int64_t)blockIdx.x * MT_ENVS + slot;
    int64_t e = -1;
    if (i < a.n) e = RESET ? a.env_ids[i] : i;
    // lanes of a slot without an env run along on env 0, for the shuffles and the barrier.  What they read there may be in the middle of
    // being written (env 0's own slot, perhaps in another workgroup, writes Head and Neck back into joint_rotmat): a race by design,
    // harmless because nothing computed from it is stored - every global store below is under `live`
    const bool live = e >= 0 && e < a.num_envs;
    const int64_t er = live ? e : 0;
    const bool joint = j < MT_JOINTS;
    const int jj = joint ? j : 0;
    const v2p_mvae_target_buffers& b = a.b;

    // the lane's place in the tree (a select chain over the launch's uniform tables)
    int parent = -1, depth = 0, body = 0;
#pragma unroll
    for (int k = 0; k < MT_JOINTS; ++k)
        if (k == jj) { parent = a.c.smpl_parents[k]; depth = a.depth[k]; body = a.body_of_smpl[k]; }
    const int src = parent < 0 ? jj : parent;

    int shape = b.env_shape_id ? b.env_shape_id[er] : 0;
    shape = shape < 0 ? 0 : (shape >= a.c.num_shapes ? a.c.num_shapes - 1 : shape);
    const float* bind = b.joint_pos_bind + (size_t)shape * (MT_JOINTS * 3);
    float m[9], rel[3], root[3], bind0[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = b.joint_rotmat[er * (MT_JOINTS * 9) + jj * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        bind0[k] = bind[k];
        rel[k] = bind[jj * 3 + k];
        if (parent >= 0) rel[k] = rel[k] - bind[parent * 3 + k];
        root[k] = b.root_pos[er * 3 + k];
        if (!RESET && b.residual_root) root[k] = root[k] + b.residual_root[er * 3 + k];
    }

    float R[9], p[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = m[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = rel[k];
    mt_chain(1, a.max_depth, depth, src, m, rel, R, p);

    if (!RESET && a.c.fix_head_orientation) {
        // the head rule (:605-634), by every lane on its own transform; the head's lane has the answer
        float q[4];
        ref_rotmat_to_quat(R, q);
        // quaternion_to_rotation_matrix (utils/konia_transform.py:474-549) x (0, 0, 1): the third column's x and y
        const float qn = ref_clamp_min(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
        const float w = q[0] / qn, x = q[1] / qn, y = q[2] / qn, z = q[3] / qn;
        const float tx = 2.f * x, ty = 2.f * y, tz = 2.f * z;
        float l0 = tz * x + ty * w, l1 = tz * y - tx * w;
        const float ln = ref_clamp_min(sqrtf(l0 * l0 + l1 * l1), 1e-12f);
        l0 = l0 / ln; l1 = l1 / ln;
        const float ball_x = b.ball_state[er * 13], ball_y = b.ball_state[er * 13 + 1];
        float h0 = ball_x - (p[0] - (bind0[0] - root[0])), h1 = ball_y - (p[1] - (bind0[1] - root[1]));
        const float hn = ref_clamp_min(sqrtf(h0 * h0 + h1 * h1), 1e-12f);
        h0 = h0 / hn; h1 = h1 / hn;
        float diff = atan2f(h1, h0) - atan2f(l1, l0);
        if (diff > MT_PI) diff = diff - 2.f * MT_PI;
        if (diff < -MT_PI) diff = diff + 2.f * MT_PI;
        const float sim_root_y = b.rb_state[er * (NB * 13) + 1];
        if ((ball_y < sim_root_y - 0.5f) || (fabsf(ball_x) > 4.f)) diff = 0.f;  // no need to correct the head if it is a miss
        diff = __shfl(diff, a.c.smpl_head, MT_LANES);
        if (joint && (j == a.c.smpl_head || j == a.c.smpl_neck)) {
            float aa[3];
            ref_rotmat_to_angle_axis(m, aa);
            aa[1] = aa[1] + diff / 2.f;
            ref_angle_axis_to_rotmat(aa, m);
            if (live) {
#pragma unroll
                for (int k = 0; k < 9; ++k) b.joint_rotmat[e * (MT_JOINTS * 9) + j * 9 + k] = m[k];
            }
        }
        mt_chain(a.fix_lo, a.fix_hi, depth, src, m, rel, R, p);
    }

    // ---- `_smpl_to_sim` of the lane's joint into the staged row, in the engine's body order
    float* row = s_row[slot];
    if (joint) {
        float q[4], aa[3];
        ref_rotmat_to_quat(R, q);
        ref_rotmat_to_angle_axis(m, aa);
        const float cur[4] = {q[1], q[2], q[3], q[0]};
#pragma unroll
        for (int k = 0; k < 4; ++k) row[MS_RB_ROT + 4 * body + k] = cur[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) row[MS_RB_POS + 3 * body + k] = p[k] - (bind0[k] - root[k]);
        float v[3] = {0.f, 0.f, 0.f};
        if (!RESET) {
            float prev[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) prev[k] = b.prev_target[er * MSD + MS_RB_ROT + 4 * body + k];
            mt_quat_diff_velocity(prev, cur, a.c.dt, v);
        }
        if (body > 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row[MS_DOF_POS + 3 * (body - 1) + k] = aa[k];
                row[MS_DOF_VEL + 3 * (body - 1) + k] = v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) row[MS_ROOT_ROT + k] = cur[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                row[MS_ROOT_POS + k] = root[k];
                row[MS_ROOT_VEL + k] = RESET ? 0.f : (root[k] - b.prev_target[er * MSD + MS_ROOT_POS + k]) / a.c.dt;
                row[MS_ROOT_ANG_VEL + k] = v[k] / a.c.dt;  // (divided by dt once more, as the reference has it, :919)
            }
        }
    }
    __syncthreads();
    if (!live) return;

    // ---- the env's 32 lanes stride the row; key_pos is rb_pos of the key bodies
    float* out = b.target + e * MSD;
    for (int col = j; col < MSD; col += MT_LANES) {
        int from = col;
        if (col >= MS_KEY_POS && col < MS_RB_POS) {
            const int k = (col - MS_KEY_POS) / 3;
            const int kb = k == 0 ? a.c.key_bodies[0] : (k == 1 ? a.c.key_bodies[1] : (k == 2 ? a.c.key_bodies[2] : a.c.key_bodies[3]));
            from = MS_RB_POS + 3 * kb + (col - MS_KEY_POS - 3 * k);
        }
        out[col] = row[from];
    }
    if (RESET) {  // `_set_env_state` (:477-490): pose, zero velocities
        if (b.root_states && j < 13) b.root_states[e * 13 + j] = j < 7 ? row[j] : 0.f;  // (root_pos and root_rot open the row)
        if (b.dof_state)
            for (int k = j; k < NDOF * 2; k += MT_LANES) b.dof_state[e * (NDOF * 2) + k] = (k & 1) ? 0.f : row[MS_DOF_POS + (k >> 1)];
        if (b.rb_state)
            for (int k = j; k < NB * 13; k += MT_LANES) {
                const int bd = k / 13, c = k - bd * 13;
                b.rb_state[e * (NB * 13) + k] = c < 3 ? row[MS_RB_POS + 3 * bd + c] : (c < 7 ? row[MS_RB_ROT + 4 * bd + (c - 3)] : 0.f);
            }
    } else if (j == 0) {
        if (b.hold_reset) b.hold_reset[e] = 0;
        if (b.hold_progress) b.hold_progress[e] = 0;
        if (b.hold_cur_time) b.hold_cur_time[e] = 0.f;
    }
}

// one thread per action component
__global__ __launch_bounds__(256) void mvae_target_actions_kernel(const MtArgs a, const float* in, float* out) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= a.n * NACT) return;
    const int64_t e = tid / NACT;
    const int c = (int)(tid - e * NACT);
    out[tid] = mvae_pd_target(a.c, a.b, e, c, in[tid]);
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

int launch_mvae_target_step(const v2p_mvae_target_cfg& c, int64_t n, const v2p_mvae_target_buffers& b, hipStream_t s) {
    MtArgs a;
    fill_args(a, c, b);
    a.n = a.num_envs = n;
    hipLaunchKernelGGL(mvae_target_kernel<false>, dim3((unsigned)((n + MT_ENVS - 1) / MT_ENVS)), dim3(MT_THREADS), 0, s, a);
    return check_hip(hipGetLastError(), "mvae_target_kernel");
}

int launch_mvae_target_reset(const v2p_mvae_target_cfg& c, int64_t num_envs, const v2p_mvae_target_buffers& b, const int64_t* env_ids, int64_t n_ids, hipStream_t s) {
    MtArgs a;
    fill_args(a, c, b);
    a.env_ids = env_ids;
    a.n = n_ids;
    a.num_envs = num_envs;
    hipLaunchKernelGGL(mvae_target_kernel<true>, dim3((unsigned)((n_ids + MT_ENVS - 1) / MT_ENVS)), dim3(MT_THREADS), 0, s, a);
    return check_hip(hipGetLastError(), "mvae_target_reset_kernel");
}

int launch_mvae_target_actions(const v2p_mvae_target_cfg& c, int64_t n, const float* actions_in, const v2p_mvae_target_buffers& b, float* actions_out, hipStream_t s) {
    MtArgs a;
    fill_args(a, c, b);
    a.n = a.num_envs = n;
    hipLaunchKernelGGL(mvae_target_actions_kernel, dim3((unsigned)((n * NACT + 255) / 256)), dim3(256), 0, s, a, actions_in, actions_out);
    return check_hip(hipGetLastError(), "mvae_target_actions_kernel");
}

}  // namespace v2p
