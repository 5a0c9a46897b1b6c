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
//
// Where the text is.  Sizes, MtArgs, the quaternion difference and the chain's levels: mvae_target_dev.hpp.  The body of the row kernel:
// mvae_target_row.inc, as text, shared with the reset by flags of flag_reset.hip (v2p_mvae_target_reset_flagged) - see there why text.
#include "mvae_target_dev.hpp"

namespace v2p {

namespace {

// RESET: row i of the launch is env env_ids[i], no head rule, no previous pose; otherwise env i
template <bool RESET>
__global__ __launch_bounds__(MT_THREADS) void mvae_target_kernel(const MtArgs a) {
#define MT_ROW_ENV(i) (RESET ? a.env_ids[i] : i)
#include "mvae_target_row.inc"
#undef MT_ROW_ENV
}

// one thread per action component
__global__ __launch_bounds__(256) void mvae_target_actions_kernel(const MtArgs a, const float* in, float* out) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (tid >= a.n * NACT) return;
    const int64_t e = tid / NACT;
    const int c = (int)(tid - e * NACT);
    out[tid] = mvae_pd_target(a.c, a.b, e, c, in[tid]);
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
