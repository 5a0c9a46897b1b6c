// The humanoid half of the single-player controller's reset, driven by flags (`PhysicsMVAEController._reset_envs`,
// physics_mvae_controller.py:167-199, for the envs whose `reset_buf` is up): every launch runs over envs 0 .. n-1 and an env whose flag
// is 0 keeps every bit.  No id list is read, so the host needs no `nonzero()` of a device result to queue them.  With
// v2p_mvae_reset_flagged (mvae_player_flagged.hip) and v2p_tennis_task_reset (which reads its own two flags) this is the whole reset:
//
//   v2p_ctl_reset_begin              `_reset_env_tensors` without the flags, and `_num_reset += 1`
//   v2p_mvae_reset_flagged           the generator's initial frame
//   v2p_mvae_target_reset_flagged    `_reset_actors` + `_set_env_state`: the pose becomes the previous target and the exposed state
//   v2p_env_push_state_flagged       `_reset_env_tensors` of the wrapped task: the exposed state goes into the engine
//   v2p_tennis_task_reset            the task half
//   v2p_ctl_reset_end                the reaction / recovery flags of the reset envs, then the flag itself
//
// The target's kernel is the text of mvae_target_kernel<true> (mvae_target_row.inc) with the flag in the id's place.  32 lanes share an
// env, two envs a wave64, eight a workgroup, and the text has a workgroup barrier between the staged row and the stores: a slot whose
// env is not flagged runs along (on env 0, storing nothing) exactly like a slot past the end of an id list, so every lane reaches the
// barrier, and the width-32 shuffles of a flagged half-wave read lanes of that half only, all of them active.  A workgroup none of
// whose eight envs is flagged leaves as a whole in front of all that, on a vote that every one of its lanes takes part in: at 1 % of
// envs done that is 92 % of the workgroups.
//
// Built without FMA contraction, like task_ops.hip and mvae_target.hip: the push is env_push_state_kernel's arithmetic.
#include "flag_reset.hpp"
#include "mvae_target_dev.hpp"
#include "v2p_dev.hpp"

namespace v2p {

namespace {

// a.env_ids: the flags [a.n], a.n = a.num_envs
__global__ __launch_bounds__(MT_THREADS) void mvae_target_reset_flagged_kernel(const MtArgs a) {
    constexpr bool RESET = true;
    {
        const int64_t own = (int64_t)blockIdx.x * MT_ENVS + threadIdx.x / MT_LANES;
        const int up = own < a.n && a.env_ids[own] != 0;
        if (!__syncthreads_or(up)) return;  // (the whole workgroup)
    }
#define MT_ROW_ENV(i) (a.env_ids[i] != 0 ? i : (int64_t)-1)
#include "mvae_target_row.inc"
#undef MT_ROW_ENV
}

constexpr int PF_BLOCK = 192;  // 8 envs x 24 bodies = 3 wave64, as env_push_state_kernel
constexpr int PF_ENVS = PF_BLOCK / NB;

// env_push_state_kernel (task_ops.hip) for the flagged envs, indexed by env: thread (e, j) puts body j's part of the exposed
// root_states / dof_state rows of env e into the engine's state
__global__ __launch_bounds__(PF_BLOCK) void env_push_state_flagged_kernel(const float* __restrict__ root_states, const float* __restrict__ dof_state,
                                                                          float* __restrict__ state, const int64_t* __restrict__ flags, int64_t n) {
    const int le = threadIdx.x / NB, j = threadIdx.x % NB;
    const int64_t e = (int64_t)blockIdx.x * PF_ENVS + le;
    if (e >= n) return;
    if (flags[e] == 0) return;
    if (j == 0) {
        const float* r = root_states + e * 13;
        for (int k = 0; k < 3; ++k) state[SIDX(ST_ROOT_POS + k)] = r[k];
        Q4 q = qnormalize(Q4{r[3], r[4], r[5], r[6]});
        state[SIDX(ST_ROOT_QUAT + 0)] = q.x; state[SIDX(ST_ROOT_QUAT + 1)] = q.y;
        state[SIDX(ST_ROOT_QUAT + 2)] = q.z; state[SIDX(ST_ROOT_QUAT + 3)] = q.w;
        for (int k = 0; k < 6; ++k) state[SIDX(ST_VEL + k)] = r[7 + k];
    } else {
        const float* d = dof_state + (e * NDOF + 3 * (j - 1)) * 2;
        Q4 jq = ref_exp_map_to_quat(V3{d[0], d[2], d[4]});
        int base = ST_JQUAT + 4 * (j - 1);
        state[SIDX(base + 0)] = jq.x; state[SIDX(base + 1)] = jq.y; state[SIDX(base + 2)] = jq.z; state[SIDX(base + 3)] = jq.w;
        int vb = ST_VEL + 6 + 3 * (j - 1);
        state[SIDX(vb + 0)] = d[1]; state[SIDX(vb + 1)] = d[3]; state[SIDX(vb + 2)] = d[5];
    }
}

// one thread per env
__global__ __launch_bounds__(256) void ctl_reset_begin_kernel(int64_t n, const int64_t* __restrict__ flags, const v2p_ctl_reset_buffers b) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (flags[e] == 0) return;
    b.progress[e] = 0;
    b.terminate[e] = 0;
    b.num_reset_reaction[e] = 0;
    b.distance[e] = 0.f;
    b.num_reset[e] = b.num_reset[e] + 1;
}

// the flag is the mask AND a buffer that is cleared: it goes last
__global__ __launch_bounds__(256) void ctl_reset_end_kernel(int64_t n, int64_t* __restrict__ flags, const v2p_ctl_reset_buffers b) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    if (flags[e] == 0) return;
    b.reset_reaction[e] = 0;
    b.reset_recovery[e] = 0;
    flags[e] = 0;
}

}  // namespace

int launch_mvae_target_reset_flagged(const v2p_mvae_target_cfg& c, int64_t num_envs, const v2p_mvae_target_buffers& b, const int64_t* flags, hipStream_t s) {
    MtArgs a;
    fill_args(a, c, b);
    a.env_ids = flags;
    a.n = a.num_envs = num_envs;
    hipLaunchKernelGGL(mvae_target_reset_flagged_kernel, dim3((unsigned)((num_envs + MT_ENVS - 1) / MT_ENVS)), dim3(MT_THREADS), 0, s, a);
    return check_hip(hipGetLastError(), "mvae_target_reset_flagged_kernel");
}

int launch_env_push_state_flagged(v2p_env* env, const int64_t* flags, hipStream_t s) {
    if (env->n <= 0) return V2P_OK;
    const unsigned blocks = (unsigned)((env->n + PF_ENVS - 1) / PF_ENVS);
    hipLaunchKernelGGL(env_push_state_flagged_kernel, dim3(blocks), dim3(PF_BLOCK), 0, s, env->buf.root_states, env->buf.dof_state, env->state, flags, env->n);
    return check_hip(hipGetLastError(), "env_push_state_flagged_kernel");
}

int launch_ctl_reset_begin(int64_t n, const int64_t* flags, const v2p_ctl_reset_buffers& b, hipStream_t s) {
    hipLaunchKernelGGL(ctl_reset_begin_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, flags, b);
    return check_hip(hipGetLastError(), "ctl_reset_begin_kernel");
}

int launch_ctl_reset_end(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers& b, hipStream_t s) {
    hipLaunchKernelGGL(ctl_reset_end_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, flags, b);
    return check_hip(hipGetLastError(), "ctl_reset_end_kernel");
}

}  // namespace v2p
