// Launchers of the imitation target from the motion generator's pose (mvae_target.hip), called by the C ABI (there too).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_mvae_target_step(const v2p_mvae_target_cfg& c, int64_t n, const v2p_mvae_target_buffers& b, hipStream_t s);
int launch_mvae_target_reset(const v2p_mvae_target_cfg& c, int64_t num_envs, const v2p_mvae_target_buffers& b, const int64_t* env_ids, int64_t n_ids, hipStream_t s);
int launch_mvae_target_actions(const v2p_mvae_target_cfg& c, int64_t n, const float* actions_in, const v2p_mvae_target_buffers& b, float* actions_out, hipStream_t s);

// `_action_to_pd_targets` (:693-703) before its clamp, component c of env e's action v: what mvae_target_actions_kernel and
// ll_policy_actions_kernel (policy_io.hip) both write
__device__ __forceinline__ float mvae_pd_target(const v2p_mvae_target_cfg& c, const v2p_mvae_target_buffers& b, int64_t e, int col, float v) {
    if (col < NDOF) {
        float base;
        if (c.pd_target_base == V2P_PD_BASE_TARGET_POS) base = b.target[e * MSD + MS_DOF_POS + col];
        else if (c.pd_target_base == V2P_PD_BASE_CURRENT_POS) base = b.dof_state[(e * NDOF + col) * 2];
        else base = b.pd_action_offset[col];
        v = c.no_scale_action ? base + v : base + b.pd_action_scale[col] * v;
    }
    return v;
}

}  // namespace v2p
