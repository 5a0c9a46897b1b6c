// Launchers of the imitation target from the motion generator's pose (mvae_target.hip), called by the C ABI (there too).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_mvae_target_step(const v2p_mvae_target_cfg& c, int64_t n, const v2p_mvae_target_buffers& b, hipStream_t s);
int launch_mvae_target_reset(const v2p_mvae_target_cfg& c, int64_t num_envs, const v2p_mvae_target_buffers& b, const int64_t* env_ids, int64_t n_ids, hipStream_t s);
int launch_mvae_target_actions(const v2p_mvae_target_cfg& c, int64_t n, const float* actions_in, const v2p_mvae_target_buffers& b, float* actions_out, hipStream_t s);

}  // namespace v2p
