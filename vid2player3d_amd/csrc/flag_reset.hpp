// Launchers of the controller's reset by flags (flag_reset.hip, mvae_player_flagged.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_mvae_reset_flagged(const v2p_mvae_cfg& c, int64_t num_envs, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const int64_t* flags,
                              const float* init_feature, const float* root_xy, const v2p_mvae_root_rule& rule, const float* joint_pos_bind_rel, hipStream_t s);
int launch_mvae_target_reset_flagged(const v2p_mvae_target_cfg& c, int64_t num_envs, const v2p_mvae_target_buffers& b, const int64_t* flags, hipStream_t s);
int launch_env_push_state_flagged(v2p_env* e, const int64_t* flags, hipStream_t s);
int launch_ctl_reset_begin(int64_t n, const int64_t* flags, const v2p_ctl_reset_buffers& b, hipStream_t s);
int launch_ctl_reset_end(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers& b, hipStream_t s);

}  // namespace v2p
