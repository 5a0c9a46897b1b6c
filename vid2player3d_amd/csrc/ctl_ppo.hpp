// Launchers of the tennis controller's PPO agent kernels (ctl_ppo.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

constexpr int CTL_PPO_MAX_ACTIONS = 128;      // two columns per lane of a wave64
constexpr int CTL_PPO_MAX_SUB_REWARDS = V2P_CTL_MAX_SUB_REWARDS;

int launch_ctl_policy_head(int64_t n, int32_t num_actions, const float* mu, const float* logstd, const float* sigma, const float* noise, float clip_actions,
                           float* actions_row, float* mus_row, float* sigmas_row, float* neglogp_row, float* actions_clamped, hipStream_t s);
int launch_ctl_rollout_record(int64_t n, int64_t obs_dim, int32_t num_sub, float clip_obs, const float* obs, const float* rew, const int64_t* reset,
                              const int64_t* terminate, const float* sub_rewards, float* next_obs_row, float* rewards_row, float* dones_row, float* terminated,
                              float* cur_rewards, float* cur_lengths, double* acc, double* sub_acc, hipStream_t s);
int launch_ppo_loss(const v2p_ppo_loss_cfg& c, int64_t rows, const v2p_ppo_loss_buffers& b, hipStream_t s);

}  // namespace v2p
