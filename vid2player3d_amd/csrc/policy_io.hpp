// Launchers of what stands around the policy networks' dense layers (policy_io.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

constexpr int POLICY_LL_OBS = 734;  // columns of the low-level policy's observation

int launch_policy_input(const v2p_policy_input_cfg& c, int64_t n, int64_t dim, const float* obs, float* x, hipStream_t s);
int launch_ll_policy_input(const v2p_policy_input_cfg& c, int64_t n, const v2p_ll_policy_src& src, float* raw_obs, float* x, hipStream_t s);
int launch_ll_policy_actions(const v2p_mvae_target_cfg& c, int64_t n, int32_t sides, float clip_actions, const float* mu, const v2p_mvae_target_buffers& b,
                             float* actions_out, hipStream_t s);

}  // namespace v2p
