// Launchers of the MotionVAE motion generator (mvae_player.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_mvae_step(const v2p_mvae_cfg& c, int64_t n, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const float* latents, const float* residual,
                     hipStream_t s);
int launch_mvae_reset(const v2p_mvae_cfg& c, int64_t num_envs, const v2p_mvae_weights& w, const v2p_mvae_buffers& b, const int64_t* env_ids, int64_t n_ids,
                      const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, hipStream_t s);
// the two-player forms: c and w hold side 0 (envs 2k) and side 1 (envs 2k+1)
int launch_mvae_dual_step(const v2p_mvae_cfg (&c)[2], int64_t n, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const float* latents, const float* residual,
                          int mapping, hipStream_t s);
int launch_mvae_dual_reset(const v2p_mvae_cfg (&c)[2], int64_t num_envs, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const v2p_mvae_racket& racket,
                           const int64_t* env_ids, int64_t n_ids, const float* init_feature, const float* root_xy, const float* joint_pos_bind_rel, int64_t bind_rows,
                           hipStream_t s);

}  // namespace v2p
