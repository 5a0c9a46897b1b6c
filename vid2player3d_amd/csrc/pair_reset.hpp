// Launchers of the two-player controller's pair reset by flags (pair_reset.hip, mvae_player_dual_flagged.hip), called by the C ABI
// (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_ctl_pair_reset_begin(int64_t n, int64_t* flags, const v2p_ctl_reset_buffers& b, int serve_from, hipStream_t s);
int launch_ctl_pair_reset_end(int64_t n, int64_t* flags, hipStream_t s);
int launch_mvae_dual_reset_flagged(const v2p_mvae_cfg (&c)[2], int64_t num_envs, const v2p_mvae_weights (&w)[2], const v2p_mvae_buffers& b, const v2p_mvae_racket& racket,
                                   const int64_t* flags, const float* init_feature, const float* root_xy, const v2p_mvae_root_rule& rule, const float* joint_pos_bind_rel,
                                   hipStream_t s);
int launch_tennis_dual_serve_flagged(int64_t n, const int64_t* flags, int serve_from, const float* racket_pos, float* ball_state, const float* draws,
                                     const v2p_serve_rule& rule, hipStream_t s);

}  // namespace v2p
