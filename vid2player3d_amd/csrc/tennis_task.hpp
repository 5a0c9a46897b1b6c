// Launchers of the tennis controller's task step (tennis_task.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_tennis_task_step(const v2p_tennis_cfg& c, int64_t n, const v2p_tennis_buffers& b, hipStream_t s);
int launch_tennis_task_obs(const v2p_tennis_cfg& c, int64_t num_envs, const v2p_tennis_buffers& b, const int64_t* env_ids, int64_t n_ids, hipStream_t s);
// the two-player batch: the task step with the dual reset law, and the ball hand-over of all pairs (n even)
int launch_tennis_dual_step(const v2p_tennis_cfg& c, const v2p_tennis_dual_cfg& dc, int64_t n, const v2p_tennis_buffers& b, hipStream_t s);
int launch_tennis_dual_handover(const v2p_tennis_cfg& c, const v2p_tennis_dual_cfg& dc, int64_t n, const v2p_tennis_buffers& b,
                                const v2p_tennis_dual_buffers& db, hipStream_t s);

}  // namespace v2p
