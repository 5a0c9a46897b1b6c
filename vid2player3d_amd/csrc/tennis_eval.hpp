// Launcher of the tennis controller's evaluation step (tennis_eval.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_tennis_eval_step(const v2p_tennis_cfg& c, const v2p_tennis_eval_cfg& ec, int64_t n, const v2p_tennis_buffers& b, const v2p_tennis_eval_buffers& x,
                            int64_t frame, hipStream_t s);

}  // namespace v2p
