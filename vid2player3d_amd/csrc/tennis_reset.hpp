// Launcher of the single-player controller's flag-driven task reset (tennis_reset.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_tennis_task_reset(const v2p_tennis_cfg& c, const v2p_tennis_reset_cfg& rc, int64_t n, const v2p_tennis_buffers& b, const v2p_tennis_reset_buffers& r,
                             hipStream_t s);

}  // namespace v2p
