// Launcher of the action part of the tennis controller's pre_physics_step (controller_actions.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_controller_actions(const v2p_controller_actions_cfg& c, int64_t n, const v2p_controller_actions_buffers& b, hipStream_t s);

}  // namespace v2p
