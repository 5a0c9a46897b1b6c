// Launcher of the two-hand backhand fix (two_hand_fix.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_two_hand_fix(const v2p_two_hand_fix_cfg& c, int64_t num_tracks, int64_t track_length, const v2p_two_hand_fix_buffers& b, hipStream_t s);
// nullptr, or what is wrong with cfg's tree, body table or arms (a static string)
const char* two_hand_fix_cfg_fault(const v2p_two_hand_fix_cfg& c);

}  // namespace v2p
