// Launchers of the match record (match_record.hip), called by the C ABI (capi.hip).
#pragma once
#include "v2p_internal.hpp"

namespace v2p {

int launch_match_record_frame(const v2p_match_record_cfg& c, int64_t n, const v2p_match_record_buffers& b, hipStream_t s);
int launch_match_record_select(const v2p_match_record_cfg& c, int64_t n, const v2p_match_record_buffers& b, hipStream_t s);
// -1, or the SMPL joint at which cfg.body_of_smpl stops being a permutation of 0..23 with the root first
int match_record_body_fault(const v2p_match_record_cfg& c);

}  // namespace v2p
