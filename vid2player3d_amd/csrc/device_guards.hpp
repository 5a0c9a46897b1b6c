// Guard zones around a device allocation (DeviceOwner, v2p_debug_guards): where the zones and the payload lie inside one allocation,
// and what a host copy of the two zones says about stores outside the payload - pure functions of plain values, no HIP, no globals:
// a host-only C++ program can include this header alone (tests/test_device_guards.py).  What allocates, fills and copies is
// device_owner.hip.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace v2p {

constexpr int64_t GUARD_ALIGN = 256;           // a zone is a multiple of this: the payload keeps hipMalloc's alignment
constexpr int64_t GUARD_MAX_ZONE = 1 << 20;
constexpr unsigned char GUARD_BYTE = 0xff;     // what both zones hold; also the poison of floating-point arrays (all-ones is a NaN)

inline bool guard_zone_valid(int64_t zone) { return zone >= 0 && zone <= GUARD_MAX_ZONE && zone % GUARD_ALIGN == 0; }

// one allocation of `total` bytes: [0, zone) front zone | [payload, payload + bytes) | [back, back + zone) back zone.  The back zone
// begins at the payload's end to the byte (no rounding: a store one element past an odd-sized array must land in it).
struct GuardLayout {
    size_t total, payload, back;
};
inline GuardLayout guard_layout(size_t bytes, size_t zone) { return {zone + bytes + zone, zone, zone + bytes}; }

// What a host copy of the zones shows.  A side is clean when its count is 0.
//   before_*: bytes of the front zone that no longer hold GUARD_BYTE; before_first = distance of the damaged byte NEAREST to the payload
//             from the payload's start (1 = the byte right in front of it)
//   behind_*: the same for the back zone; behind_first = offset of the first damaged byte from the payload's end (0 = the byte right behind it)
struct GuardScan {
    size_t before_count, before_first, behind_count, behind_first;
    bool clean() const { return before_count == 0 && behind_count == 0; }
};
inline GuardScan guard_scan(const unsigned char* front, const unsigned char* back, size_t zone) {
    GuardScan s = {0, 0, 0, 0};
    for (size_t i = 0; i < zone; ++i) {
        if (front[i] != GUARD_BYTE) {
            ++s.before_count;
            s.before_first = zone - i;  // (ascending i: the last hit is the nearest to the payload)
        }
        if (back[i] != GUARD_BYTE && s.behind_count++ == 0) s.behind_first = i;
    }
    return s;
}

}  // namespace v2p
