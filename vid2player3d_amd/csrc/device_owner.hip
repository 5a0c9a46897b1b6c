// DeviceOwner (v2p_internal.hpp): the only place of the library that frees device memory, pinned host memory or events.  Host code only.
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <new>

#include "v2p_internal.hpp"

namespace v2p {

// v2p_debug_guards: bytes of each guard zone of the allocations made from now on, 0 = none (process-wide; read by device_bytes)
static std::atomic<int64_t> guard_zone_bytes{0};

static int checked(hipError_t e, const char* call, const char* name) {
    char what[128];
    snprintf(what, sizeof(what), name ? "%s(%s)" : "%s", call, name);
    return check_hip(e, what);
}

void DeviceOwner::free_item(const Item& it) {
    if (it.kind == DEVICE) (void)hipFree(it.base);
    if (it.kind == PINNED) (void)hipHostFree(it.p);
    if (it.kind == EVENTS) {
        hipEvent_t* ev = (hipEvent_t*)it.p;
        for (size_t i = 0; i < it.count; ++i) (void)hipEventDestroy(ev[i]);
        delete[] ev;
    }
}

DeviceOwner::~DeviceOwner() {
    if (items.empty()) return;
    DeviceGuard g(device);
    for (const Item& it : items) free_item(it);
}

void DeviceOwner::release(const void* p) {
    for (size_t i = items.size(); p && i-- > 0;)
        if (items[i].p == p) {
            DeviceGuard g(device);
            free_item(items[i]);
            if (items[i].kind == DEVICE && items[i].zone) {
                --guarded;
                if (items[i].poisoned) --poisoned;
            }
            items.erase(items.begin() + (ptrdiff_t)i);
            return;
        }
}

int DeviceOwner::device_bytes(void** p, size_t bytes, const char* name, Fill fill, const void* host, bool floating) {
    const size_t zone = (size_t)guard_zone_bytes.load();
    const GuardLayout lay = guard_layout(bytes, zone);  // (zone 0: total = bytes, payload at 0)
    const bool poison = zone && fill == NO_FILL && !host;
    void* base = nullptr;
    int rc = checked(hipMalloc(&base, lay.total), "hipMalloc", name);
    char* q = (char*)base + (base ? lay.payload : 0);
    if (rc == V2P_OK && zone) {
        rc = checked(hipMemset(base, GUARD_BYTE, zone), "hipMemset", name);
        if (rc == V2P_OK) rc = checked(hipMemset((char*)base + lay.back, GUARD_BYTE, zone), "hipMemset", name);
        // poison: see the class comment (floating point 0xff = NaN, everything else 0x00 = what a fresh page holds)
        if (poison) fill = floating ? FILL_FF : FILL_00;
    }
    if (rc == V2P_OK && host) rc = checked(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice), "hipMemcpy", name);
    else if (rc == V2P_OK && fill != NO_FILL) rc = checked(hipMemset(q, fill == FILL_FF ? 0xff : 0, bytes), "hipMemset", name);
    if (rc != V2P_OK) {
        if (base) (void)hipFree(base);
        return rc;
    }
    items.push_back({q, bytes, DEVICE, base, zone, name, poison && floating});
    if (zone) {
        ++guarded;
        if (poison && floating) ++poisoned;
    }
    *p = q;
    return V2P_OK;
}

int DeviceOwner::check_guards(hipStream_t s, std::vector<GuardDamage>* damage) const {
    damage->clear();
    if (!guarded) return V2P_OK;
    DeviceGuard g(device);
    int rc = check_hip(hipStreamSynchronize(s), "hipStreamSynchronize(check_guards)");
    std::vector<unsigned char> host;
    for (size_t i = 0; i < items.size() && rc == V2P_OK; ++i) {
        const Item& it = items[i];
        if (it.kind != DEVICE || !it.zone) continue;
        host.resize(2 * it.zone);
        rc = checked(hipMemcpy(host.data(), it.base, it.zone, hipMemcpyDeviceToHost), "hipMemcpy", it.name);
        if (rc == V2P_OK) rc = checked(hipMemcpy(host.data() + it.zone, (const char*)it.p + it.count, it.zone, hipMemcpyDeviceToHost), "hipMemcpy", it.name);
        if (rc != V2P_OK) break;
        const GuardScan sc = guard_scan(host.data(), host.data() + it.zone, it.zone);
        if (sc.before_count) damage->push_back({it.name, false, sc.before_first, sc.before_count});
        if (sc.behind_count) damage->push_back({it.name, true, sc.behind_first, sc.behind_count});
    }
    return rc;
}

int DeviceOwner::pinned_bytes(void** p, size_t bytes, const char* name) {
    void* q = nullptr;
    const int rc = checked(hipHostMalloc(&q, bytes, hipHostMallocDefault), "hipHostMalloc", name);
    if (rc != V2P_OK) return rc;
    memset(q, 0, bytes);
    items.push_back({q, bytes, PINNED, nullptr, 0, name});
    *p = q;
    return V2P_OK;
}

int DeviceOwner::events(hipEvent_t** ev, size_t count, unsigned flags, const char* name) {
    hipEvent_t* a = new (std::nothrow) hipEvent_t[count]();
    if (!a) { set_error("%s: out of host memory", name ? name : "hipEventCreate"); return V2P_ERR_NOMEM; }
    for (size_t i = 0; i < count; ++i) {
        const int rc = checked(hipEventCreateWithFlags(&a[i], flags), "hipEventCreate", name);
        if (rc != V2P_OK) {
            free_item({a, i, EVENTS, nullptr, 0, name});
            return rc;
        }
    }
    items.push_back({a, count, EVENTS, nullptr, 0, name});
    *ev = a;
    return V2P_OK;
}

// v2p_debug_guards_selftest: known damage, written by the host into the library's own allocation, must be reported exactly
static int guards_selftest(int device) {
    DeviceOwner own;
    own.device = device;
    DeviceGuard g(device);
    if (!g.ok) { set_error("v2p_debug_guards_selftest: cannot select device %d", device); return V2P_ERR_HIP; }
    float *a = nullptr, *c = nullptr;
    int32_t* b = nullptr;
    const size_t na = 100, nb = 7, nc = 64;  // (400 and 28 bytes: the back zones do not begin at a multiple of 256)
    int rc = own.alloc(&a, na, "selftest_a");
    if (rc == V2P_OK) rc = own.alloc(&b, nb, "selftest_b");
    if (rc == V2P_OK) rc = own.alloc(&c, nc, "selftest_c", DeviceOwner::FILL_00);
    if (rc != V2P_OK) return rc;
    const char* bad = nullptr;
    if (own.guarded != 3 || own.poisoned != 1) bad = "three guarded arrays, one of them a poisoned float array, were expected";
    unsigned char ha[na * sizeof(float)], hb[nb * sizeof(int32_t)];
    rc = check_hip(hipMemcpy(ha, a, sizeof(ha), hipMemcpyDeviceToHost), "hipMemcpy(selftest_a)");
    if (rc == V2P_OK) rc = check_hip(hipMemcpy(hb, b, sizeof(hb), hipMemcpyDeviceToHost), "hipMemcpy(selftest_b)");
    if (rc != V2P_OK) return rc;
    for (size_t i = 0; i < sizeof(ha) && !bad; ++i)
        if (ha[i] != 0xff) bad = "the NO_FILL float array is not poisoned with 0xff";
    for (size_t i = 0; i < sizeof(hb) && !bad; ++i)
        if (hb[i] != 0x00) bad = "the NO_FILL integer array is not zero";
    std::vector<DeviceOwner::GuardDamage> d;
    if (rc == V2P_OK) rc = own.check_guards(nullptr, &d);
    if (rc == V2P_OK && !bad && !d.empty()) bad = "fresh zones are reported as damaged";
    // one byte right in front of a's payload, four bytes from the fifth byte behind b's end on
    if (rc == V2P_OK) rc = check_hip(hipMemset((char*)a - 1, 0, 1), "hipMemset(selftest_a)");
    if (rc == V2P_OK) rc = check_hip(hipMemset((char*)b + sizeof(hb) + 4, 0, 4), "hipMemset(selftest_b)");
    if (rc == V2P_OK) rc = own.check_guards(nullptr, &d);
    if (rc != V2P_OK) return rc;
    if (!bad && !(d.size() == 2 && !strcmp(d[0].name, "selftest_a") && !d[0].behind && d[0].first == 1 && d[0].count == 1 &&
                  !strcmp(d[1].name, "selftest_b") && d[1].behind && d[1].first == 4 && d[1].count == 4))
        bad = "the damage written by the host (1 byte before selftest_a, 4 bytes behind selftest_b) is not what check_guards reports";
    if (bad) { set_error("v2p_debug_guards_selftest: %s", bad); return V2P_ERR_INTERNAL; }
    return V2P_OK;
}

}  // namespace v2p

extern "C" {

int v2p_debug_guards(int64_t zone_bytes) {
    if (!v2p::guard_zone_valid(zone_bytes)) {
        v2p::set_error("v2p_debug_guards: %lld bytes: a zone is 0 (off) or a multiple of %lld up to %lld", (long long)zone_bytes, (long long)v2p::GUARD_ALIGN,
                       (long long)v2p::GUARD_MAX_ZONE);
        return V2P_ERR_INVALID;
    }
    return (int)v2p::guard_zone_bytes.exchange(zone_bytes);
}

int v2p_debug_guards_selftest(int device) {
    const int64_t prev = v2p::guard_zone_bytes.exchange(v2p::GUARD_ALIGN);
    const int rc = v2p::guards_selftest(device);
    v2p::guard_zone_bytes.store(prev);
    return rc;
}

}  // extern "C"
