// DeviceOwner (v2p_internal.hpp): the only place of the library that frees device memory, pinned host memory or events.  Host code only.
#include <stdio.h>
#include <string.h>

#include <new>

#include "v2p_internal.hpp"

namespace v2p {

static int checked(hipError_t e, const char* call, const char* name) {
    char what[128];
    snprintf(what, sizeof(what), name ? "%s(%s)" : "%s", call, name);
    return check_hip(e, what);
}

void DeviceOwner::free_item(const Item& it) {
    if (it.kind == DEVICE) (void)hipFree(it.p);
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
            items.erase(items.begin() + (ptrdiff_t)i);
            return;
        }
}

int DeviceOwner::device_bytes(void** p, size_t bytes, const char* name, Fill fill, const void* host) {
    void* q = nullptr;
    int rc = checked(hipMalloc(&q, bytes), "hipMalloc", name);
    if (rc == V2P_OK && host) rc = checked(hipMemcpy(q, host, bytes, hipMemcpyHostToDevice), "hipMemcpy", name);
    else if (rc == V2P_OK && fill != NO_FILL) rc = checked(hipMemset(q, fill == FILL_FF ? 0xff : 0, bytes), "hipMemset", name);
    if (rc != V2P_OK) {
        if (q) (void)hipFree(q);
        return rc;
    }
    items.push_back({q, bytes, DEVICE});
    *p = q;
    return V2P_OK;
}

int DeviceOwner::pinned_bytes(void** p, size_t bytes, const char* name) {
    void* q = nullptr;
    const int rc = checked(hipHostMalloc(&q, bytes, hipHostMallocDefault), "hipHostMalloc", name);
    if (rc != V2P_OK) return rc;
    memset(q, 0, bytes);
    items.push_back({q, bytes, PINNED});
    *p = q;
    return V2P_OK;
}

int DeviceOwner::events(hipEvent_t** ev, size_t count, unsigned flags, const char* name) {
    hipEvent_t* a = new (std::nothrow) hipEvent_t[count]();
    if (!a) { set_error("%s: out of host memory", name ? name : "hipEventCreate"); return V2P_ERR_NOMEM; }
    for (size_t i = 0; i < count; ++i) {
        const int rc = checked(hipEventCreateWithFlags(&a[i], flags), "hipEventCreate", name);
        if (rc != V2P_OK) {
            free_item({a, i, EVENTS});
            return rc;
        }
    }
    items.push_back({a, count, EVENTS});
    *ev = a;
    return V2P_OK;
}

}  // namespace v2p
