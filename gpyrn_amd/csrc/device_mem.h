// Device and pinned memory of libgprn_hip.so: ONE allocator and the two owners everything goes through.  Free of gprn_ctx and of
// HIP (tests/device_mem_check.cpp runs it over malloc): an error is a return code plus a message.
#pragma once
#include <stddef.h>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/gprn_hip.h"

// The raw functions, defined ONCE (api.hip: the only place that names the four HIP calls).  A failed device allocation returns
// GPRN_E_NOMEM and is not sticky (the batch drivers allocate again, in halves), a failed pinned one GPRN_E_HIP; both leave *p
// null and the reason in *err.  The counters: allocations live now / made since load (options "live_allocs", "allocs_made").
int mem_dev_alloc(void** p, size_t bytes, std::string* err);
void mem_dev_free(void* p);
int mem_pin_alloc(void** p, size_t bytes, std::string* err);
void mem_pin_free(void* p);
extern std::atomic<long long> g_mem_live, g_mem_made;

template <typename T>
static int mem_alloc(T** p, size_t count, bool pinned, std::string* err)       // (a zero count: one element)
{
    *p = nullptr;
    const size_t bytes = (count ? count : 1) * sizeof(T);
    return pinned ? mem_pin_alloc((void**)p, bytes, err) : mem_dev_alloc((void**)p, bytes, err);
}

// Owns device and pinned allocations: everything it hands out is freed in release() and in its destructor, on every path
// (CallScratch for one call; SmallBatchMem, MidBatch and through them batch_tail.hip's TailKept between side-by-side calls; the
// lifetime groups of gprn_ctx).  A failed alloc / pin leaves a null pointer.  c: whatever has the `err` the message goes to.
struct DeviceOwner {
    std::vector<void*> dev, pinned;
    DeviceOwner() = default;
    DeviceOwner(const DeviceOwner&) = delete; DeviceOwner& operator=(const DeviceOwner&) = delete;
    ~DeviceOwner() { release(); }
    template <typename T>
    int alloc(T** p, size_t count, std::string* err) { const int rc = mem_alloc(p, count, false, err); if (!rc) dev.push_back(*p); return rc; }
    template <typename T>
    int pin(T** p, size_t bytes, std::string* err) { const int rc = mem_alloc((char**)p, bytes, true, err); if (!rc) pinned.push_back(*p); return rc; }
    template <class Ctx, typename T> int alloc(Ctx* c, T** p, size_t count) { return alloc(p, count, &c->err); }
    template <class Ctx, typename T> int pin(Ctx* c, T** p, size_t bytes) { return pin(p, bytes, &c->err); }
    bool empty() const { return dev.empty() && pinned.empty(); }
    void release() { for (void* p : dev) mem_dev_free(p); for (void* p : pinned) mem_pin_free(p); dev.clear(); pinned.clear(); }
};

// ONE buffer that only grows: ensure(count) keeps it when it holds that many elements, else frees it and allocates anew (the
// contents are not carried over); a grow that fails leaves it empty -- null, capacity 0 -- and usable again.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                   // elements
    const bool pinned;
    explicit DevBuf(bool pinned_ = false) : pinned(pinned_) {}
    DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t count, std::string* err)
    {
        if (count <= cap) return GPRN_OK;
        release();
        const int rc = mem_alloc(&p, count, pinned, err);
        if (!rc) cap = count;
        return rc;
    }
    void release() { if (pinned) mem_pin_free(p); else mem_dev_free(p); p = nullptr; cap = 0; }
};
