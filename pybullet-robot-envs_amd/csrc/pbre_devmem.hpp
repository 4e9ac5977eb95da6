// pbre_devmem.hpp -- move-only owners of the device resources an engine holds: a hipMalloc / hipHostMalloc buffer, an event, a stream.
// An owner releases its handle when it goes out of scope, so an engine that fails half-way through its set-up, and one that is destroyed,
// give back exactly what was made.  An owner converts to the raw handle: that is what kernels, Params and FusedArgs get.
// (tests/host_emu/devmem_test.cpp compiles this header against counting stand-ins of the HIP calls: PBRE_DEVMEM_STUBS)
#pragma once
#ifndef PBRE_DEVMEM_STUBS
#include <hip/hip_runtime_api.h>
#endif

namespace pbre {

template <class H, class Free>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { release(); h = o.h; o.h = nullptr; } return *this; }
    ~Owned() { release(); }
    void release() { if (h) Free()(h); h = nullptr; }
    H* out() { release(); return &h; }      // for the HIP call that makes the handle: hipMalloc(buf.out(), bytes), hipEventCreate(ev.out())
    operator H() const { return h; }
};
struct FreeDevice { void operator()(void* p) const { (void)hipFree(p); } };
struct FreeHost { void operator()(void* p) const { (void)hipHostFree(p); } };
struct FreeEvent { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct FreeStream { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
template <class T> using DevBuf = Owned<T*, FreeDevice>;
template <class T> using HostBuf = Owned<T*, FreeHost>;
using Event = Owned<hipEvent_t, FreeEvent>;
using Stream = Owned<hipStream_t, FreeStream>;

}  // namespace pbre
