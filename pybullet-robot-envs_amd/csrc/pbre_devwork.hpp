// pbre_devwork.hpp -- what a unit that keeps per-ctx work buffers does with the owners of pbre_devmem.hpp: grow one, upload a table once, stage
// a host-synchronous call.  (tests/host_emu/devmem_test.cpp compiles this header too against counting stand-ins of the HIP calls)
#pragma once
#include <cstddef>
#include <vector>
#include "pbre_devmem.hpp"

namespace pbre {

// Makes `buf` hold at least `need` elements; `cap` is what it holds.  Never shrinks.  sync_first: the device is synchronised before the old
// buffer goes, because work in flight on another stream may still use it.  On failure buf is empty and cap 0, so the next call tries again.
template <class T>
inline hipError_t grow(DevBuf<T>& buf, size_t& cap, size_t need, bool sync_first) {
    if (need <= cap) return hipSuccess;
    hipError_t e = sync_first ? hipDeviceSynchronize() : hipSuccess;
    if (e != hipSuccess) return e;
    cap = 0;
    if ((e = hipMalloc(buf.out(), need * sizeof(T))) != hipSuccess) buf.h = nullptr;
    else cap = need;
    return e;
}

// A host table that never changes, into an empty owner; it stays empty if the allocation or the copy fails.
inline hipError_t upload_once(DevBuf<float>& buf, const std::vector<float>& tab) {
    hipError_t e = hipMalloc(buf.out(), tab.size() * sizeof(float));
    if (e != hipSuccess) buf.h = nullptr;
    else if ((e = hipMemcpy(buf, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) buf.release();
    return e;
}

// The host-synchronous variant of a call whose kernels write device buffers: the caller's host arrays get consecutive slices of one
// device block, in the order of add().  A null host pointer is an output not asked for: dev() is null, its bytes stay reserved (pass
// 0 bytes to reserve none).  begin() grows the block and enqueues the uploads (in = true), the caller enqueues its kernels on the
// slices, finish() enqueues the downloads and waits for the stream.  The block is only used between a quiesce and that wait, so it
// grows without a device synchronise.
struct Stage {
    struct Slice { void* host; size_t bytes, off; bool in; } s[8];
    int k = 0;
    size_t total = 0;
    char* base = nullptr;
    int add(const void* host, size_t bytes, bool in = false) { s[k] = {(void*)host, bytes, total, in}; total += bytes; return k++; }
    template <class T> T* dev(int i) const { return s[i].host && s[i].bytes ? (T*)(base + s[i].off) : nullptr; }
    hipError_t copy(bool in, hipStream_t st) const {
        hipError_t e = hipSuccess;
        for (int i = 0; i < k && e == hipSuccess; i++) {
            if (s[i].in != in || !dev<void>(i)) continue;
            e = in ? hipMemcpyAsync(dev<void>(i), s[i].host, s[i].bytes, hipMemcpyHostToDevice, st) : hipMemcpyAsync(s[i].host, dev<void>(i), s[i].bytes, hipMemcpyDeviceToHost, st);
        }
        return e;
    }
    hipError_t begin(DevBuf<char>& buf, size_t& cap, hipStream_t st) {
        const hipError_t e = grow(buf, cap, total > 4 ? total : 4, false);
        base = buf;
        return e == hipSuccess ? copy(true, st) : e;
    }
    hipError_t finish(hipStream_t st) const {
        const hipError_t e = copy(false, st);
        return e == hipSuccess ? hipStreamSynchronize(st) : e;
    }
};

}  // namespace pbre
