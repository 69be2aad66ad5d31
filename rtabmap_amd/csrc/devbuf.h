// devbuf.h -- growable device / pinned-host buffers (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcd {

// growable device buffer: capacity at least doubles; the first `keep` bytes survive a growth (device-to-device copy on
// `s`, ordered after everything already enqueued there).  The old allocation is freed after the stream drained.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes, size_t keep, hipStream_t s, int64_t* total) {
        if (bytes <= cap) return hipSuccess;
        size_t ncap = cap ? cap * 2 : 256;
        while (ncap < bytes) ncap *= 2;
        void* np = nullptr;
        hipError_t e = hipMalloc(&np, ncap);
        if (e != hipSuccess) return e;
        if (p && keep) {
            e = hipMemcpyAsync(np, p, keep < cap ? keep : cap, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
        }
        if (p) {
            e = hipStreamSynchronize(s);
            if (e != hipSuccess) { (void)hipFree(np); return e; }
            (void)hipFree(p);
        }
        if (total) *total += (int64_t)ncap - (int64_t)cap;
        p = np;
        cap = ncap;
        return hipSuccess;
    }
    void release(int64_t* total) {
        if (p) (void)hipFree(p);
        if (total) *total -= (int64_t)cap;
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return (T*)p; }
};

#define TF_TRY(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return e__; } while (0)

// grow a table, new part filled with `byte`
inline hipError_t grow_filled(DevBuf& buf, size_t bytes, int byte, hipStream_t s, int64_t* total) {
    const size_t old = buf.cap;
    if (bytes <= old) return hipSuccess;
    hipError_t e = buf.reserve(bytes, old, s, total);
    if (e != hipSuccess) return e;
    return hipMemsetAsync((char*)buf.p + old, byte, buf.cap - old, s);
}
inline hipError_t grow_zeroed(DevBuf& buf, size_t bytes, hipStream_t s, int64_t* total) { return grow_filled(buf, bytes, 0, s, total); }

struct PinBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        size_t ncap = cap ? cap * 2 : 4096;
        while (ncap < bytes) ncap *= 2;
        void* np = nullptr;
        hipError_t e = hipHostMalloc(&np, ncap, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        if (p) (void)hipHostFree(p);
        p = np;
        cap = ncap;
        return hipSuccess;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return (T*)p; }
};

}  // namespace lcd
