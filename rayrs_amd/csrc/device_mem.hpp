// device_mem.hpp -- owners of what the HIP runtime hands out: a device buffer, a pinned host buffer, an event, a
// stream.  Each is move-only and releases in its destructor; the calls that allocate and release live here and nowhere
// else in the host code.  They return the runtime's own status: callers report it with HIP_TRY (scene_internal.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace rayrs {

class DevBuf {
    void* p_ = nullptr;
    size_t bytes_ = 0;
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    ~DevBuf() { if (p_) (void)hipFree(p_); }
    // At least `bytes`: keeps an allocation that is large enough, else frees it and allocates anew.  After a failure
    // the buffer is empty, so that a frame after an out-of-memory error starts clean.
    hipError_t reserve(size_t bytes) {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = p_ ? hipFree(p_) : hipSuccess;
        if (e != hipSuccess) return e;
        p_ = nullptr, bytes_ = 0;
        e = hipMalloc(&p_, bytes);
        if (e == hipSuccess) bytes_ = bytes;
        else p_ = nullptr;
        return e;
    }
    hipError_t upload(const void* src, size_t bytes) {
        const hipError_t e = reserve(bytes);
        return e == hipSuccess && bytes ? hipMemcpy(p_, src, bytes, hipMemcpyHostToDevice) : e;
    }
    hipError_t download(void* dst, size_t bytes) const { return bytes ? hipMemcpy(dst, p_, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
    template <class T = void> T* as() const { return static_cast<T*>(p_); }
};

class PinnedBuf {
    void* p_ = nullptr;
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    hipError_t alloc(size_t bytes) { return hipHostMalloc(&p_, bytes, hipHostMallocDefault); }  // (once, on an empty owner)
    template <class T> T* as() const { return static_cast<T*>(p_); }
};

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    hipError_t create() { return hipEventCreate(&e_); }  // (once, on an empty owner)
    operator hipEvent_t() const { return e_; }
};

class Stream {
    hipStream_t s_ = nullptr;
public:
    Stream() = default;
    Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
    ~Stream() { if (s_) (void)hipStreamDestroy(s_); }
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(&s_, flags); }  // (once, on an empty owner)
    operator hipStream_t() const { return s_; }
};

}  // namespace rayrs
