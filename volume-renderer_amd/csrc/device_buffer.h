// device_buffer.h -- owners of what RendererCore allocates through HIP: device memory, pinned host memory, events.  An empty
// owner never calls into HIP (a host-only handle, device < 0, makes no HIP call ever); the destructors and reset() ignore the
// status of the release (a failing hipFree means an earlier sticky error, which the next HIP call reports).
#pragma once
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <utility>

namespace vr {

struct HipError : std::runtime_error {
    hipError_t code;
    HipError(hipError_t c, const std::string &what) : std::runtime_error(what), code(c) {}
};
struct DeviceMemoryError : HipError { using HipError::HipError; };   // a device allocation a call cannot do without failed (VR_E_NOMEM)
inline void hipCheck(hipError_t e, const std::string &what) { if (e != hipSuccess) throw HipError(e, what + ": " + hipGetErrorString(e)); }

// `size()` elements of T in device memory (raw bytes: T = uint8_t); move-only.  Every allocating call frees the earlier
// allocation first and leaves the buffer empty when it fails; hipFree waits for the kernels that use the memory.
template <class T>
class DeviceBuffer {
public:
    DeviceBuffer() = default;
    DeviceBuffer(size_t n, const std::string &what) { alloc(n, what); }
    DeviceBuffer(DeviceBuffer &&o) noexcept { swap(o); }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DeviceBuffer() { reset(); }
    void swap(DeviceBuffer &o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    T *release() { T *p = p_; p_ = nullptr; n_ = 0; return p; }
    bool tryAlloc(size_t n) { if (raw(n) == hipSuccess) return true; (void)hipGetLastError(); return false; }   // the optional copies: no memory is no error
    void alloc(size_t n, const std::string &what) { hipCheck(raw(n), "hipMalloc(" + what + ")"); }
    void allocOrNoMemory(size_t n, const std::string &what) { if (!tryAlloc(n)) throw DeviceMemoryError(hipErrorOutOfMemory, what + " failed"); }
    bool ensure(size_t n, const std::string &what) { if (n <= n_) return false; alloc(n, what); return true; }   // grow only; true: a new allocation

private:
    hipError_t raw(size_t n) { reset(); const hipError_t e = hipMalloc(reinterpret_cast<void **>(&p_), n * sizeof(T)); if (e == hipSuccess) n_ = n; else p_ = nullptr; return e; }
    T *p_ = nullptr;
    size_t n_ = 0;
};

class PinnedBuffer {                          // pinned host bytes (presentRGBA8's frames)
public:
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    PinnedBuffer &operator=(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { reset(); }
    uint8_t *get() const { return static_cast<uint8_t *>(p_); }
    void reset() { if (p_) (void)hipHostFree(p_); p_ = nullptr; }
    void alloc(size_t bytes, const char *what) { reset(); const hipError_t e = hipHostMalloc(&p_, bytes, hipHostMallocDefault); if (e != hipSuccess) p_ = nullptr; hipCheck(e, what); }

private:
    void *p_ = nullptr;
};

class Event {
public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { reset(); }
    operator hipEvent_t() const { return e_; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    void create(unsigned flags = hipEventDefault) { reset(); const hipError_t e = hipEventCreateWithFlags(&e_, flags); if (e != hipSuccess) e_ = nullptr; hipCheck(e, "hipEventCreate"); }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace vr
