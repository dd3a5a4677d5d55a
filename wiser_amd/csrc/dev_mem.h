// Move-only owners of what the engine holds on the device: memory blocks,
// pinned host blocks, streams and events.  The block owner is generic over a
// two-function memory policy and needs no HIP header (WSR_DEV_MEM_NO_HIP:
// only that part, for the CPU check in tests/cpp/dev_mem_check.cc).
#pragma once
#include <cstddef>
#include <utility>

namespace gpu {
struct HipDevice;   // (the default policy, below)
// One block of n elements from P: void* P::allocate(bytes), void P::release(ptr),
// both throwing on failure.  Whatever throws, the buffer is left empty: never
// with a freed pointer, never with a size it does not hold.
template <class T, class P = HipDevice>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    DevBuf t(std::move(o));   // (o is left empty; t frees what this one held)
    std::swap(p_, t.p_);
    std::swap(n_, t.n_);
    return *this;
  }
  ~DevBuf() { drop(); }
  T* get() const { return p_; }
  operator T*() const { return p_; }   // (kernel launches and copies take the buffer as it is)
  size_t size() const { return n_; }   // elements
  size_t bytes() const { return n_ * sizeof(T); }
  void reset() {
    T* p = std::exchange(p_, nullptr);
    n_ = 0;
    if (p) P::release(p);
  }
  void alloc(size_t n) {
    reset();
    p_ = static_cast<T*>(P::allocate(n * sizeof(T)));
    n_ = n;
  }
  // Grow on demand: need > size() frees the block and allocates cap_for_need
  // elements (contents are not kept).  Returns whether it reallocated.
  bool reserve(size_t need, size_t cap_for_need) {
    if (need <= n_) return false;
    alloc(cap_for_need);
    return true;
  }

 private:
  void drop() noexcept { try { reset(); } catch (...) {} }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Buffers that are sized together: all freed, then all allocated with n
// elements each; if anything fails, all of them end up empty.
template <class... B>
void alloc_group(size_t n, B&... b) {
  try {
    (b.reset(), ...);
    (b.alloc(n), ...);
  } catch (...) {
    ((b = B()), ...);
    throw;
  }
}
}  // namespace gpu

#ifndef WSR_DEV_MEM_NO_HIP
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

namespace gpu {
inline void hip_ok(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_OK(expr) gpu::hip_ok((expr), #expr)

struct HipDevice {
  static void* allocate(size_t bytes) { void* p = nullptr; HIP_OK(hipMalloc(&p, bytes)); return p; }
  static void release(void* p) { HIP_OK(hipFree(p)); }
};
struct HipPinned {
  static void* allocate(size_t bytes) { void* p = nullptr; HIP_OK(hipHostMalloc(&p, bytes)); return p; }
  static void release(void* p) { HIP_OK(hipHostFree(p)); }
};
template <class T>
using PinnedBuf = DevBuf<T, HipPinned>;

// A stream or an event: converts to the raw handle, destroyed with its owner
// (no synchronisation, errors ignored).
template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  explicit Handle(H h) : h_(h) {}
  Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept { Handle t(std::move(o)); std::swap(h_, t.h_); return *this; }
  ~Handle() { if (h_) (void)Destroy(h_); }
  operator H() const { return h_; }

 private:
  H h_ = nullptr;
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

inline Stream make_stream(const int* priority = nullptr) {   // non-blocking
  hipStream_t s = nullptr;
  HIP_OK(priority ? hipStreamCreateWithPriority(&s, hipStreamNonBlocking, *priority)
                  : hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return Stream(s);
}
inline Event make_event(bool timing = false) {
  hipEvent_t e = nullptr;
  HIP_OK(timing ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return Event(e);
}
}  // namespace gpu
#endif  // WSR_DEV_MEM_NO_HIP
