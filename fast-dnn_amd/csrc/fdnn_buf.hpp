// fdnn_buf.hpp -- the one place that allocates and frees device and pinned host memory.  Every buffer of the library is a
// member or a local of this owner type: what a struct declares goes with the struct, and a HIP_TRY that returns early
// frees the locals behind it.  One allocation per buffer (no arena).  A destructor runs on the device that is current:
// whoever deletes a model or a context sets it first (DeviceGuard in destroy_ctx, fdnn_model_free), the buffers do not.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <utility>

namespace fdnn {

// Device memory (kDevice), pinned host memory, or host memory the device reads and writes in place (kMapped: p on the
// host, dev its device alias).  reserve() grows it, the owner's end frees it; converts to T *, like the pointer it replaces.
template <class T, bool kDevice = false, bool kMapped = false>
struct Buf {
  T *p = nullptr;
  T *dev = nullptr;       // kMapped only
  size_t count = 0;       // elements
  bool pageable = false;  // from malloc: pinned memory was refused (reserve(n, true))
  Buf() = default;
  Buf(const Buf &) = delete;
  ~Buf() { release(); }
  operator T *() const { return p; }
  void swap(Buf &o) { std::swap(p, o.p); std::swap(dev, o.dev); std::swap(count, o.count); std::swap(pageable, o.pageable); }
  void release() {
    if (p && pageable) std::free(p);
    else if (p && kDevice) hipFree(p);
    else if (p) hipHostFree(p);
    p = dev = nullptr;
    count = 0, pageable = false;
  }
  // Room for n elements: a buffer that is too small is freed, then allocated anew.  pageable_ok: where pinned memory is
  // refused, malloc serves (the error is cleared; the copy to the device is then a synchronous one).  Whether a refusal
  // matters otherwise is the caller's rule: the buffer stays null.
  hipError_t reserve(size_t n, bool pageable_ok = false) {
    if (n <= count) return hipSuccess;
    release();
    hipError_t e = kDevice ? hipMalloc(reinterpret_cast<void **>(&p), sizeof(T) * n)
                           : hipHostMalloc(reinterpret_cast<void **>(&p), sizeof(T) * n, kMapped ? hipHostMallocMapped : hipHostMallocDefault);
    if (e == hipSuccess && kMapped && (e = hipHostGetDevicePointer(reinterpret_cast<void **>(&dev), p, 0)) != hipSuccess) hipHostFree(p);
    if (e != hipSuccess && pageable_ok) {
      (void)hipGetLastError();
      pageable = (p = static_cast<T *>(std::malloc(sizeof(T) * n))) != nullptr;
      e = p ? hipSuccess : hipErrorOutOfMemory;
    }
    if (e != hipSuccess) p = dev = nullptr;
    count = p ? n : 0;
    return e;
  }
  // Every byte to `byte`, ordered on the NULL stream: returns before it has run (see the wait at the end of make_ctx).
  hipError_t fill(int byte) { return hipMemset(p, byte, sizeof(T) * count); }
};
template <class T> using DevBuf = Buf<T, true>;
template <class T> using Mapped = Buf<T, false, true>;

}  // namespace fdnn
