// fdnn_stream_order.hpp -- what the objects that own ONE set of device buffers share (the float net, the half net, the
// report: fdnn_float_api.cpp, fdnn_half_api.cpp): the order between the streams they are called on, and the device check of
// their constructors.
#pragma once
#include "fdnn_internal.hpp"

namespace fdnn {

// One set of buffers serves every call of an object: a call on another stream waits (on the device) for the one before.
struct StreamOrder {
  hipEvent_t ev = nullptr;
  hipStream_t last = nullptr;
  bool valid = false;
  ~StreamOrder() {
    if (ev) hipEventDestroy(ev);
  }
  hipError_t enter(hipStream_t s) {
    if (!ev) {
      hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
      if (e != hipSuccess) return e;
    }
    return valid && last != s ? hipStreamWaitEvent(s, ev, 0) : hipSuccess;
  }
  hipError_t leave(hipStream_t s) {
    last = s;
    valid = true;
    return hipEventRecord(ev, s);
  }
};

inline int device_ok(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(FDNN_E_DEVICE, "no HIP device available: this library has no CPU path");
  if (device < 0 || device >= count) return fail(FDNN_E_ARG, "device index out of range");
  return FDNN_OK;
}

}  // namespace fdnn
