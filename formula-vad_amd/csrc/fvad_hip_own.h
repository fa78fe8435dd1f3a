// Move-only owners of what the host code creates through HIP: device memory,
// pinned host memory, events and streams.  Each is a std::unique_ptr with a
// deleter; kernels and HIP calls take the raw handle through .get().  The
// make_* helpers return an FVAD_* status through fvad::set_error and leave
// the owner untouched when they fail.  Host code only (no .hip file includes
// this).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <string>

#include "../../include/fvad.h"

namespace fvad {

int set_error(int code, const std::string &msg);  // fvad_last_error()'s message; returns code

struct DevFree {
  void operator()(void *p) const { (void)hipFree(p); }
};
struct PinnedFree {
  void operator()(void *p) const { (void)hipHostFree(p); }
};
struct EventDestroy {
  void operator()(ihipEvent_t *e) const { (void)hipEventDestroy(e); }
};
struct StreamDestroy {
  void operator()(ihipStream_t *s) const { (void)hipStreamDestroy(s); }
};
template <typename T>
using dev_ptr = std::unique_ptr<T, DevFree>;
template <typename T>
using pinned_ptr = std::unique_ptr<T, PinnedFree>;
using event_ptr = std::unique_ptr<ihipEvent_t, EventDestroy>;
using stream_ptr = std::unique_ptr<ihipStream_t, StreamDestroy>;

// count elements of T in device memory (count 0 allocates 1)
template <typename T>
int make_dev(dev_ptr<T> &p, size_t count) {
  void *q = nullptr;
  const hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
  if (e != hipSuccess) return set_error(FVAD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  p.reset(static_cast<T *>(q));
  return FVAD_OK;
}

template <typename T>
int make_pinned(pinned_ptr<T> &p, size_t count) {
  void *q = nullptr;
  const hipError_t e = hipHostMalloc(&q, (count ? count : 1) * sizeof(T), hipHostMallocDefault);
  if (e != hipSuccess) return set_error(FVAD_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
  p.reset(static_cast<T *>(q));
  return FVAD_OK;
}

// timing: the event can be an end of hipEventElapsedTime; the others only order streams
inline int make_event(event_ptr &ev, bool timing = false) {
  hipEvent_t q = nullptr;
  const hipError_t e = timing ? hipEventCreate(&q) : hipEventCreateWithFlags(&q, hipEventDisableTiming);
  if (e != hipSuccess) return set_error(FVAD_EDEVICE, std::string("hipEventCreate: ") + hipGetErrorString(e));
  ev.reset(q);
  return FVAD_OK;
}

// hipStreamNonBlocking: the synchronous null-stream copies of setup calls
// never wait for what is queued on it
inline int make_stream(stream_ptr &s, unsigned flags = hipStreamNonBlocking) {
  hipStream_t q = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&q, flags);
  if (e != hipSuccess) return set_error(FVAD_EDEVICE, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  s.reset(q);
  return FVAD_OK;
}

}  // namespace fvad
