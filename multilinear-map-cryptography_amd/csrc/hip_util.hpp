// hip_util.hpp -- what every translation unit of libtns needs from HIP: the error type and the
// checks that throw it, scoped events and stream ordering, the grow-only device / pinned / mapped
// buffers, and the launch-geometry helpers.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>

#include "../../include/tns.h"

namespace tns {

// A thrown tns::Error carries one of the TNS_* status codes of include/tns.h
// (mirroring TwistAndShoutError, src/lib.rs:59-78) across the C++ layer; the
// C-ABI entry points catch it and store the message for tns_last_error().
struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

void set_last_error(const std::string &msg);

#define TNS_HIP(call)                                                                  \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess)                                                              \
      throw ::tns::Error(TNS_ERR_DEVICE, std::string("HIP error ") + hipGetErrorString(_e) + \
                                             " at " __FILE__ ":" + std::to_string(__LINE__)); \
  } while (0)

#define TNS_LAUNCH_CHECK() TNS_HIP(hipGetLastError())

// A HIP event that lives as long as its scope (ordering only unless flags say otherwise).
struct Event {
  hipEvent_t e = nullptr;
  explicit Event(unsigned flags = hipEventDisableTiming) { TNS_HIP(hipEventCreateWithFlags(&e, flags)); }
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() { (void)hipEventDestroy(e); }
  operator hipEvent_t() const { return e; }
};

// `waiter` runs nothing queued after this call before what is queued on `producer` so far is done
inline void stream_wait(hipStream_t waiter, hipStream_t producer) {
  Event ready;
  TNS_HIP(hipEventRecord(ready, producer));
  TNS_HIP(hipStreamWaitEvent(waiter, ready, 0));
}

// Grow-only device allocation (never shrinks; freed with its owner).  Growing frees the old
// allocation first: a pointer taken from ensure() is good until the next ensure() of more bytes.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }  // (into a cache)
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void *ensure(size_t n) {
    if (n <= bytes && p) return p;
    release();
    size_t want = n ? n : 16;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      p = nullptr;
      throw Error(TNS_ERR_OOM, "hipMalloc of " + std::to_string(want) + " bytes failed: " +
                                   hipGetErrorString(e));
    }
    bytes = want;
    return p;
  }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
};

// Grow-only pinned host buffer (async device-to-host readbacks).
struct PinnedBuf {
  void *p = nullptr;
  size_t bytes = 0;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  void *ensure(size_t n) {
    if (n <= bytes && p) return p;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    hipError_t e = hipHostMalloc(&p, n ? n : 16, hipHostMallocDefault);
    if (e != hipSuccess) throw Error(TNS_ERR_OOM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
    bytes = n ? n : 16;
    return p;
  }
};

// Grow-only fine-grained (coherent, device-mapped) host buffer: a kernel's last workgroup writes
// a small result and a flag here, and the host polls the flag instead of a stream synchronize.
struct MappedHostBuf {
  void *p = nullptr, *dev = nullptr;
  size_t bytes = 0;
  MappedHostBuf() = default;
  MappedHostBuf(const MappedHostBuf &) = delete;
  MappedHostBuf &operator=(const MappedHostBuf &) = delete;
  ~MappedHostBuf() {
    if (p) (void)hipHostFree(p);
  }
  void *ensure(size_t n) {
    if (n <= bytes && p) return p;
    if (p) (void)hipHostFree(p);
    p = dev = nullptr;
    bytes = 0;
    hipError_t e = hipHostMalloc(&p, n ? n : 64, hipHostMallocMapped | hipHostMallocCoherent);
    if (e != hipSuccess) throw Error(TNS_ERR_OOM, std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
    e = hipHostGetDevicePointer(&dev, p, 0);
    if (e != hipSuccess) throw Error(TNS_ERR_DEVICE, std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    std::memset(p, 0, n ? n : 64);
    bytes = n ? n : 64;
    return p;
  }
};

inline unsigned grid_for(size_t work, unsigned block, unsigned max_blocks = 4096) {
  size_t g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > max_blocks) g = max_blocks;
  return (unsigned)g;
}

inline unsigned ilog2_exact(size_t n) {
  unsigned l = 0;
  while (((size_t)1 << l) < n) l++;
  return l;
}

inline size_t next_pow2(size_t n) {  // Rust usize::next_power_of_two (0 -> 1)
  size_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

}  // namespace tns
