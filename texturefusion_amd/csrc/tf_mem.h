// tf_mem.h -- who owns device and pinned memory: the only place in csrc/ that allocates or frees either.  Host only.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../include/tf_fusion.h"

namespace tf {

void set_error(const std::string& msg);

// Move-only owner of one allocation: the pointer and its byte count change together, the destructor frees.  Empty (null,
// 0 bytes) until alloc succeeds and again after it fails.  DevMem lives on the current device, PinMem in pinned host memory.
struct DevMem {
  void* p = nullptr;
  size_t bytes = 0;
  DevMem() = default;
  DevMem(DevMem&& o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned) { o.p = nullptr; o.bytes = 0; }
  DevMem& operator=(DevMem&& o) noexcept {
    if (this != &o) { release(); p = o.p; bytes = o.bytes; pinned = o.pinned; o.p = nullptr; o.bytes = 0; }
    return *this;
  }
  ~DevMem() { release(); }
  void release() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; bytes = 0;
  }
  // frees what it holds, then allocates n bytes; the caller has made sure nothing still uses the old allocation
  int alloc(size_t n) {
    release();
    const hipError_t e = pinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
    if (e != hipSuccess) {
      p = nullptr;
      set_error(std::string(pinned ? "hipHostMalloc(" : "hipMalloc(") + std::to_string(n) + " B): " + hipGetErrorString(e));
      return TF_ERR_HIP;
    }
    bytes = n;
    return TF_OK;
  }
  template <typename T> T* as(size_t at = 0) const { return reinterpret_cast<T*>(static_cast<uint8_t*>(p) + at); }
  explicit operator bool() const { return p != nullptr; }

 protected:
  explicit DevMem(bool pin) : pinned(pin) {}
  bool pinned = false;
};
struct PinMem : DevMem {
  PinMem() : DevMem(true) {}
};

// Fitted buffer: a no-op while m holds at least `bytes`; otherwise drains `s` if m was in use (launches on it may still
// read or write the old allocation), frees, then allocates.  A caller whose buffer is also used on a second stream drains
// that one first.
inline int fit(DevMem& m, size_t bytes, hipStream_t s) {
  if (bytes <= m.bytes) return TF_OK;
  const hipError_t e = m.p ? hipStreamSynchronize(s) : hipSuccess;
  if (e != hipSuccess) { set_error(std::string("hipStreamSynchronize: ") + hipGetErrorString(e)); return TF_ERR_HIP; }
  return m.alloc(bytes);
}

}  // namespace tf
