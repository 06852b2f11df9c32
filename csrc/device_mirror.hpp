// A device array and its pinned host copy, drained before it is freed: the
// storage of every device-side check (device_checks.hpp).  GPU translation
// units only.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

#include "hip_check.hpp"

namespace p2p {

template <class T>
class DeviceMirror {
 public:
  DeviceMirror() = default;
  DeviceMirror(const DeviceMirror&) = delete;
  DeviceMirror& operator=(const DeviceMirror&) = delete;
  ~DeviceMirror() { release(); }

  // Room for n entries.  Growing frees the old arrays, which the stream may
  // still read or write: `drain` -- the caller's own wait for its stream --
  // runs first.  Never called between an enqueue and its wait.
  template <class Drain>
  void reserve(size_t n, Drain&& drain) {
    if (n <= cap_) return;
    if (cap_) drain();
    const size_t cap = std::max(n, 2 * cap_);
    release();
    HIPCHECK(hipMalloc(&dev_, sizeof(T) * cap));
    HIPCHECK(hipHostMalloc(&host_, sizeof(T) * cap, hipHostMallocDefault));
    cap_ = cap;
  }
  // One stream-ordered copy of the first n entries to the host array.
  void readback(size_t n, hipStream_t stream) {
    if (n) HIPCHECK(hipMemcpyAsync(host_, dev_, sizeof(T) * n, hipMemcpyDeviceToHost, stream));
  }
  T* device() const { return dev_; }
  const T* host() const { return host_; }  // valid once the caller has waited for the readback
  size_t capacity() const { return cap_; }

 private:
  void release() {
    if (dev_) (void)hipFree(dev_);
    if (host_) (void)hipHostFree(host_);
    dev_ = host_ = nullptr;
    cap_ = 0;
  }
  T* dev_ = nullptr;
  T* host_ = nullptr;
  size_t cap_ = 0;
};

}  // namespace p2p
