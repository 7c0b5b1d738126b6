// dev_buf.h — HIP_CHECK and the RAII device allocation the whole device layer uses.
#pragma once

#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>
#include <vector>

namespace yrt {

#define HIP_CHECK(x)                                                                              \
  do {                                                                                            \
    hipError_t _e = (x);                                                                          \
    if (_e != hipSuccess)                                                                         \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(_e) + " at " #x);    \
  } while (0)

// RAII device allocation
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() {}
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void alloc(size_t n) {
    if (n <= bytes && p) return;
    release();
    if (n == 0) n = 16;
    HIP_CHECK(hipMalloc(&p, n));
    bytes = n;
  }
  template <class T>
  void upload(const std::vector<T>& v) {
    alloc(v.size() * sizeof(T));
    if (!v.empty()) HIP_CHECK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  }
  template <class T>
  T* as() const { return (T*)p; }
};

}  // namespace yrt
