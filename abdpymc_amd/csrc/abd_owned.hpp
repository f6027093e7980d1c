// abd_owned.hpp -- the four owning handles of the host layer: device memory, pinned host memory, streams, events.
// Move-only; an empty handle destroys to nothing; moving leaves the source empty.  Each converts implicitly to the raw
// pointer / HIP handle it owns, so kernel argument structs, launches and copies take it as they took the raw value.
// No kernels here, and HIP is reached through <hip/hip_runtime.h> alone (tests/native substitutes that header).
#pragma once

#include <cstring>
#include <utility>

#include <hip/hip_runtime.h>

namespace abdi {

// Device memory of n elements of T (hipMalloc / hipFree); unsigned char for the panels held in the context's storage type.
template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    reset(std::exchange(o.p_, nullptr));
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset(T* p = nullptr) {  // releases what it holds and takes p over
    if (p_) (void)hipFree(p_);
    p_ = p;
  }
  // releases what it holds, then allocates n elements (left empty on failure)
  hipError_t alloc(size_t n) {
    reset();
    const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  // ... and zeroes them on stream st (not waited for)
  hipError_t alloc_zero(size_t n, hipStream_t st) {
    if (const hipError_t e = alloc(n)) return e;
    return hipMemsetAsync(p_, 0, n * sizeof(T), st);
  }
  // ... or fills them from host memory (synchronous copy)
  hipError_t upload(const void* src, size_t n) {
    if (const hipError_t e = alloc(n)) return e;
    return hipMemcpy(p_, src, n * sizeof(T), hipMemcpyHostToDevice);
  }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
};

// Pinned host memory of n elements of T, zeroed.  alloc: mapped and coherent (fine-grained), with both views -- host() for
// the host's reads and writes, dev() for kernel arguments.  alloc_pinned: plain pinned memory, a copy target: host() only.
template <typename T>
class MappedBuf {
 public:
  MappedBuf() = default;
  MappedBuf(MappedBuf&& o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
  MappedBuf& operator=(MappedBuf&& o) noexcept {
    T* const h = std::exchange(o.h_, nullptr);
    reset(h, std::exchange(o.d_, nullptr));
    return *this;
  }
  ~MappedBuf() { reset(); }
  void reset(T* h = nullptr, T* d = nullptr) {  // releases what it holds and takes (h, d) over
    if (h_) (void)hipHostFree(h_);
    h_ = h;
    d_ = d;
  }
  hipError_t alloc(size_t n) { return alloc(n, hipHostMallocMapped | hipHostMallocCoherent); }
  hipError_t alloc_pinned(size_t n) { return alloc(n, hipHostMallocDefault); }
  T* host() const { return h_; }
  T* dev() const { return d_; }
  operator T*() const { return h_; }

 private:
  hipError_t alloc(size_t n, unsigned flags) {
    reset();
    hipError_t e = hipHostMalloc((void**)&h_, n * sizeof(T), flags);
    if (e != hipSuccess) {
      h_ = nullptr;
      return e;
    }
    std::memset(h_, 0, n * sizeof(T));
    if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void**)&d_, h_, 0);
    if (e != hipSuccess) reset();
    return e;
  }
  T* h_ = nullptr;
  T* d_ = nullptr;
};

// A non-blocking HIP stream.
class Stream {
 public:
  Stream() = default;
  Stream(Stream&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {
    reset(std::exchange(o.s_, nullptr));
    return *this;
  }
  ~Stream() { reset(); }
  void reset(hipStream_t s = nullptr) {  // releases what it holds and takes s over
    if (s_) (void)hipStreamDestroy(s_);
    s_ = s;
  }
  hipError_t create() {
    reset();
    const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
    if (e != hipSuccess) s_ = nullptr;
    return e;
  }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};

// A HIP event.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
  Event& operator=(Event&& o) noexcept {
    reset(std::exchange(o.e_, nullptr));
    return *this;
  }
  ~Event() { reset(); }
  void reset(hipEvent_t e = nullptr) {  // releases what it holds and takes e over
    if (e_) (void)hipEventDestroy(e_);
    e_ = e;
  }
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    const hipError_t e = hipEventCreateWithFlags(&e_, flags);
    if (e != hipSuccess) e_ = nullptr;
    return e;
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace abdi
