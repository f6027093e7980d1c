// A stand-in for <hip/hip_runtime.h> on the CPU (tests/native/owned_harness.cpp): the calls abd_owned.hpp makes, backed by
// malloc.  Every create / allocate call is numbered; call number fake_hip::fail_at fails; fake_hip::live counts what exists.
#pragma once
#include <cstdlib>
#include <cstring>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
enum hipMemcpyKind { hipMemcpyHostToDevice = 1 };
enum { hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000, hipStreamNonBlocking = 1, hipEventDefault = 0 };
typedef struct fake_stream* hipStream_t;
typedef struct fake_event* hipEvent_t;

namespace fake_hip {
inline long live = 0, calls = 0, fail_at = 0;
inline hipError_t make(void** p, size_t bytes) {
  if (++calls == fail_at) return hipErrorOutOfMemory;  // (*p is left as it was: the handles must not trust it)
  *p = std::malloc(bytes ? bytes : 1);
  ++live;
  return hipSuccess;
}
inline hipError_t drop(void* p) {
  std::free(p);
  --live;
  return hipSuccess;
}
}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t n) { return fake_hip::make(p, n); }
inline hipError_t hipFree(void* p) { return fake_hip::drop(p); }
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return fake_hip::make(p, n); }
inline hipError_t hipHostFree(void* p) { return fake_hip::drop(p); }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { return *d = h, hipSuccess; }
inline hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t) { return std::memset(p, v, n), hipSuccess; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { return std::memcpy(d, s, n), hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return fake_hip::make((void**)s, 1); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::drop(s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_hip::make((void**)e, 1); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::drop(e); }
