// Private to native/src: what gpu.hip (the I/O engines), bulk_ops.hip
// (one-shot bulk operations) and parity_ops.hip (P+Q parity) need in
// common. Nothing engine-specific.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

#include "hipstore/engine.h"

namespace hipstore {

#define HIP_CHECK(expr)                                                   \
  do {                                                                    \
    hipError_t _e = (expr);                                               \
    if (_e != hipSuccess) {                                               \
      throw std::runtime_error(std::string("HIP error: ") +               \
                               hipGetErrorString(_e) + " at " #expr);     \
    }                                                                     \
  } while (0)

// Internal linkage on purpose: each of the two translation units gets
// its own copy, under the names it had when there was one file.
namespace {

constexpr uint32_t kWavesPerWg = 4;     // 256-thread workgroups

// Host pointer -> pointer the GPU may dereference.
template <typename T>
T* device_view(T* host_ptr) {
  void* dev = nullptr;
  HIP_CHECK(hipHostGetDevicePointer(&dev, const_cast<void*>(
      reinterpret_cast<const void*>(host_ptr)), 0));
  return reinterpret_cast<T*>(dev);
}

// Contiguous device-to-device range copy (volume clone): grid-stride
// over 16-byte elements, staged through LDS like the block kernels.
// No descriptors — the common clone case is one contiguous extent and
// per-tile descriptor fetches over PCIe dominated a descriptor-based
// clone (measured ~4x). Launched by hbm_copy_sync and HbmBdev::resize.
__global__ __launch_bounds__(256) void k_copy_range(
    const float4* __restrict__ src, float4* __restrict__ dst, uint64_t n16) {
  __shared__ __attribute__((aligned(16))) float4 lds[256];
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * blockDim.x;
  for (uint64_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16;
       i += stride) {
    lds[threadIdx.x] = src[i];
    dst[i] = lds[threadIdx.x];
  }
}

// A one-shot stream: device selected, own non-blocking stream created
// (never a device-wide sync: it would block on live persistent service
// kernels), and the hipErrorNotReady that polling elsewhere on this
// thread leaves behind cleared, so that only a failure of the caller's
// own work can fail the call. Synchronised, then destroyed, on every
// way out of the scope.
struct ScopedStream {
  hipStream_t stream = nullptr;

  explicit ScopedStream(int device) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    (void)hipGetLastError();
  }
  ~ScopedStream() {
    (void)hipStreamSynchronize(stream);
    (void)hipStreamDestroy(stream);
  }
  ScopedStream(const ScopedStream&) = delete;
  ScopedStream& operator=(const ScopedStream&) = delete;
};

// Pinned host buffer that grows on demand and keeps what it has. It
// frees only in its destructor: hipHostFree waits for the device to go
// idle, which stalls behind resident service kernels (see
// IoQueue::run), so the per-thread buffers below free nothing per call.
template <typename T>
struct PinnedBuf {
  T* ptr = nullptr;
  uint64_t capacity = 0;  // elements

  PinnedBuf() = default;
  ~PinnedBuf() { free_pinned(ptr); }
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;

  T* reserve(uint64_t n) {
    if (n > capacity) {
      free_pinned(ptr);
      ptr = nullptr;
      capacity = 0;
      ptr = static_cast<T*>(alloc_pinned(n * sizeof(T)));
      if (ptr == nullptr) throw std::runtime_error("bulk: out of memory");
      capacity = n;
    }
    return ptr;
  }
};

// Own stream, one launch, synchronise: only a failure of this launch
// (the stream starts with the last error cleared) may fail the call.
template <typename Launch>
int run_granule_kernel(int device, Launch launch) {
  try {
    ScopedStream ss(device);
    launch(ss.stream);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(ss.stream);
    return err == hipSuccess ? kIoOk : kIoFailed;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

}  // namespace

}  // namespace hipstore
