// Private to native/src: what gpu.hip (the I/O engines) and bulk_ops.hip
// (one-shot bulk operations) both need. Nothing engine-specific.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <stdexcept>
#include <string>

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

}  // namespace

}  // namespace hipstore
