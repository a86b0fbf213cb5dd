// MI355X (gfx950) bulk device operations on HBM bdevs: range copy,
// CRC32C, granule compare, marked copy, marked pack / unpack and
// granule fingerprints. Each call owns its stream, runs to completion
// and returns; none touches a channel, a ring or a service kernel (those
// are gpu.hip). Every call but the CRC and the range copy also has a
// generic path through bdev_read_sync / bdev_write_sync for bdevs that
// are not HBM-resident.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "gpu_internal.h"
#include "hipstore/crc32c.h"
#include "hipstore/engine.h"
#include "hipstore/fingerprint.h"

namespace hipstore {

// CPU fallback defined in crc32c.cpp.
void crc32c_cpu_fallback(Bdev* bdev, uint64_t offset, uint32_t block_size,
                         uint32_t count, uint32_t* out);

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

namespace {

// --- CRC32C (Castagnoli, reflected 0x82F63B78) -----------------------------
//
// One LANE per block: lanes of a wave digest 64 different blocks in
// parallel, the 256-entry table lives in LDS (one copy per workgroup,
// broadcast reads are conflict-free). Parallelism comes from batch
// width (count >= a few thousand blocks fills the chip), which matches
// the NVMe-oF/TCP digest use: one CRC per in-flight 4 KiB PDU.
__global__ __launch_bounds__(256) void k_crc32c_blocks(
    const uint8_t* __restrict__ base, uint32_t block_size, uint32_t count,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t table[256];
  // Build the table once per workgroup (cheap: 8 iterations/entry).
  if (threadIdx.x < 256) {
    uint32_t crc = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      crc = (crc & 1u) ? (crc >> 1) ^ 0x82F63B78u : crc >> 1;
    }
    table[threadIdx.x] = crc;
  }
  __syncthreads();
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= count) return;
  const uint8_t* p = base + static_cast<uint64_t>(idx) * block_size;
  uint32_t crc = 0xFFFFFFFFu;
  // 4 bytes per iteration through a word load (block_size % 4 == 0 is
  // guaranteed by the 512-byte block granularity).
  const uint32_t* pw = reinterpret_cast<const uint32_t*>(p);
  for (uint32_t i = 0; i < block_size / 4; ++i) {
    uint32_t w = pw[i];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      crc = (crc >> 8) ^ table[(crc ^ (w & 0xFFu)) & 0xFFu];
      w >>= 8;
    }
  }
  out[idx] = ~crc;
}

// --- granule compare / marked copy (replica scrub, clone verify) -----------
//
// One workgroup owns one 64-bit bitmap word (64 granules) per
// grid-stride step; each of its 4 waves compares 16 consecutive
// granules, one whole granule at a time: 16 B/lane loads of both
// sides, XOR, OR into a lane-private accumulator, then one 64-bit
// ballot decides the granule's bit (wave-uniform). The four 16-bit
// partials meet in LDS and thread 0 writes the word with one plain
// store: no atomics, no pre-zeroed buffer, and tail bits past
// n_granules are written as 0 because their granules are never
// visited. Granules below 1 KiB leave the upper lanes idle.
constexpr uint32_t kDiffGranulesPerWave = 64 / kWavesPerWg;

__global__ __launch_bounds__(kWavesPerWg * 64) void k_diff_granules(
    const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
    uint64_t n_granules, uint32_t granule_bytes,
    unsigned long long* __restrict__ bitmap) {
  __shared__ uint32_t partial[kWavesPerWg];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint64_t n_words = (n_granules + 63) >> 6;
  for (uint64_t w = blockIdx.x; w < n_words; w += gridDim.x) {
    const uint64_t g0 = w * 64 + wave * kDiffGranulesPerWave;
    uint32_t bits = 0;
    for (uint32_t j = 0; j < kDiffGranulesPerWave; ++j) {
      const uint64_t g = g0 + j;
      if (g >= n_granules) break;  // wave-uniform
      const uint4* __restrict__ pa =
          reinterpret_cast<const uint4*>(a + g * granule_bytes);
      const uint4* __restrict__ pb =
          reinterpret_cast<const uint4*>(b + g * granule_bytes);
      uint32_t acc = 0;
#pragma unroll 4
      for (uint32_t i = lane; i < n16; i += 64) {
        const uint4 x = pa[i];
        const uint4 y = pb[i];
        acc |= (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
      }
      if (__ballot(acc != 0) != 0ull) bits |= 1u << j;
    }
    if (lane == 0) partial[wave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long word = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWavesPerWg; ++k) {
        word |= static_cast<unsigned long long>(partial[k])
                << (k * kDiffGranulesPerWave);
      }
      bitmap[w] = word;
    }
    __syncthreads();  // partial[] is rewritten by the next step
  }
}

// Copies exactly the granules whose bitmap bit is set. Same work split
// as k_diff_granules (workgroup per word, wave per 16-bit slice, wave
// per granule), so the bit test is wave-uniform and a zero word costs
// one load. Unmarked granules of dst are never written.
__global__ __launch_bounds__(kWavesPerWg * 64) void k_copy_marked(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
    const unsigned long long* __restrict__ bitmap, uint64_t n_granules,
    uint32_t granule_bytes) {
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint64_t n_words = (n_granules + 63) >> 6;
  for (uint64_t w = blockIdx.x; w < n_words; w += gridDim.x) {
    const unsigned long long word = bitmap[w];
    uint32_t bits = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(
        (word >> (wave * kDiffGranulesPerWave)) & 0xFFFFu));
    while (bits != 0) {
      const uint32_t j = static_cast<uint32_t>(__builtin_ctz(bits));
      bits &= bits - 1;
      const uint64_t g = w * 64 + wave * kDiffGranulesPerWave + j;
      if (g >= n_granules) break;  // stray tail bits in the caller's bitmap
      const uint4* __restrict__ ps =
          reinterpret_cast<const uint4*>(src + g * granule_bytes);
      uint4* __restrict__ pd =
          reinterpret_cast<uint4*>(dst + g * granule_bytes);
#pragma unroll 4
      for (uint32_t i = lane; i < n16; i += 64) pd[i] = ps[i];
    }
  }
}

// --- marked gather / scatter (incremental checkpoints) ---------------------
//
// k_pack_marked moves the marked granules of one window [g_begin, g_end)
// of a range into a dense buffer, in ascending granule order;
// k_unpack_marked is its inverse. Same work split as k_copy_marked. A
// granule's dense slot is a pure function of the bitmap:
//   slot = rank_before_word[w] + popcount(word & ((1 << bit) - 1))
//          - window_first_rank
// rank_before_word is the exclusive prefix popcount of the bitmap,
// built on the host next to the pinned bitmap copy (12 bytes of PCIe
// reads per 64 granules), so there are no atomics, no ordering between
// workgroups and nothing that depends on what the dense buffer held. A
// window may begin and end inside a word: bits outside it are masked
// for the walk but still counted below a bit, which is what subtracting
// window_first_rank (marks before g_begin) expects. The host keeps
// g_end <= n_granules, so stray tail bits of the caller's bitmap are
// never visited, and they lie above every valid bit, so they are never
// counted either. `window_count` bounds the slot: nothing outside
// [0, window_count * granule) of the dense buffer is touched.
struct MarkedWindow {
  uint64_t g_begin;
  uint64_t g_end;
  uint32_t first_rank;  // marked granules before g_begin
  uint32_t count;       // marked granules in the window
};

template <bool kPack>
__device__ __forceinline__ void marked_window_walk(
    uint8_t* __restrict__ bdev_base, uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, const MarkedWindow win,
    uint32_t granule_bytes) {
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint64_t w_end = (win.g_end + 63) >> 6;
  for (uint64_t w = (win.g_begin >> 6) + blockIdx.x; w < w_end;
       w += gridDim.x) {
    const unsigned long long word = bitmap[w];
    const uint64_t g0 = w * 64;
    unsigned long long inside = word;
    if (g0 < win.g_begin) inside &= ~0ull << (win.g_begin - g0);
    if (win.g_end - g0 < 64) inside &= (1ull << (win.g_end - g0)) - 1;
    uint32_t bits = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(
        (inside >> (wave * kDiffGranulesPerWave)) & 0xFFFFu));
    if (bits == 0) continue;  // wave-uniform
    const uint32_t rank0 =
        __builtin_amdgcn_readfirstlane(rank_before_word[w]) - win.first_rank;
    while (bits != 0) {
      const uint32_t bit = wave * kDiffGranulesPerWave +
                           static_cast<uint32_t>(__builtin_ctz(bits));
      bits &= bits - 1;
      const uint32_t slot =
          rank0 + static_cast<uint32_t>(__popcll(word & ((1ull << bit) - 1)));
      if (slot >= win.count) break;  // bitmap and ranks disagree: stay inside
      uint4* __restrict__ pg = reinterpret_cast<uint4*>(
          bdev_base + (g0 + bit) * granule_bytes);
      uint4* __restrict__ ps = reinterpret_cast<uint4*>(
          dense + static_cast<uint64_t>(slot) * granule_bytes);
      if (kPack) {
#pragma unroll 4
        for (uint32_t i = lane; i < n16; i += 64) ps[i] = pg[i];
      } else {
#pragma unroll 4
        for (uint32_t i = lane; i < n16; i += 64) pg[i] = ps[i];
      }
    }
  }
}

__global__ __launch_bounds__(kWavesPerWg * 64) void k_pack_marked(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule_bytes) {
  marked_window_walk<true>(const_cast<uint8_t*>(src), dense, bitmap,
                           rank_before_word, win, granule_bytes);
}

__global__ __launch_bounds__(kWavesPerWg * 64) void k_unpack_marked(
    uint8_t* __restrict__ dst, const uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule_bytes) {
  marked_window_walk<false>(dst, const_cast<uint8_t*>(dense), bitmap,
                            rank_before_word, win, granule_bytes);
}

// --- granule fingerprints (base-less incremental checkpoints) --------------
//
// The definition is in fingerprint.h. A wave takes one whole granule at
// a time and waves grid-stride over granules; lane l is stream l, so its
// 16-byte loads are vectors l, l + 64, ... and a wave-instruction reads
// 1 KiB contiguously. Whole rows go four at a time: the four loads are
// issued before the first dependent round, so several stay in flight
// behind the two multiply chains. Lanes without a vector keep their
// seed. The two u64 sums cross the 64 lanes by a shuffle butterfly and
// lane 0 writes the 16 bytes with one store: no LDS, no atomics, and
// nothing depends on what `out` held.
__device__ __forceinline__ uint64_t fp_round(uint64_t acc, uint64_t q) {
  const uint64_t v = acc + q * kFingerprintP2;
  return ((v << 31) | (v >> 33)) * kFingerprintP1;
}

__device__ __forceinline__ uint64_t fp_mix(uint64_t h) {
  h ^= h >> 33;
  h *= kFingerprintP2;
  h ^= h >> 29;
  h *= kFingerprintP3;
  h ^= h >> 32;
  return h;
}

__device__ __forceinline__ uint64_t fp_q0(const uint4 v) {
  return (static_cast<uint64_t>(v.y) << 32) | v.x;
}
__device__ __forceinline__ uint64_t fp_q1(const uint4 v) {
  return (static_cast<uint64_t>(v.w) << 32) | v.z;
}

constexpr uint32_t kFingerprintUnroll = 4;  // rows loaded ahead of their rounds

__global__ __launch_bounds__(kWavesPerWg * 64) void k_fingerprint_granules(
    const uint8_t* __restrict__ base, uint64_t n_granules,
    uint32_t granule_bytes, uint4* __restrict__ out) {
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint32_t rows = n16 >> 6;  // whole rows of 64 vectors
  const uint32_t rest = n16 & 63;  // vectors of the ragged last row
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kWavesPerWg;
  for (uint64_t g = static_cast<uint64_t>(blockIdx.x) * kWavesPerWg + wave;
       g < n_granules; g += stride) {  // wave-uniform
    const uint4* __restrict__ p =
        reinterpret_cast<const uint4*>(base + g * granule_bytes) + lane;
    uint64_t a = kFingerprintP1 * (lane + 1);
    uint64_t b = kFingerprintP2 * (lane + 1);
    uint32_t r = 0;
    for (; r + kFingerprintUnroll <= rows; r += kFingerprintUnroll) {
      uint4 v[kFingerprintUnroll];
#pragma unroll
      for (uint32_t k = 0; k < kFingerprintUnroll; ++k) v[k] = p[(r + k) * 64];
#pragma unroll
      for (uint32_t k = 0; k < kFingerprintUnroll; ++k) {
        a = fp_round(a, fp_q0(v[k]));
        b = fp_round(b, fp_q1(v[k]));
      }
    }
    for (; r < rows; ++r) {
      const uint4 v = p[r * 64];
      a = fp_round(a, fp_q0(v));
      b = fp_round(b, fp_q1(v));
    }
    if (lane < rest) {
      const uint4 v = p[rows * 64];
      a = fp_round(a, fp_q0(v));
      b = fp_round(b, fp_q1(v));
    }
    uint64_t d0 = fp_mix(a ^ fp_mix(b));
    uint64_t d1 = fp_mix(b + fp_mix(a));
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      d0 += __shfl_xor(d0, m);
      d1 += __shfl_xor(d1, m);
    }
    if (lane == 0) {
      out[g] = make_uint4(static_cast<uint32_t>(d0),
                          static_cast<uint32_t>(d0 >> 32),
                          static_cast<uint32_t>(d1),
                          static_cast<uint32_t>(d1 >> 32));
    }
  }
}

// --- host helpers shared by every call below -------------------------------

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

constexpr uint64_t kDiffHostChunk = 1ull << 20;  // generic-path read size cap
// 256 MiB of bitmap; keeps the pinned buffer and the host fold bounded.
constexpr uint64_t kMaxDiffGranules = 1ull << 31;

// Per-thread pinned buffers of the granule calls. The GPU writes / reads
// the bitmap and its ranks in place (zero-copy; the bitmap is 1/4096 of
// the data at 512-byte granules). `chunks` and `staging` are distinct
// because copy_span_generic and marked_generic can each run under a
// caller that holds the other. A sink or source callback must not call
// back into this family on its own thread: it would reuse `words`.
struct BulkCtx {
  PinnedBuf<unsigned long long> words;  // bitmap
  PinnedBuf<uint32_t> ranks;    // exclusive prefix popcount of `words`
  PinnedBuf<uint8_t> chunks;    // 2 x kDiffHostChunk, generic compare / copy
  PinnedBuf<uint8_t> staging;   // dense stream (two halves on the GPU path)
  PinnedBuf<uint8_t> prints;    // fingerprints (two halves on the GPU path)
};
constexpr uint64_t kMinBitmapWords = 4096;  // floor of `words` and `ranks`

BulkCtx& bulk_ctx() {
  thread_local BulkCtx ctx;
  return ctx;
}

}  // namespace

void crc32c_hbm_blocks(Bdev* bdev, uint64_t offset, uint32_t block_size,
                       uint32_t count, uint32_t* out) {
  if (block_size % 4 != 0) {
    throw std::runtime_error("crc32c: block_size must be a multiple of 4");
  }
  if (offset % bdev->block_size() != 0 ||
      offset + static_cast<uint64_t>(block_size) * count > bdev->size_bytes()) {
    throw std::runtime_error("crc32c: range out of bounds");
  }
  if (count == 0) return;  // nothing to digest: no zero-sized launch
  void* base = bdev->device_base();
  if (base == nullptr) {
    crc32c_cpu_fallback(bdev, offset, block_size, count, out);
    return;
  }
  HIP_CHECK(hipSetDevice(bdev->gpu_device()));
  // Thread-local stream + result buffer: hipHostMalloc and stream
  // creation cost ~1 ms each, which collapsed per-I/O digests (NVMe/TCP
  // targets call this once per large read). Own non-blocking stream +
  // stream sync, never a device-wide sync (it would block on live
  // persistent service kernels).
  struct DigestCtx {
    hipStream_t stream = nullptr;
    PinnedBuf<uint32_t> out;

    ~DigestCtx() {
      if (stream != nullptr) (void)hipStreamDestroy(stream);
    }
  };
  thread_local DigestCtx ctx;
  if (ctx.stream == nullptr) {
    HIP_CHECK(hipStreamCreateWithFlags(&ctx.stream, hipStreamNonBlocking));
  }
  if (count > ctx.out.capacity) {
    ctx.out.reserve(std::max<uint64_t>(
        count, std::max<uint64_t>(1024, ctx.out.capacity * 2)));
  }
  const uint32_t grid = (count + 255) / 256;
  hipLaunchKernelGGL(k_crc32c_blocks, dim3(grid), dim3(256), 0, ctx.stream,
                     static_cast<const uint8_t*>(base) + offset, block_size,
                     count, device_view(ctx.out.ptr));
  HIP_CHECK(hipStreamSynchronize(ctx.stream));
  memcpy(out, ctx.out.ptr, static_cast<size_t>(count) * 4);
}

uint32_t crc32c_hbm_range(Bdev* bdev, uint64_t offset, uint64_t length) {
  constexpr uint32_t kDigestBlock = 4096;
  if (length == 0 || length % kDigestBlock != 0 ||
      length / kDigestBlock > UINT32_MAX) {
    throw std::runtime_error(
        "crc32c: range length must be a non-zero multiple of 4096");
  }
  const uint32_t count = static_cast<uint32_t>(length / kDigestBlock);
  std::vector<uint32_t> crcs(count);
  crc32c_hbm_blocks(bdev, offset, kDigestBlock, count, crcs.data());
  uint32_t crc = crcs[0];
  for (uint32_t i = 1; i < count; ++i) {
    crc = crc32c_combine(crc, crcs[i], kDigestBlock);
  }
  return crc;
}

int hbm_copy_sync(Bdev* src, uint64_t src_offset, Bdev* dst,
                  uint64_t dst_offset, uint64_t length) {
  uint8_t* src_base = static_cast<uint8_t*>(src->device_base());
  uint8_t* dst_base = static_cast<uint8_t*>(dst->device_base());
  if (src_base == nullptr || dst_base == nullptr) return kIoInvalid;
  if (length == 0 || length % 16 != 0 ||
      src_offset + length > src->size_bytes() ||
      dst_offset + length > dst->size_bytes()) {
    return kIoInvalid;
  }
  // float4 accesses: hipMalloc bases are 256-byte aligned, so the
  // offsets decide the alignment of both pointers.
  if (src_offset % 16 != 0 || dst_offset % 16 != 0) return kIoInvalid;
  // Overlap (only possible within one backing store): the grid-stride
  // kernel gives neither memcpy nor memmove semantics there.
  const uint8_t* s0 = src_base + src_offset;
  const uint8_t* d0 = dst_base + dst_offset;
  if (src->gpu_device() == dst->gpu_device() && s0 < d0 + length &&
      d0 < s0 + length) {
    return kIoInvalid;
  }
  const int src_dev = src->gpu_device();
  const int dst_dev = dst->gpu_device();
  try {
    ScopedStream ss(dst_dev);
    hipError_t err = hipSuccess;
    if (src_dev != dst_dev) {
      // Cross-GPU: one xGMI peer copy (SDMA saturates the link).
      (void)hipSetDevice(src_dev);
      (void)hipDeviceEnablePeerAccess(dst_dev, 0);
      (void)hipSetDevice(dst_dev);
      (void)hipDeviceEnablePeerAccess(src_dev, 0);
      err = hipMemcpyPeerAsync(dst_base + dst_offset, dst_dev,
                               src_base + src_offset, src_dev, length,
                               ss.stream);
    } else {
      // Same device: contiguous LDS-staged range copy, grid-stride
      // (2048 workgroups fill the chip; no per-tile descriptors).
      const uint64_t n16 = length / 16;
      const uint32_t grid = static_cast<uint32_t>(
          std::min<uint64_t>((n16 + 255) / 256, 2048));
      hipLaunchKernelGGL(k_copy_range, dim3(grid), dim3(256), 0, ss.stream,
                         reinterpret_cast<const float4*>(src_base + src_offset),
                         reinterpret_cast<float4*>(dst_base + dst_offset),
                         n16);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(ss.stream);
    return err == hipSuccess ? kIoOk : kIoFailed;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

// ---------------------------------------------------------------------------
// Granule compare / marked copy
// ---------------------------------------------------------------------------

namespace {

// Shared validation; one bdev is the pair (bdev, bdev). Bounds are
// phrased by subtraction so no 64-bit sum can wrap. A call that takes a
// bitmap passes it: it must cover the range.
bool granule_ranges_ok(Bdev* a, uint64_t a_offset, Bdev* b, uint64_t b_offset,
                       uint64_t length, uint32_t granule,
                       const std::vector<uint64_t>* bitmap = nullptr) {
  if (a == nullptr || b == nullptr) return false;
  const uint64_t bs = a->block_size();
  if (bs == 0 || bs != b->block_size() || bs > kDiffHostChunk) return false;
  if (granule == 0 || granule % bs != 0 || granule % 16 != 0) return false;
  if (length == 0 || length % granule != 0 || a_offset % granule != 0 ||
      b_offset % granule != 0) {
    return false;
  }
  if (length > a->size_bytes() || a_offset > a->size_bytes() - length ||
      length > b->size_bytes() || b_offset > b->size_bytes() - length) {
    return false;
  }
  const uint64_t n_granules = length / granule;
  if (n_granules > kMaxDiffGranules) return false;
  return bitmap == nullptr || bitmap->size() >= (n_granules + 63) / 64;
}

// Device the pair's kernels run on, or -1 for the generic path: both
// bdevs HBM-resident, and across devices `a`'s device must be able to
// reach `b`'s memory (peer access, enabled as ReplicatedBdev does).
int granule_kernel_device(Bdev* a, Bdev* b) {
  if (a->device_base() == nullptr || b->device_base() == nullptr) return -1;
  if (!gpu_available()) return -1;
  const int a_dev = a->gpu_device();
  const int b_dev = b->gpu_device();
  if (a_dev < 0 || b_dev < 0) return -1;
  if (a_dev == b_dev) return a_dev;
  int can = 0;
  if (hipSetDevice(a_dev) != hipSuccess ||
      hipDeviceCanAccessPeer(&can, a_dev, b_dev) != hipSuccess || can == 0) {
    return -1;
  }
  const hipError_t err = hipDeviceEnablePeerAccess(b_dev, 0);
  (void)hipGetLastError();  // "already enabled" must not stick
  if (err != hipSuccess && err != hipErrorPeerAccessAlreadyEnabled) return -1;
  return a_dev;
}

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

uint32_t granule_grid(uint64_t n_granules) {
  return static_cast<uint32_t>(
      std::min<uint64_t>((n_granules + 63) / 64, 2048));
}

// Largest multiple of the block size that fits the generic-path cap.
uint64_t host_chunk_bytes(Bdev* bdev) {
  return kDiffHostChunk / bdev->block_size() * bdev->block_size();
}

int diff_generic(Bdev* a, uint64_t a_offset, Bdev* b, uint64_t b_offset,
                 uint64_t length, uint32_t granule,
                 unsigned long long* words, uint64_t n_words) {
  memset(words, 0, n_words * 8);
  uint8_t* buf_a = bulk_ctx().chunks.reserve(2 * kDiffHostChunk);
  uint8_t* buf_b = buf_a + kDiffHostChunk;
  const uint64_t chunk = host_chunk_bytes(a);
  for (uint64_t pos = 0; pos < length; pos += chunk) {
    const uint64_t n = std::min(chunk, length - pos);
    int status = bdev_read_sync(a, a_offset + pos, buf_a, n);
    if (status == kIoOk) status = bdev_read_sync(b, b_offset + pos, buf_b, n);
    if (status != kIoOk) return status;
    // A chunk need not start or end on a granule boundary (granules
    // above the cap span several chunks): compare piecewise.
    for (uint64_t off = 0; off < n;) {
      const uint64_t g = (pos + off) / granule;
      const uint64_t piece =
          std::min<uint64_t>(granule - (pos + off) % granule, n - off);
      if (memcmp(buf_a + off, buf_b + off, piece) != 0) {
        words[g / 64] |= 1ull << (g % 64);
      }
      off += piece;
    }
  }
  return kIoOk;
}

int copy_span_generic(Bdev* src, uint64_t src_offset, Bdev* dst,
                      uint64_t dst_offset, uint64_t length) {
  uint8_t* buf = bulk_ctx().chunks.reserve(2 * kDiffHostChunk);
  const uint64_t chunk = host_chunk_bytes(src);
  for (uint64_t pos = 0; pos < length; pos += chunk) {
    const uint64_t n = std::min(chunk, length - pos);
    int status = bdev_read_sync(src, src_offset + pos, buf, n);
    if (status == kIoOk) status = bdev_write_sync(dst, dst_offset + pos, buf, n);
    if (status != kIoOk) return status;
  }
  return kIoOk;
}

// What every call that takes a bitmap works from: the pinned copy of
// the caller's bitmap with stray tail bits cleared (the kernels read it
// in place), the number of marks, and, when asked for, the exclusive
// prefix popcount that k_pack_marked / k_unpack_marked read.
// `chunk_granules` belongs to pack / unpack, which set it.
struct MarkedPlan {
  uint64_t n_granules = 0;
  uint64_t n_words = 0;
  uint64_t marked = 0;
  uint64_t chunk_granules = 0;
  unsigned long long* words = nullptr;
  uint32_t* ranks = nullptr;
};

// `bitmap` holds at least ceil(n_granules / 64) words (granule_ranges_ok).
MarkedPlan build_marked_plan(uint64_t n_granules,
                             const std::vector<uint64_t>& bitmap,
                             bool want_ranks) {
  MarkedPlan plan;
  plan.n_granules = n_granules;
  plan.n_words = (n_granules + 63) / 64;
  const uint64_t room = std::max(plan.n_words, kMinBitmapWords);
  plan.words = bulk_ctx().words.reserve(room);
  if (want_ranks) plan.ranks = bulk_ctx().ranks.reserve(room);
  uint64_t rank = 0;  // <= kMaxDiffGranules, fits the u32 the kernels read
  for (uint64_t w = 0; w < plan.n_words; ++w) {
    unsigned long long word = bitmap[w];
    const uint64_t left = n_granules - w * 64;
    if (left < 64) word &= (1ull << left) - 1;
    plan.words[w] = word;
    if (want_ranks) plan.ranks[w] = static_cast<uint32_t>(rank);
    rank += static_cast<uint64_t>(__builtin_popcountll(word));
  }
  plan.marked = rank;
  return plan;
}

// Walks a plan's runs of consecutive marked granules in ascending
// order. next() hands out the run at or after the cursor, cut to
// `max_len` granules; the rest of a cut run is the next call's.
struct RunCursor {
  const MarkedPlan& plan;
  uint64_t g = 0;

  bool next(uint64_t max_len, uint64_t* begin, uint64_t* len) {
    // A zero word (or zero rest of one) is skipped whole.
    for (;; g = (g / 64 + 1) * 64) {
      if (g >= plan.n_granules) return false;
      const unsigned long long rest = plan.words[g / 64] >> (g % 64);
      if (rest != 0) {
        g += static_cast<uint64_t>(__builtin_ctzll(rest));
        break;
      }
    }
    uint64_t end = g + 1;
    while (end < plan.n_granules && end - g < max_len &&
           ((plan.words[end / 64] >> (end % 64)) & 1)) {
      ++end;
    }
    *begin = g;
    *len = end - g;
    g = end;
    return true;
  }
};

}  // namespace

uint64_t bdev_common_length(Bdev* a, uint64_t a_offset, Bdev* b,
                            uint64_t b_offset, uint32_t granule) {
  if (granule == 0 || a_offset > a->size_bytes() ||
      b_offset > b->size_bytes()) {
    return 0;
  }
  const uint64_t room =
      std::min(a->size_bytes() - a_offset, b->size_bytes() - b_offset);
  return room / granule * granule;
}

int bdev_diff_sync(Bdev* a, uint64_t a_offset, Bdev* b, uint64_t b_offset,
                   uint64_t length, uint32_t granule, uint32_t max_report,
                   std::vector<uint64_t>* bitmap_out, DiffStats* stats) {
  if (!granule_ranges_ok(a, a_offset, b, b_offset, length, granule)) {
    return kIoInvalid;
  }
  const uint64_t n_granules = length / granule;
  const uint64_t n_words = (n_granules + 63) / 64;
  unsigned long long* words = nullptr;
  int status;
  try {
    words = bulk_ctx().words.reserve(std::max(n_words, kMinBitmapWords));
    const int device = granule_kernel_device(a, b);
    if (device >= 0) {
      unsigned long long* dev_words = device_view(words);
      const uint8_t* pa = static_cast<uint8_t*>(a->device_base()) + a_offset;
      const uint8_t* pb = static_cast<uint8_t*>(b->device_base()) + b_offset;
      status = run_granule_kernel(device, [&](hipStream_t stream) {
        hipLaunchKernelGGL(k_diff_granules, dim3(granule_grid(n_granules)),
                           dim3(kWavesPerWg * 64), 0, stream, pa, pb,
                           n_granules, granule, dev_words);
      });
    } else {
      status = diff_generic(a, a_offset, b, b_offset, length, granule, words,
                            n_words);
    }
  } catch (const std::exception&) {
    status = kIoFailed;
  }
  if (status != kIoOk) return status;
  if (stats != nullptr) {
    stats->granules = n_granules;
    stats->mismatched = 0;
    stats->first_mismatches.clear();
    for (uint64_t w = 0; w < n_words; ++w) {
      unsigned long long word = words[w];
      stats->mismatched += static_cast<uint64_t>(__builtin_popcountll(word));
      while (word != 0 && stats->first_mismatches.size() < max_report) {
        stats->first_mismatches.push_back(
            w * 64 + static_cast<uint64_t>(__builtin_ctzll(word)));
        word &= word - 1;
      }
    }
  }
  if (bitmap_out != nullptr) bitmap_out->assign(words, words + n_words);
  return kIoOk;
}

int bdev_copy_marked_sync(Bdev* src, uint64_t src_offset, Bdev* dst,
                          uint64_t dst_offset, uint64_t length,
                          uint32_t granule,
                          const std::vector<uint64_t>& bitmap,
                          uint64_t* copied) {
  if (!granule_ranges_ok(src, src_offset, dst, dst_offset, length, granule,
                         &bitmap)) {
    return kIoInvalid;
  }
  // Overlap is only possible within one backing store (validated
  // ranges: the differences below cannot wrap).
  const uint8_t* s_base = static_cast<uint8_t*>(src->device_base());
  const uint8_t* d_base = static_cast<uint8_t*>(dst->device_base());
  const bool same_store =
      src == dst || (s_base != nullptr && s_base == d_base &&
                     src->gpu_device() == dst->gpu_device());
  if (same_store) {
    const uint64_t lo = std::min(src_offset, dst_offset);
    const uint64_t hi = std::max(src_offset, dst_offset);
    if (hi - lo < length) return kIoInvalid;
  }
  if (copied != nullptr) *copied = 0;
  try {
    const MarkedPlan plan = build_marked_plan(length / granule, bitmap, false);
    if (plan.marked == 0) return kIoOk;  // nothing to copy: no launch
    int status = kIoOk;
    const int device = granule_kernel_device(src, dst);
    if (device >= 0) {
      const unsigned long long* dev_words = device_view(plan.words);
      const uint8_t* ps = s_base + src_offset;
      uint8_t* pd = static_cast<uint8_t*>(dst->device_base()) + dst_offset;
      status = run_granule_kernel(device, [&](hipStream_t stream) {
        hipLaunchKernelGGL(k_copy_marked, dim3(granule_grid(plan.n_granules)),
                           dim3(kWavesPerWg * 64), 0, stream, ps, pd,
                           dev_words, plan.n_granules, granule);
      });
    } else {
      // Runs of marked granules move as one span.
      RunCursor runs{plan};
      uint64_t g = 0;
      uint64_t len = 0;
      while (status == kIoOk && runs.next(UINT64_MAX, &g, &len)) {
        status = copy_span_generic(src, src_offset + g * granule, dst,
                                   dst_offset + g * granule, len * granule);
      }
    }
    if (status == kIoOk && copied != nullptr) *copied = plan.marked;
    return status;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

// ---------------------------------------------------------------------------
// Marked gather / scatter through a dense staging stream
// ---------------------------------------------------------------------------

namespace {

constexpr uint64_t kDefaultStagingHalf = 16ull << 20;

// The window that starts at granule `g_begin` and holds the next
// min(chunk, marks left) marked granules: it ends right after the last
// of them.
MarkedWindow next_marked_window(const MarkedPlan& plan, uint64_t g_begin,
                                uint64_t first_rank) {
  MarkedWindow win;
  win.g_begin = g_begin;
  win.first_rank = static_cast<uint32_t>(first_rank);
  win.count = static_cast<uint32_t>(
      std::min(plan.chunk_granules, plan.marked - first_rank));
  uint64_t need = win.count;
  uint64_t g_end = g_begin;
  for (uint64_t w = g_begin / 64; w < plan.n_words && need > 0; ++w) {
    unsigned long long word = plan.words[w];
    if (w * 64 < g_begin) word &= ~0ull << (g_begin - w * 64);
    const uint64_t have = static_cast<uint64_t>(__builtin_popcountll(word));
    if (have < need) {
      need -= have;
      continue;
    }
    for (; need > 1; --need) word &= word - 1;
    g_end = w * 64 + static_cast<uint64_t>(__builtin_ctzll(word)) + 1;
    need = 0;
  }
  win.g_end = g_end;
  return win;
}

// A window's kernel runs for a fraction of a millisecond and the GPU
// idles until the host has seen it end and launched the window after
// next, so poll for that long before falling back to a sleeping wait.
void wait_marked_event(hipEvent_t event) {
  using clock = std::chrono::steady_clock;
  const auto give_up = clock::now() + std::chrono::milliseconds(2);
  hipError_t err = hipEventQuery(event);
  while (err == hipErrorNotReady && clock::now() < give_up) {
    err = hipEventQuery(event);
  }
  (void)hipGetLastError();  // hipErrorNotReady must not stick
  if (err == hipErrorNotReady) err = hipEventSynchronize(event);
  HIP_CHECK(err);
}

// A one-shot stream with one event per half of a two-half pinned
// buffer: the window loops below launch into one half while the host
// works on the other.
struct HalvesStream : ScopedStream {
  hipEvent_t done[2] = {nullptr, nullptr};

  explicit HalvesStream(int device) : ScopedStream(device) {
    for (hipEvent_t& e : done) {
      HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
  }
  ~HalvesStream() {
    (void)hipStreamSynchronize(stream);  // before the events go
    for (hipEvent_t e : done) {
      if (e != nullptr) (void)hipEventDestroy(e);
    }
  }
};

uint32_t marked_window_grid(const MarkedWindow& win) {
  return granule_grid((win.g_end + 63) / 64 * 64 - win.g_begin / 64 * 64);
}

// What both GPU window loops run on. One stream and one event per
// staging half: launch window k+1, then wait for window k only. The
// kernels read the plan and fill or drain the two halves in place, so
// the device's view of those is kept here too.
struct MarkedStream : HalvesStream {
  uint32_t granule;
  uint64_t half_bytes;
  uint8_t* staging;
  uint8_t* dev_staging;
  const unsigned long long* dev_words;
  const uint32_t* dev_ranks;
  uint8_t* base;  // the bdev's range in device memory

  MarkedStream(int device, Bdev* bdev, uint64_t offset, uint32_t granule_bytes,
               const MarkedPlan& plan)
      : HalvesStream(device), granule(granule_bytes),
        half_bytes(plan.chunk_granules * granule_bytes),
        staging(bulk_ctx().staging.reserve(2 * half_bytes)),
        dev_staging(device_view(staging)), dev_words(device_view(plan.words)),
        dev_ranks(device_view(plan.ranks)),
        base(static_cast<uint8_t*>(bdev->device_base()) + offset) {}

  // k_pack_marked or k_unpack_marked over one window and one half.
  template <typename Kernel>
  void launch(Kernel kernel, const MarkedWindow& win, int half) {
    hipLaunchKernelGGL(kernel, dim3(marked_window_grid(win)),
                       dim3(kWavesPerWg * 64), 0, stream, base,
                       dev_staging + half * half_bytes, dev_words, dev_ranks,
                       win, granule);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(done[half], stream));
  }
};

// Pack launches one window ahead, then waits for the current one.
int marked_gpu(MarkedStream& ms, const MarkedPlan& plan, const PackSink& sink,
               uint64_t* packed) {
  MarkedWindow cur = next_marked_window(plan, 0, 0);
  ms.launch(k_pack_marked, cur, 0);
  for (int half = 0;; half ^= 1) {
    const uint64_t next_rank = cur.first_rank + static_cast<uint64_t>(cur.count);
    MarkedWindow next{};
    if (next_rank < plan.marked) {
      next = next_marked_window(plan, cur.g_end, next_rank);
      ms.launch(k_pack_marked, next, half ^ 1);
    }
    wait_marked_event(ms.done[half]);
    const int status =
        sink(ms.staging + half * ms.half_bytes, cur.first_rank, cur.count);
    if (status != 0) return status;
    *packed = next_rank;
    if (next_rank >= plan.marked) return kIoOk;
    cur = next;
  }
}

int marked_gpu(MarkedStream& ms, const MarkedPlan& plan,
               const UnpackSource& source, uint64_t* unpacked) {
  bool used[2] = {false, false};
  uint64_t g_begin = 0;
  uint64_t launched = 0;
  for (int half = 0; launched < plan.marked; half ^= 1) {
    const MarkedWindow win = next_marked_window(plan, g_begin, launched);
    // The kernel two windows back read this half: let it finish first.
    if (used[half]) wait_marked_event(ms.done[half]);
    const int status =
        source(ms.staging + half * ms.half_bytes, win.first_rank, win.count);
    if (status != 0) {
      HIP_CHECK(hipStreamSynchronize(ms.stream));
      *unpacked = launched;
      return status;
    }
    ms.launch(k_unpack_marked, win, half);
    used[half] = true;
    launched += win.count;
    g_begin = win.g_end;
  }
  HIP_CHECK(hipStreamSynchronize(ms.stream));
  *unpacked = launched;
  return kIoOk;
}

// Generic path: the same chunks, filled from (or drained to) runs of
// marked granules in spans of at most 1 MiB.
template <typename Chunk>
int marked_generic(Bdev* bdev, uint64_t offset, uint32_t granule,
                   const MarkedPlan& plan, bool pack, const Chunk& chunk,
                   uint64_t* moved) {
  uint8_t* buf = bulk_ctx().staging.reserve(plan.chunk_granules * granule);
  const uint64_t span = host_chunk_bytes(bdev);
  RunCursor runs{plan};
  for (uint64_t first_rank = 0; first_rank < plan.marked;) {
    const uint64_t count =
        std::min(plan.chunk_granules, plan.marked - first_rank);
    if (!pack) {
      const int status = chunk(buf, first_rank, count);
      if (status != 0) return status;
    }
    uint64_t g = 0;
    uint64_t len = 0;
    // `count` marks are left, so the cursor cannot run dry in here.
    for (uint64_t filled = 0;
         filled < count && runs.next(count - filled, &g, &len);
         filled += len) {
      const uint64_t bytes = len * granule;
      for (uint64_t pos = 0; pos < bytes; pos += span) {
        const uint64_t n = std::min(span, bytes - pos);
        uint8_t* p = buf + filled * granule + pos;
        const uint64_t at = offset + g * granule + pos;
        const int status = pack ? bdev_read_sync(bdev, at, p, n)
                                : bdev_write_sync(bdev, at, p, n);
        if (status != kIoOk) return status;
      }
    }
    if (pack) {
      const int status = chunk(buf, first_rank, count);
      if (status != 0) return status;
    }
    first_rank += count;
    *moved = first_rank;
  }
  return kIoOk;
}

// bdev_pack_marked_sync (Chunk = PackSink) and bdev_unpack_marked_sync
// (Chunk = UnpackSource): validate, plan, return early on nothing to
// do, then stream the marked granules on the GPU or generic path.
template <typename Chunk>
int marked_stream_sync(Bdev* bdev, uint64_t offset, uint64_t length,
                       uint32_t granule, const std::vector<uint64_t>& bitmap,
                       uint64_t staging_bytes, const Chunk& chunk,
                       uint64_t* moved_out) {
  uint64_t unused = 0;
  uint64_t* moved = moved_out != nullptr ? moved_out : &unused;
  *moved = 0;
  try {
    if (!granule_ranges_ok(bdev, offset, bdev, offset, length, granule,
                           &bitmap) ||
        (staging_bytes != 0 && staging_bytes < granule)) {
      return kIoInvalid;
    }
    MarkedPlan plan = build_marked_plan(length / granule, bitmap, true);
    if (plan.marked == 0) return kIoOk;
    if (!chunk) return kIoInvalid;
    const uint64_t half =
        staging_bytes == 0 ? kDefaultStagingHalf : staging_bytes / 2;
    plan.chunk_granules =
        std::min(std::max<uint64_t>(1, half / granule), plan.marked);
    const int device = granule_kernel_device(bdev, bdev);
    if (device >= 0) {
      MarkedStream ms(device, bdev, offset, granule, plan);
      return marked_gpu(ms, plan, chunk, moved);
    }
    return marked_generic(bdev, offset, granule, plan,
                          std::is_same<Chunk, PackSink>::value, chunk, moved);
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

}  // namespace

int bdev_pack_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                          uint32_t granule,
                          const std::vector<uint64_t>& bitmap,
                          uint64_t staging_bytes, const PackSink& sink,
                          uint64_t* packed) {
  return marked_stream_sync(src, src_offset, length, granule, bitmap,
                            staging_bytes, sink, packed);
}

int bdev_unpack_marked_sync(Bdev* dst, uint64_t dst_offset, uint64_t length,
                            uint32_t granule,
                            const std::vector<uint64_t>& bitmap,
                            uint64_t staging_bytes,
                            const UnpackSource& source, uint64_t* unpacked) {
  return marked_stream_sync(dst, dst_offset, length, granule, bitmap,
                            staging_bytes, source, unpacked);
}

// ---------------------------------------------------------------------------
// Granule fingerprints
// ---------------------------------------------------------------------------

namespace {

uint32_t fingerprint_grid(uint64_t n_granules) {
  return static_cast<uint32_t>(std::min<uint64_t>(
      (n_granules + kWavesPerWg - 1) / kWavesPerWg, 2048));
}

// One launch per window of `window` granules, fingerprints written in
// place into one half of `prints`; window k+1 runs while the sink sees
// window k.
int fingerprint_gpu(int device, Bdev* bdev, uint64_t offset,
                    uint64_t n_granules, uint32_t granule, uint64_t window,
                    const FingerprintSink& sink, uint64_t* done) {
  HalvesStream hs(device);
  const uint64_t half_bytes = window * kFingerprintBytes;
  uint8_t* prints = bulk_ctx().prints.reserve(2 * half_bytes);
  uint8_t* dev_prints = device_view(prints);
  const uint8_t* base = static_cast<uint8_t*>(bdev->device_base()) + offset;
  auto launch = [&](uint64_t first, int half) {
    const uint64_t count = std::min(window, n_granules - first);  // >= 1
    hipLaunchKernelGGL(k_fingerprint_granules, dim3(fingerprint_grid(count)),
                       dim3(kWavesPerWg * 64), 0, hs.stream,
                       base + first * granule, count, granule,
                       reinterpret_cast<uint4*>(dev_prints + half * half_bytes));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(hs.done[half], hs.stream));
  };
  launch(0, 0);
  for (int half = 0;; half ^= 1) {
    const uint64_t first = *done;
    const uint64_t count = std::min(window, n_granules - first);
    if (first + count < n_granules) launch(first + count, half ^ 1);
    wait_marked_event(hs.done[half]);
    const int status = sink(prints + half * half_bytes, first, count);
    if (status != 0) return status;
    *done = first + count;
    if (*done >= n_granules) return kIoOk;
  }
}

// Generic path: the same windows, read in spans of at most 1 MiB through
// the incremental hasher (a granule may be larger than a span).
int fingerprint_generic(Bdev* bdev, uint64_t offset, uint64_t n_granules,
                        uint32_t granule, uint64_t window,
                        const FingerprintSink& sink, uint64_t* done) {
  // Spans are cut on multiples of the block size and of 16.
  const uint64_t unit = std::lcm<uint64_t>(bdev->block_size(), 16);
  const uint64_t span = kDiffHostChunk / unit * unit;
  if (span == 0) return kIoInvalid;
  uint8_t* prints = bulk_ctx().prints.reserve(window * kFingerprintBytes);
  uint8_t* buf = bulk_ctx().chunks.reserve(2 * kDiffHostChunk);
  GranuleHasher hasher;
  while (*done < n_granules) {
    const uint64_t first = *done;
    const uint64_t count = std::min(window, n_granules - first);
    const uint64_t bytes = count * granule;
    uint64_t in_granule = 0;  // bytes of the current granule hashed so far
    uint64_t filled = 0;      // granules of this window finished
    for (uint64_t pos = 0; pos < bytes; pos += span) {
      const uint64_t n = std::min(span, bytes - pos);
      const int status =
          bdev_read_sync(bdev, offset + first * granule + pos, buf, n);
      if (status != kIoOk) return status;
      for (uint64_t off = 0; off < n;) {
        const uint64_t piece = std::min<uint64_t>(granule - in_granule, n - off);
        hasher.update(buf + off, piece);
        off += piece;
        in_granule += piece;
        if (in_granule == granule) {
          hasher.finish(prints + filled * kFingerprintBytes);
          ++filled;
          in_granule = 0;
        }
      }
    }
    const int status = sink(prints, first, count);
    if (status != 0) return status;
    *done = first + count;
  }
  return kIoOk;
}

}  // namespace

int bdev_fingerprint_sync(Bdev* bdev, uint64_t offset, uint64_t length,
                          uint32_t granule, uint64_t staging_bytes,
                          const FingerprintSink& sink, uint64_t* done_out) {
  uint64_t unused = 0;
  uint64_t* done = done_out != nullptr ? done_out : &unused;
  *done = 0;
  try {
    if (!granule_ranges_ok(bdev, offset, bdev, offset, length, granule) ||
        (staging_bytes != 0 && staging_bytes < 2 * kFingerprintBytes) ||
        !sink) {
      return kIoInvalid;
    }
    const uint64_t n_granules = length / granule;  // >= 1
    const uint64_t half =
        staging_bytes == 0 ? kDefaultStagingHalf : staging_bytes / 2;
    const uint64_t window =
        std::min(std::max<uint64_t>(1, half / kFingerprintBytes), n_granules);
    const int device = granule_kernel_device(bdev, bdev);
    if (device >= 0) {
      return fingerprint_gpu(device, bdev, offset, n_granules, granule, window,
                             sink, done);
    }
    return fingerprint_generic(bdev, offset, n_granules, granule, window, sink,
                               done);
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

// Measurement aid (tools/delta_bench.py): times, on the host clock from
// the first enqueue to the end of a stream synchronise, what moves the
// marked bytes of an HBM bdev to pinned host memory.
//   mode 0: hipMemcpyAsync of the same byte count from the start of the
//           volume, in pieces as large as the pinned buffer (PCIe ceiling)
//   mode 1: one hipMemcpyAsync per run of marked granules (what
//           k_pack_marked replaces)
//   mode 2: bdev_pack_marked_sync with a sink that discards
// Modes 0 and 1 land in a pinned ring of at most `ring_bytes`; a run
// that would cross its end is split there.
int marked_copy_probe(Bdev* src, uint32_t granule,
                      const std::vector<uint64_t>& bitmap, int mode,
                      uint64_t ring_bytes, uint64_t staging_bytes,
                      MarkedCopyProbe* out) {
  using clock = std::chrono::steady_clock;
  *out = MarkedCopyProbe{};
  if (src == nullptr || mode < 0 || mode > 2) return kIoInvalid;
  const uint64_t length = src->size_bytes() / std::max(granule, 1u) * granule;
  if (mode == 2) {
    const auto t0 = clock::now();
    const int status = bdev_pack_marked_sync(
        src, 0, length, granule, bitmap, staging_bytes,
        [out](const uint8_t*, uint64_t, uint64_t) {
          ++out->calls;
          return 0;
        },
        &out->granules);
    out->seconds = std::chrono::duration<double>(clock::now() - t0).count();
    return status;
  }
  try {
    if (!granule_ranges_ok(src, 0, src, 0, length, granule, &bitmap)) {
      return kIoInvalid;
    }
    const MarkedPlan plan = build_marked_plan(length / granule, bitmap, false);
    const int device = granule_kernel_device(src, src);
    if (device < 0 || plan.marked == 0 || ring_bytes < granule) {
      return kIoInvalid;
    }
    const uint64_t total = plan.marked * granule;
    const uint64_t ring = std::min(ring_bytes / granule * granule, total);
    HIP_CHECK(hipSetDevice(device));
    // The ring outlives the stream: declared first, released last.
    PinnedBuf<uint8_t> ring_buf;
    uint8_t* pinned = ring_buf.reserve(ring);
    memset(pinned, 0, ring);  // touch every page before the clock starts
    ScopedStream ss(device);
    const uint8_t* base = static_cast<uint8_t*>(src->device_base());
    uint64_t at = 0;  // write position in the ring
    auto copy = [&](uint64_t from, uint64_t bytes) {
      while (bytes > 0) {
        const uint64_t n = std::min(bytes, ring - at);
        HIP_CHECK(hipMemcpyAsync(pinned + at, base + from, n,
                                 hipMemcpyDeviceToHost, ss.stream));
        ++out->calls;
        at = (at + n) % ring;
        from += n;
        bytes -= n;
      }
    };
    const auto t0 = clock::now();
    if (mode == 0) {
      copy(0, total);
    } else {
      RunCursor runs{plan};
      uint64_t g = 0;
      uint64_t len = 0;
      while (runs.next(UINT64_MAX, &g, &len)) copy(g * granule, len * granule);
    }
    HIP_CHECK(hipStreamSynchronize(ss.stream));
    out->seconds = std::chrono::duration<double>(clock::now() - t0).count();
    out->granules = plan.marked;
    return kIoOk;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

}  // namespace hipstore
