// Private to native/src: what the calls that walk a bitmap of marked
// granules window by window have in common. bulk_ops.hip (pack / unpack)
// defines the functions; compress_ops.hip (LZ compress / decompress) and
// crypt_ops.hip (XTS pack / unpack) use them, so all cut the same windows
// from the same plan, and share the wave-per-granule walk below.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "gpu_internal.h"

namespace hipstore {

// One window [g_begin, g_end) of a range; see k_pack_marked.
struct MarkedWindow {
  uint64_t g_begin;
  uint64_t g_end;
  uint32_t first_rank;  // marked granules before g_begin
  uint32_t count;       // marked granules in the window
};

// What every call that takes a bitmap works from: the pinned copy of
// the caller's bitmap with stray tail bits cleared (the kernels read it
// in place), the number of marks, and, when asked for, the exclusive
// prefix popcount that the window kernels read. `chunk_granules` belongs
// to the windowed calls, which set it.
struct MarkedPlan {
  uint64_t n_granules = 0;
  uint64_t n_words = 0;
  uint64_t marked = 0;
  uint64_t chunk_granules = 0;
  unsigned long long* words = nullptr;
  uint32_t* ranks = nullptr;
};

constexpr uint64_t kDefaultStagingHalf = 16ull << 20;

// Shared validation; one bdev is the pair (bdev, bdev). A call that
// takes a bitmap passes it: it must cover the range.
bool granule_ranges_ok(Bdev* a, uint64_t a_offset, Bdev* b, uint64_t b_offset,
                       uint64_t length, uint32_t granule,
                       const std::vector<uint64_t>* bitmap = nullptr);

// Device the pair's kernels run on, or -1 for the generic path.
int granule_kernel_device(Bdev* a, Bdev* b);

// Workgroups for `n_granules` granules, one bitmap word each, at most 2048.
uint32_t granule_grid(uint64_t n_granules);

// `bitmap` holds at least ceil(n_granules / 64) words (granule_ranges_ok).
// The plan lives in the calling thread's pinned buffers until that
// thread builds the next one.
MarkedPlan build_marked_plan(uint64_t n_granules,
                             const std::vector<uint64_t>& bitmap,
                             bool want_ranks);

// The window that starts at granule `g_begin` and holds the next
// min(chunk, marks left) marked granules: it ends right after the last
// of them.
MarkedWindow next_marked_window(const MarkedPlan& plan, uint64_t g_begin,
                                uint64_t first_rank);

// Polls briefly, then sleeps; throws on a failed stream.
void wait_marked_event(hipEvent_t event);

inline uint32_t marked_window_grid(const MarkedWindow& win) {
  return granule_grid((win.g_end + 63) / 64 * 64 - win.g_begin / 64 * 64);
}

// Internal linkage because its base is (gpu_internal.h gives every
// translation unit its own ScopedStream).
namespace {

__device__ __forceinline__ uint32_t uniform(uint32_t v) {
  return __builtin_amdgcn_readfirstlane(v);
}

// fn(granule index, window slot) once per marked granule of the window,
// by one wave. Unlike marked_window_walk (bulk_ops.hip), which gives a
// workgroup a whole bitmap word, this walk gives every granule of the
// window's words a wave of its own, grid-stride: a 16 MiB window of
// 4 KiB granules is 64 words, and 64 workgroups leave most of the chip
// idle under kernels that are bound by arithmetic or by the latency of a
// serial parse, not by bandwidth (compress_ops.hip, crypt_ops.hip). The
// slot is the same pure function of the bitmap and rank_before_word.
template <typename Fn>
__device__ __forceinline__ void wave_window_walk(
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, const MarkedWindow win,
    Fn fn) {
  const uint32_t n_waves = blockDim.x >> 6;
  const uint64_t g_first = win.g_begin & ~63ull;
  const uint64_t span = ((win.g_end + 63) & ~63ull) - g_first;
  for (uint64_t v = static_cast<uint64_t>(blockIdx.x) * n_waves +
                    uniform(threadIdx.x >> 6);
       v < span; v += static_cast<uint64_t>(gridDim.x) * n_waves) {
    const uint64_t g = g_first + v;  // wave-uniform, like all below
    if (g < win.g_begin || g >= win.g_end) continue;
    const unsigned long long word = bitmap[g >> 6];
    const uint32_t bit = static_cast<uint32_t>(g & 63);
    if (((word >> bit) & 1) == 0) continue;
    const uint32_t slot =
        uniform(rank_before_word[g >> 6]) - win.first_rank +
        static_cast<uint32_t>(__popcll(word & ((1ull << bit) - 1)));
    if (slot >= win.count) continue;  // bitmap and ranks disagree: stay inside
    fn(g, slot);
  }
}

// Workgroups of `waves` waves for wave_window_walk: a wave per granule of
// the window's bitmap words, at most 2048.
inline uint32_t wave_window_grid(const MarkedWindow& win, uint32_t waves) {
  const uint64_t span = (win.g_end + 63) / 64 * 64 - win.g_begin / 64 * 64;
  return static_cast<uint32_t>(
      std::min<uint64_t>((span + waves - 1) / waves, 2048));
}

// A one-shot stream with one event per half of a two-half pinned
// buffer: the window loops launch into one half while the host works on
// the other.
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

}  // namespace

}  // namespace hipstore
