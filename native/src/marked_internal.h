// Private to native/src: what the calls that walk a bitmap of marked
// granules window by window have in common. bulk_ops.hip (pack / unpack)
// defines the functions; compress_ops.hip (LZ compress / decompress)
// uses them, so both cut the same windows from the same plan.
#pragma once

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
