// Private to native/src: the window core of the calls that walk a bitmap
// of marked granules window by window: validation and plan, the windows,
// the stream with its two staging halves, the pack-ahead and unpack
// loops, the wave-per-granule walk of the kernels and the host cursor of
// the generic paths. bulk_ops.hip (pack / unpack) defines the functions;
// compress_ops.hip (LZ compress / decompress) and crypt_ops.hip (XTS pack
// / unpack) use them, so all cut the same windows from the same plan and
// run the same loops.
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

// Validation, plan and chunk size of every windowed call over one bdev:
// kIoInvalid unless granule_ranges_ok and staging_bytes is 0 or at least
// a granule, then the plan with ranks. kIoOk with plan->marked == 0 means
// nothing to do; marks without a callback are kIoInvalid. A half of the
// staging holds chunk_granules granules: half of staging_bytes (16 MiB
// for 0), at least one granule, at most all the marked ones.
int plan_marked_windows(Bdev* bdev, uint64_t offset, uint64_t length,
                        uint32_t granule, const std::vector<uint64_t>& bitmap,
                        uint64_t staging_bytes, bool have_callback,
                        MarkedPlan* plan);

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

// What every call that reports its progress starts with: `moved_out` may
// be null, the count starts at 0, and whatever body(moved) throws (a
// failed HIP call, an allocation) is kIoFailed.
template <typename Body>
int marked_call(uint64_t* moved_out, Body body) {
  uint64_t unused = 0;
  uint64_t* moved = moved_out != nullptr ? moved_out : &unused;
  *moved = 0;
  try {
    return body(moved);
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

// The marked granules of a range in ascending order, for the generic
// paths of the codecs: their chunks arrive in that order and need the
// index of every granule (its unit number, its dictionary). Stray bits
// past the range are masked, as in the plan.
struct MarkCursor {
  const std::vector<uint64_t>& bitmap;
  uint64_t n_granules;
  uint64_t w = 0;
  uint64_t word = 0;
  bool loaded = false;

  // The caller takes no more granules than the range has marks.
  uint64_t next() {
    for (;; ++w, loaded = false) {
      if (!loaded) {
        word = bitmap[w];
        const uint64_t left = n_granules - w * 64;
        if (left < 64) word &= (1ull << left) - 1;
        loaded = true;
      }
      if (word != 0) break;
    }
    const uint64_t g = w * 64 + static_cast<uint64_t>(__builtin_ctzll(word));
    word &= word - 1;
    return g;
  }
};

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

// What the GPU window loops of a call run on. One stream and one event
// per staging half; the kernels read the plan and fill or drain the two
// halves of the caller's pinned `staging` in place, so the device's view
// of those is kept here too.
struct WindowStream : HalvesStream {
  uint32_t granule;
  uint64_t half_bytes;
  uint8_t* staging;
  uint8_t* dev_staging;
  const unsigned long long* dev_words;
  const uint32_t* dev_ranks;
  uint8_t* base;  // the bdev's range in device memory

  WindowStream(int device, Bdev* bdev, uint64_t offset, uint32_t granule_bytes,
               const MarkedPlan& plan, PinnedBuf<uint8_t>& staging_buf)
      : HalvesStream(device), granule(granule_bytes),
        half_bytes(plan.chunk_granules * granule_bytes),
        staging(staging_buf.reserve(2 * half_bytes)),
        dev_staging(device_view(staging)), dev_words(device_view(plan.words)),
        dev_ranks(device_view(plan.ranks)),
        base(static_cast<uint8_t*>(bdev->device_base()) + offset) {}

  uint8_t* half_of(int half) const { return staging + half * half_bytes; }

  // After a launch: its error, then `event` behind it on the stream.
  void record(hipEvent_t event) {
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(event, stream));
  }

  // A kernel with k_pack_marked's leading arguments over one window and
  // one half; `tail` are the arguments after the granule size.
  template <typename Kernel, typename... Tail>
  void launch(Kernel kernel, uint32_t grid, uint32_t threads,
              const MarkedWindow& win, int half, const Tail&... tail) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), 0, stream, base,
                       dev_staging + half * half_bytes, dev_words, dev_ranks,
                       win, granule, tail...);
    record(done[half]);
  }
};

// Pack side. launch(win, half) queues the kernel that starts window `win`
// in `half`; finish(win, half) queues whatever the window still needs once
// that kernel is on the stream, the last of it recording done[half] (a
// call whose launch does that has nothing to finish);
// deliver(win, half) hands the finished half on and returns 0 to go on.
// Window k+1 is launched before window k is waited for, so the GPU works
// while the host has the other half.
template <typename Launch, typename Finish, typename Deliver>
int pack_windows(HalvesStream& hs, const MarkedPlan& plan, Launch launch,
                 Finish finish, Deliver deliver, uint64_t* packed) {
  MarkedWindow cur = next_marked_window(plan, 0, 0);
  launch(cur, 0);
  for (int half = 0;; half ^= 1) {
    const uint64_t next_rank = cur.first_rank + static_cast<uint64_t>(cur.count);
    finish(cur, half);
    MarkedWindow next{};
    if (next_rank < plan.marked) {
      next = next_marked_window(plan, cur.g_end, next_rank);
      launch(next, half ^ 1);
    }
    wait_marked_event(hs.done[half]);
    const int status = deliver(cur, half);
    if (status != 0) return status;
    *packed = next_rank;
    if (next_rank >= plan.marked) return kIoOk;
    cur = next;
  }
}

// Unpack side. fetch(win, half) fills `half` for window `win` and returns
// 0 to go on; launch(win, half) queues its kernels, the last recording
// done[half]. Before a half is filled again the kernel two windows back,
// which read it, has finished, and reuse(half) says whether to go on
// after it. `unpacked` counts the granules of the windows launched; every
// way out waits for them.
template <typename Reuse, typename Fetch, typename Launch>
int unpack_windows(HalvesStream& hs, const MarkedPlan& plan, Reuse reuse,
                   Fetch fetch, Launch launch, uint64_t* unpacked) {
  bool used[2] = {false, false};
  uint64_t g_begin = 0;
  uint64_t launched = 0;
  int status = kIoOk;
  for (int half = 0; launched < plan.marked; half ^= 1) {
    const MarkedWindow win = next_marked_window(plan, g_begin, launched);
    if (used[half]) {
      wait_marked_event(hs.done[half]);
      status = reuse(half);
      if (status != kIoOk) break;
    }
    status = fetch(win, half);
    if (status != kIoOk) break;
    launch(win, half);
    used[half] = true;
    launched += win.count;
    g_begin = win.g_end;
  }
  HIP_CHECK(hipStreamSynchronize(hs.stream));
  *unpacked = launched;
  return status;
}

}  // namespace

}  // namespace hipstore
