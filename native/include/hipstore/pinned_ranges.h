// Process-wide registry of pinned host ranges and their device views.
//
// The HBM engines put device-visible buffer addresses into their tile
// descriptors. Asking the runtime for each one (hipHostGetDevicePointer)
// takes the runtime's lock per tile, and submitter threads convoy on it.
// Everything the process pins itself (alloc_pinned, registered vhost
// guest memory) is recorded here instead as (host base, length, device
// base), and a submitter translates from the range it hit last:
//
//   - writers (add/remove) take the mutex and bump a generation counter;
//   - a reader keeps a PinnedRangeCache of its own (one per channel) and
//     revalidates it with one relaxed load of the generation. Only a
//     changed generation or a buffer outside the cached range takes the
//     mutex;
//   - a buffer in no registered range goes to the caller's fallback
//     resolver, whose answer is never cached.
//
// A translation holds only while the range stays registered, which is
// the caller's contract already: a buffer must not be freed under an
// I/O that names it. Whoever frees and whoever next submits are ordered
// by whatever handed the address from one to the other, and that order
// is enough for the relaxed generation load to see the removal.
//
// Plain C++ on purpose, no HIP: the resolver is passed in, so this
// header compiles and is tested without a GPU.

#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>

namespace hipstore {

struct PinnedRange {
  uintptr_t host = 0;
  size_t length = 0;
  uintptr_t device = 0;

  // Whether [p, p + bytes) lies inside the range; subtraction only, so
  // nothing wraps.
  bool holds(uintptr_t p, size_t bytes) const {
    return p >= host && bytes <= length && p - host <= length - bytes;
  }
};

// A reader's remembered range. generation 0 never matches the registry.
struct PinnedRangeCache {
  PinnedRange range;
  uint64_t generation = 0;
};

class PinnedRangeRegistry {
 public:
  // Record [host, host + length) as visible to the device at `device`.
  // A range already recorded at `host` is replaced.
  void add(const void* host, size_t length, const void* device) {
    if (host == nullptr || length == 0) return;
    std::lock_guard<std::mutex> lock(mutex_);
    PinnedRange& r = ranges_[reinterpret_cast<uintptr_t>(host)];
    r.host = reinterpret_cast<uintptr_t>(host);
    r.length = length;
    r.device = reinterpret_cast<uintptr_t>(device);
    bump();
  }

  // Forget the range recorded at `host`; call BEFORE the memory is
  // unpinned, so that the address cannot be handed out and recorded
  // again in between. Returns false if none was recorded.
  bool remove(const void* host) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (ranges_.erase(reinterpret_cast<uintptr_t>(host)) == 0) return false;
    bump();
    return true;
  }

  size_t size() const {
    std::lock_guard<std::mutex> lock(mutex_);
    return ranges_.size();
  }

  // Device address of the `bytes`-long buffer at `host`. `fallback(host)`
  // resolves (or throws for) a buffer that no single registered range
  // holds entirely.
  template <typename Fallback>
  void* translate(PinnedRangeCache& cache, void* host, size_t bytes,
                  Fallback&& fallback) const {
    const uintptr_t p = reinterpret_cast<uintptr_t>(host);
    if (cache.generation == generation_.load(std::memory_order_relaxed) &&
        cache.range.holds(p, bytes)) {
      return reinterpret_cast<void*>(cache.range.device +
                                     (p - cache.range.host));
    }
    if (find(p, bytes, &cache)) {
      return reinterpret_cast<void*>(cache.range.device +
                                     (p - cache.range.host));
    }
    return fallback(host);
  }

 private:
  // Under the mutex: the range holding [p, p + bytes), remembered in
  // `cache` together with the generation it belongs to.
  bool find(uintptr_t p, size_t bytes, PinnedRangeCache* cache) const {
    std::lock_guard<std::mutex> lock(mutex_);
    auto it = ranges_.upper_bound(p);  // first range that starts past p
    if (it == ranges_.begin()) return false;
    --it;
    if (!it->second.holds(p, bytes)) return false;
    cache->range = it->second;
    cache->generation = generation_.load(std::memory_order_relaxed);
    return true;
  }

  void bump() {
    generation_.store(generation_.load(std::memory_order_relaxed) + 1,
                      std::memory_order_release);
  }

  mutable std::mutex mutex_;
  std::map<uintptr_t, PinnedRange> ranges_;  // by host base; disjoint
  std::atomic<uint64_t> generation_{1};
};

// The one registry of the process. Never destroyed: buffers are freed
// from static destructors and detached threads too.
inline PinnedRangeRegistry& pinned_ranges() {
  static PinnedRangeRegistry* const registry = new PinnedRangeRegistry;
  return *registry;
}

}  // namespace hipstore
