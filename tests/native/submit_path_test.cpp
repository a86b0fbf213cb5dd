// Stand-alone checks of the two lock-free pieces of the submit path:
// the pinned-range registry (hipstore/pinned_ranges.h) and the sharded
// I/O statistics of Bdev (hipstore/bdev.h). No GPU and no HIP: the
// registry's fallback resolver is a function of this file. Built plain
// and with -fsanitize=thread by `make submit-path-test`; exits non-zero
// on the first failed check.

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>
#include <vector>

#include "hipstore/bdev.h"
#include "hipstore/pinned_ranges.h"

using hipstore::PinnedRangeCache;
using hipstore::PinnedRangeRegistry;

namespace {

int g_failures = 0;

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_failures;                                                     \
    }                                                                   \
  } while (0)

// Addresses are never dereferenced: the registry only does arithmetic.
void* addr(uintptr_t v) { return reinterpret_cast<void*>(v); }
uintptr_t val(void* p) { return reinterpret_cast<uintptr_t>(p); }

// The fallback marks its answers: host + kFallbackBias.
constexpr uintptr_t kFallbackBias = uintptr_t{1} << 60;
std::atomic<uint64_t> g_fallback_calls{0};
void* fallback(void* host) {
  g_fallback_calls.fetch_add(1, std::memory_order_relaxed);
  return addr(val(host) + kFallbackBias);
}
void* pageable(void*) { throw std::runtime_error("not pinned"); }

void test_hit_miss_remove() {
  PinnedRangeRegistry reg;
  PinnedRangeCache cache;
  reg.add(addr(0x10000), 0x4000, addr(0x900000));
  CHECK(reg.size() == 1);
  // hit: first, last and inner tile
  CHECK(val(reg.translate(cache, addr(0x10000), 4096, fallback)) == 0x900000);
  CHECK(val(reg.translate(cache, addr(0x13000), 4096, fallback)) == 0x903000);
  CHECK(val(reg.translate(cache, addr(0x10010), 16, fallback)) == 0x900010);
  const uint64_t before = g_fallback_calls.load();
  CHECK(val(reg.translate(cache, addr(0x11000), 4096, fallback)) == 0x901000);
  CHECK(g_fallback_calls.load() == before);
  // miss: below, above, and in an empty registry's neighbourhood
  CHECK(val(reg.translate(cache, addr(0xF000), 4096, fallback)) ==
        0xF000 + kFallbackBias);
  CHECK(val(reg.translate(cache, addr(0x14000), 4096, fallback)) ==
        0x14000 + kFallbackBias);
  CHECK(g_fallback_calls.load() == before + 2);
  // the fallback's error reaches the caller
  bool threw = false;
  try {
    reg.translate(cache, addr(0x20000), 4096, pageable);
  } catch (const std::runtime_error&) {
    threw = true;
  }
  CHECK(threw);
  // a miss does not spoil the remembered range
  CHECK(val(reg.translate(cache, addr(0x12000), 4096, fallback)) == 0x902000);
  // removal: the remembered entry must not answer any more
  CHECK(reg.remove(addr(0x10000)));
  CHECK(!reg.remove(addr(0x10000)));
  CHECK(reg.size() == 0);
  CHECK(val(reg.translate(cache, addr(0x12000), 4096, fallback)) ==
        0x12000 + kFallbackBias);
}

void test_reregistration_through_cache() {
  PinnedRangeRegistry reg;
  PinnedRangeCache cache;
  reg.add(addr(0x40000), 0x2000, addr(0xA00000));
  CHECK(val(reg.translate(cache, addr(0x41000), 4096, fallback)) == 0xA01000);
  // freed and handed out again at the same host address, other view
  reg.remove(addr(0x40000));
  reg.add(addr(0x40000), 0x2000, addr(0xB00000));
  CHECK(val(reg.translate(cache, addr(0x41000), 4096, fallback)) == 0xB01000);
  // replaced in place, shorter: the old length must not answer either
  reg.add(addr(0x40000), 0x1000, addr(0xC00000));
  CHECK(val(reg.translate(cache, addr(0x40000), 4096, fallback)) == 0xC00000);
  CHECK(val(reg.translate(cache, addr(0x41000), 4096, fallback)) ==
        0x41000 + kFallbackBias);
}

void test_touching_ranges_and_straddling_tile() {
  PinnedRangeRegistry reg;
  PinnedRangeCache cache;
  // [0x50000, 0x52000) and [0x52000, 0x53000): touch, do not overlap,
  // and their device views are unrelated.
  reg.add(addr(0x50000), 0x2000, addr(0xD00000));
  reg.add(addr(0x52000), 0x1000, addr(0x100000));
  CHECK(val(reg.translate(cache, addr(0x51000), 4096, fallback)) == 0xD01000);
  CHECK(val(reg.translate(cache, addr(0x52000), 4096, fallback)) == 0x100000);
  CHECK(val(reg.translate(cache, addr(0x51FF0), 16, fallback)) == 0xD01FF0);
  CHECK(val(reg.translate(cache, addr(0x52FF0), 16, fallback)) == 0x100FF0);
  // A tile that starts in the first range and ends in the second: not
  // the first range's arithmetic, whichever range is remembered.
  CHECK(val(reg.translate(cache, addr(0x51000), 4096, fallback)) == 0xD01000);
  CHECK(val(reg.translate(cache, addr(0x51800), 4096, fallback)) ==
        0x51800 + kFallbackBias);
  CHECK(val(reg.translate(cache, addr(0x52000), 4096, fallback)) == 0x100000);
  CHECK(val(reg.translate(cache, addr(0x51800), 4096, fallback)) ==
        0x51800 + kFallbackBias);
  // ... and one that would end past the last range
  CHECK(val(reg.translate(cache, addr(0x52800), 4096, fallback)) ==
        0x52800 + kFallbackBias);
  // lengths that would wrap the address space
  CHECK(val(reg.translate(cache, addr(0x52000), ~size_t{0}, fallback)) ==
        0x52000 + kFallbackBias);
}

// Eight readers, each with a cache of its own, while one writer
// removes and re-records a range with a new device base every time.
// The writer announces the base that currently holds (0 while it is
// changing it); a reader that saw the same non-zero announcement before
// and after a lookup must have got exactly that base. Stable ranges on
// both sides of the churned one must always translate.
void test_concurrent_lookup() {
  PinnedRangeRegistry reg;
  constexpr uintptr_t kStableLo = 0x100000, kChurn = 0x200000,
                      kStableHi = 0x300000, kLen = 0x10000;
  reg.add(addr(kStableLo), kLen, addr(0x7000000));
  reg.add(addr(kStableHi), kLen, addr(0x8000000));
  std::atomic<uintptr_t> announced{0};
  std::atomic<bool> stop{false};
  std::atomic<uint64_t> wrong{0}, verified{0};

  std::vector<std::thread> readers;
  for (int r = 0; r < 8; ++r) {
    readers.emplace_back([&, r] {
      PinnedRangeCache cache;
      uint64_t i = r;
      while (!stop.load(std::memory_order_acquire)) {
        const uintptr_t off = (i++ % 15) * 4096;
        if (val(reg.translate(cache, addr(kStableLo + off), 4096, fallback)) !=
            0x7000000 + off) {
          wrong.fetch_add(1);
        }
        const uintptr_t e1 = announced.load(std::memory_order_acquire);
        const uintptr_t got =
            val(reg.translate(cache, addr(kChurn + off), 4096, fallback));
        const uintptr_t e2 = announced.load(std::memory_order_acquire);
        if (e1 != 0 && e1 == e2) {
          if (got != e1 + off) wrong.fetch_add(1);
          verified.fetch_add(1, std::memory_order_relaxed);
        }
        if (val(reg.translate(cache, addr(kStableHi + off), 4096, fallback)) !=
            0x8000000 + off) {
          wrong.fetch_add(1);
        }
      }
    });
  }
  // Every device base is used once, so an equal announcement before
  // and after a lookup means nothing changed in between.
  uintptr_t base = uintptr_t{1} << 40;
  for (int round = 0; round < 20000; ++round) {
    base += 0x100000;
    reg.add(addr(kChurn), kLen, addr(base));
    announced.store(base, std::memory_order_release);
    if (round % 64 == 0) std::this_thread::yield();
    announced.store(0, std::memory_order_release);
    reg.remove(addr(kChurn));
  }
  stop.store(true, std::memory_order_release);
  for (auto& t : readers) t.join();
  CHECK(wrong.load() == 0);
  CHECK(verified.load() > 0);
  CHECK(reg.size() == 2);
  printf("concurrent lookup: %llu verified against the writer\n",
         static_cast<unsigned long long>(verified.load()));
}

// Bdev::account() from eight threads: the totals are exact.
class CountingBdev : public hipstore::Bdev {
 public:
  CountingBdev() : Bdev("count", "test", 512, 1 << 20) {}
  std::shared_ptr<hipstore::IoChannel> get_channel() override { return {}; }
  void submit(hipstore::IoChannel*, hipstore::IoRequest req) override {
    account(req);
  }
  int poll(hipstore::IoChannel*) override { return 0; }
};

void test_sharded_iostat() {
  auto bdev = std::make_shared<CountingBdev>();
  CHECK(reinterpret_cast<uintptr_t>(bdev.get()) % 64 == 0);
  constexpr int kThreads = 8, kRequests = 100000;
  struct Sum {
    uint64_t reads = 0, writes = 0, unmaps = 0, rbytes = 0, wbytes = 0;
  };
  std::vector<Sum> sums(kThreads);
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t) {
    threads.emplace_back([&, t] {
      uint64_t x = 0x9E3779B97F4A7C15ull * (t + 1);
      Sum& mine = sums[t];
      for (int i = 0; i < kRequests; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        hipstore::IoRequest req;
        req.op = static_cast<hipstore::IoOp>(x & 3);
        req.length = 512 * (1 + ((x >> 8) % 2048));  // 512 B .. 1 MiB
        switch (req.op) {
          case hipstore::IoOp::kRead:
            ++mine.reads; mine.rbytes += req.length; break;
          case hipstore::IoOp::kWrite:
            ++mine.writes; mine.wbytes += req.length; break;
          case hipstore::IoOp::kFill: ++mine.unmaps; break;
          case hipstore::IoOp::kFlush: break;
        }
        bdev->submit(nullptr, std::move(req));
      }
    });
  }
  for (auto& t : threads) t.join();
  Sum want;
  for (const Sum& s : sums) {
    want.reads += s.reads; want.writes += s.writes; want.unmaps += s.unmaps;
    want.rbytes += s.rbytes; want.wbytes += s.wbytes;
  }
  const hipstore::Bdev::IoStat got = bdev->iostat();
  CHECK(got.num_read_ops == want.reads);
  CHECK(got.num_write_ops == want.writes);
  CHECK(got.num_unmap_ops == want.unmaps);
  CHECK(got.bytes_read == want.rbytes);
  CHECK(got.bytes_written == want.wbytes);
  CHECK(want.reads > 0 && want.writes > 0 && want.unmaps > 0);
  CHECK(want.reads + want.writes + want.unmaps < uint64_t{kThreads} * kRequests);
}

}  // namespace

int main() {
  test_hit_miss_remove();
  test_reregistration_through_cache();
  test_touching_ranges_and_straddling_tile();
  test_concurrent_lookup();
  test_sharded_iostat();
  if (g_failures != 0) {
    fprintf(stderr, "submit_path_test: %d check(s) failed\n", g_failures);
    return 1;
  }
  printf("submit_path_test: ok\n");
  return 0;
}
