// Stand-alone check of the parity host code (native/src/parity.cpp): the
// GF(2^8) tables against bit-wise field arithmetic, the rebuild
// coefficients, and encode / check / every single and double loss on
// the generic path over malloc bdevs. Host code only: the few engine
// entry points parity.cpp needs are defined here, without a GPU. Built
// and run under AddressSanitizer by `make parity-test`.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hipstore/parity.h"

namespace hipstore {

bool gpu_available() { return false; }
void* alloc_pinned(size_t bytes) { return malloc(bytes); }
void free_pinned(void* ptr) { free(ptr); }

static int run_sync(Bdev* bdev, IoOp op, uint64_t offset, void* buf,
                    uint64_t len) {
  auto channel = bdev->get_channel();
  int status = kIoFailed;
  bool done = false;
  IoRequest req;
  req.op = op;
  req.offset = offset;
  req.length = len;
  req.buffer = buf;
  req.on_complete = [&](int s) { status = s; done = true; };
  bdev->submit(channel.get(), std::move(req));
  while (!done) bdev->poll(channel.get());
  return status;
}
int bdev_read_sync(Bdev* bdev, uint64_t offset, void* buf, uint64_t len) {
  return run_sync(bdev, IoOp::kRead, offset, buf, len);
}
int bdev_write_sync(Bdev* bdev, uint64_t offset, const void* buf,
                    uint64_t len) {
  return run_sync(bdev, IoOp::kWrite, offset, const_cast<void*>(buf), len);
}

// No GPU path in this program.
int parity_kernel_device(const std::vector<Bdev*>&) { return -1; }
int parity_encode_gpu(int, const ParitySet&, uint8_t*, uint8_t*, uint64_t) {
  return kIoFailed;
}
int parity_check_gpu(int, const ParitySet&, const uint8_t*, const uint8_t*,
                     uint64_t, uint32_t, std::vector<uint64_t>*,
                     std::vector<uint64_t>*) {
  return kIoFailed;
}
int parity_rebuild_gpu(int, const ParitySet&, const uint8_t*, const uint8_t*,
                       ParityCoeffs, uint8_t*, uint8_t*, uint64_t) {
  return kIoFailed;
}

}  // namespace hipstore

using namespace hipstore;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

// Shift-and-reduce multiply: no tables.
static uint8_t slow_mul(uint8_t a, uint8_t b) {
  uint32_t r = 0;
  for (uint32_t x = a; b != 0; b >>= 1, x = (x << 1) ^ ((x & 0x80) ? 0x11D : 0)) {
    if (b & 1) r ^= x;
  }
  return static_cast<uint8_t>(r);
}

int main() {
  for (int a = 0; a < 256; ++a) {
    for (int b = 0; b < 256; ++b) {
      CHECK(gf256_mul(a, b) == slow_mul(a, b));
    }
    if (a != 0) CHECK(gf256_mul(a, gf256_inv(a)) == 1);
  }
  CHECK(gf256_pow2(0) == 1 && gf256_pow2(8) == 0x1D && gf256_pow2(255) == 1);
  CHECK(gf256_mul(gf256_pow2(-31), gf256_pow2(31)) == 1);

  // k = 5 over 2 MiB + 1 block (three generic spans), distinct offsets.
  constexpr uint32_t kK = 5;
  constexpr uint64_t kBlock = 512;
  constexpr uint64_t kLength = (2u << 20) + kBlock;
  std::vector<BdevPtr> bdevs;
  std::vector<ParityMember> data;
  std::vector<std::vector<uint8_t>> want(kK + 2, std::vector<uint8_t>(kLength));
  uint32_t seed = 12345;
  for (uint32_t i = 0; i < kK + 2; ++i) {
    bdevs.push_back(create_malloc_bdev("m" + std::to_string(i), kBlock,
                                       kLength / kBlock + i + 1));
    if (i >= kK) continue;
    for (uint8_t& b : want[i]) b = static_cast<uint8_t>((seed = seed * 1664525u + 1013904223u) >> 24);
    CHECK(bdev_write_sync(bdevs[i].get(), i * kBlock, want[i].data(), kLength) == kIoOk);
    data.push_back({bdevs[i].get(), i * kBlock});
  }
  const ParityMember p{bdevs[kK].get(), kK * kBlock};
  const ParityMember q{bdevs[kK + 1].get(), (kK + 1) * kBlock};
  std::vector<ParityMember> all = data;
  all.push_back(p);
  all.push_back(q);
  for (uint64_t b = 0; b < kLength; ++b) {
    for (uint32_t i = 0; i < kK; ++i) {
      want[kK][b] ^= want[i][b];
      want[kK + 1][b] ^= slow_mul(gf256_pow2(i), want[i][b]);
    }
  }
  auto intact = [&] {
    std::vector<uint8_t> got(kLength);
    for (uint32_t i = 0; i < kK + 2; ++i) {
      CHECK(bdev_read_sync(all[i].bdev, all[i].offset, got.data(), kLength) == kIoOk);
      CHECK(got == want[i]);
    }
  };
  ParityReport report;
  CHECK(bdev_parity_encode_sync(data, p, q, kLength, &report) == kIoOk);
  CHECK(!report.on_gpu);
  intact();
  ParityCheck check;
  CHECK(bdev_parity_check_sync(data, p, q, kLength, 512, 4, &check) == kIoOk);
  CHECK(check.p.mismatched == 0 && check.q.mismatched == 0);

  std::vector<uint8_t> junk(kLength, 0xE7);
  for (int x = 0; x < static_cast<int>(kK) + 2; ++x) {
    for (int y = x; y < static_cast<int>(kK) + 2; ++y) {  // y == x: single loss
      std::vector<int> lost;
      for (int m : {x, y}) {
        CHECK(bdev_write_sync(all[m].bdev, all[m].offset, junk.data(), kLength) == kIoOk);
        const int id = m < static_cast<int>(kK) ? m : m == static_cast<int>(kK) ? kParityLostP : kParityLostQ;
        if (lost.empty() || lost[0] != id) lost.push_back(id);
      }
      CHECK(bdev_parity_check_sync(data, p, q, kLength, 512, 0, &check) == kIoOk);
      CHECK(check.p.mismatched + check.q.mismatched > 0);
      CHECK(bdev_parity_rebuild_sync(data, p, q, kLength, lost, &report) == kIoOk);
      intact();
    }
  }
  CHECK(bdev_parity_rebuild_sync(data, p, {}, kLength, {0, 1}, &report) == kIoInvalid);
  CHECK(!report.error.empty());
  printf("parity_test: ok\n");
  return 0;
}
