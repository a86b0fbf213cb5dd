// Stand-alone check of the HSLZ1 host codec (native/src/compress.cpp):
// round trips of every content class through the compressor, the
// validator and the decoder, and malformed streams against the validator
// and the decoder, which must refuse them without touching memory they
// do not own. Host code only. Built and run under AddressSanitizer and
// UBSan by `make compress-test`.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hipstore/compress.h"

using namespace hipstore;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static uint32_t g_seed = 2026;
static uint8_t next_byte() {
  return static_cast<uint8_t>((g_seed = g_seed * 1664525u + 1013904223u) >> 24);
}

// Heap copies of exactly the right size, so that any access outside the
// piece or the granule is an AddressSanitizer report.
static void round_trip(const std::vector<uint8_t>& in, bool expect_raw) {
  const uint32_t g = static_cast<uint32_t>(in.size());
  std::vector<uint8_t> out(g);
  const uint32_t size = lz_compress_granule(in.data(), g, out.data());
  CHECK(size >= 1 && size <= g);
  CHECK((size == g) == expect_raw);
  const std::vector<uint8_t> piece(out.begin(), out.begin() + size);
  std::string why;
  CHECK(lz_validate_granule(piece.data(), piece.size(), g, &why));
  std::vector<uint8_t> back(g, 0xEE);
  CHECK(lz_decompress_granule(piece.data(), piece.size(), g, back.data()));
  CHECK(back == in);
}

static void refused(const std::vector<uint8_t>& piece, uint32_t g) {
  std::string why;
  std::vector<uint8_t> out(g);
  CHECK(!lz_validate_granule(piece.data(), piece.size(), g, &why));
  CHECK(!why.empty());
  CHECK(!lz_decompress_granule(piece.data(), piece.size(), g, out.data()));
}

// 8 literals, a match of `len` at `offset`, then `tail` literals under
// `last_token`: legal for len = g - 13, tail = 5, last_token = 0x50.
static std::vector<uint8_t> block_of(uint32_t offset, uint32_t len,
                                     uint8_t last_token, uint32_t tail) {
  std::vector<uint8_t> b = {0x8F, 'A', 'A', 'A', 'A', 'A', 'A', 'A', 'A',
                            static_cast<uint8_t>(offset),
                            static_cast<uint8_t>(offset >> 8)};
  uint32_t rest = len - 4 - 15;
  for (; rest >= 255; rest -= 255) b.push_back(255);
  b.push_back(static_cast<uint8_t>(rest));
  b.push_back(last_token);
  b.insert(b.end(), tail, 'Z');
  return b;
}

int main() {
  for (uint32_t g : {512u, 528u, 4096u, 16384u}) {
    std::vector<uint8_t> v(g, 0);
    round_trip(v, false);  // zeros: chains of 255
    for (uint8_t& b : v) b = next_byte();
    round_trip(v, true);  // random: raw
    for (uint32_t period : {1u, 3u, 7u, 64u, 65u}) {
      for (uint32_t i = 0; i < g; ++i) v[i] = static_cast<uint8_t>('a' + i % period);
      round_trip(v, false);
    }
    for (uint8_t& b : v) b = next_byte();
    memcpy(&v[g / 2], &v[0], g / 2);  // a repeat that runs to the last byte
    round_trip(v, false);
    const char* words[] = {"granule ", "window ", "bitmap ", "rank ", "of the "};
    for (uint32_t i = 0; i < g;) {  // text-like
      for (const char* w = words[next_byte() % 5]; *w != 0 && i < g; ++w) v[i++] = *w;
    }
    round_trip(v, false);

    const std::vector<uint8_t> good = block_of(8, g - 13, 0x50, 5);
    std::string why;
    CHECK(lz_validate_granule(good.data(), good.size(), g, &why));
    refused(block_of(0, g - 13, 0x50, 5), g);   // offset 0
    refused(block_of(9, g - 13, 0x50, 5), g);   // offset past the start
    refused(block_of(8, g - 12, 0x50, 5), g);   // match overruns G
    refused(block_of(8, g - 10, 0x20, 2), g);   // match into the last 5
    refused(block_of(8, g - 13, 0x60, 5), g);   // literals overrun the piece
    refused(block_of(8, g - 14, 0x50, 5), g);   // output shorter than G
    refused(block_of(8, g - 13, 0xF0, 5), g);   // literal length never ends
    for (size_t cut = 0; cut < good.size(); ++cut) {  // every truncation
      refused(std::vector<uint8_t>(good.begin(), good.begin() + cut), g);
    }
    refused(std::vector<uint8_t>(g + 1, 0), g);  // longer than G
    // every single-byte change of a legal block decodes or is refused
    for (size_t at = 0; at < good.size(); ++at) {
      std::vector<uint8_t> bent = good;
      bent[at] ^= 0xFF;
      std::vector<uint8_t> out(g);
      CHECK(lz_validate_granule(bent.data(), bent.size(), g) ==
            lz_decompress_granule(bent.data(), bent.size(), g, out.data()));
    }
  }
  std::vector<uint8_t> odd(520, 0);
  std::string why;
  CHECK(!lz_validate_granule(odd.data(), 100, 520, &why));  // G % 16 != 0
  printf("compress_test: ok\n");
  return 0;
}
