// Stand-alone check of the HSLZD1 host codec (native/src/compress.cpp):
// edits of a dictionary through the compressor, the validator and the
// decoder, then every truncation and single-byte change of a piece, which
// must be refused or decoded inside the buffers. Host code only; built
// and run under AddressSanitizer and UBSan by `make compress-test`.

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
static uint32_t g_seed = 2027;
static uint8_t next_byte() {
  return static_cast<uint8_t>((g_seed = g_seed * 1664525u + 1013904223u) >> 24);
}

// Heap copies of exactly the right size, for AddressSanitizer's sake.
static std::vector<uint8_t> round_trip(const std::vector<uint8_t>& x,
                                       const std::vector<uint8_t>& d,
                                       uint32_t at_most) {
  const uint32_t g = static_cast<uint32_t>(x.size());
  std::vector<uint8_t> out(g);
  const uint32_t size = lz_dict_compress_granule(x.data(), d.data(), g, out.data());
  CHECK(size >= 1 && size <= at_most);
  const std::vector<uint8_t> piece(out.begin(), out.begin() + size);
  CHECK(lz_dict_validate_granule(piece.data(), piece.size(), g));
  std::vector<uint8_t> back(g, 0xEE);
  CHECK(lz_dict_decompress_granule(piece.data(), piece.size(), g, d.data(),
                                   back.data()));
  CHECK(back == x);
  return piece;
}

int main() {
  for (uint32_t g : {512u, 528u, 4096u, 16384u}) {
    std::vector<uint8_t> d(g);
    for (uint8_t& b : d) b = next_byte();
    // two sequences (token, <= 4 literals, offset, length), 5 literals
    const uint32_t edit_bound = 2 * (1 + 4 + 2 + 1 + (g - 19) / 255) + 6;
    std::vector<uint8_t> x = d;
    round_trip(x, d, edit_bound);  // equal: one match from the first byte
    x[g / 2] ^= 0x40;
    const std::vector<uint8_t> good = round_trip(x, d, edit_bound);
    x[g / 2] ^= 0x40, x[1] ^= 0x40;  // no aligned match at the first position
    round_trip(x, d, edit_bound);
    memmove(&x[3], &d[0], g - 3);  // shifted: table candidates only
    round_trip(x, d, g);
    memset(x.data(), 0, g);  // matches inside the granule, offset 1
    round_trip(x, d, g / 4);
    for (uint8_t& b : x) b = next_byte();  // unrelated: raw
    CHECK(round_trip(x, d, g).size() == g);
    std::vector<uint8_t> out(g);
    for (size_t cut = 0; cut < good.size(); ++cut) {  // every truncation
      const std::vector<uint8_t> part(good.begin(), good.begin() + cut);
      CHECK(!lz_dict_validate_granule(part.data(), part.size(), g));
      CHECK(!lz_dict_decompress_granule(part.data(), part.size(), g, d.data(),
                                        out.data()));
    }
    // every single-byte change of a legal piece decodes or is refused
    for (size_t at = 0; at < 3 * good.size(); ++at) {
      std::vector<uint8_t> bent = good;
      bent[at / 3] ^= static_cast<uint8_t>(0xFF8001u >> (at % 3 * 8));
      CHECK(lz_dict_validate_granule(bent.data(), bent.size(), g) ==
            lz_dict_decompress_granule(bent.data(), bent.size(), g, d.data(),
                                       out.data()));
    }
  }
  printf("dict_compress_test: ok\n");
  return 0;
}
