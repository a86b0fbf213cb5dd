// Stand-alone check of the HSXTS1 host codec (native/src/crypt.cpp):
// FIPS-197 and XTS known answers, round trips on heap buffers of exactly
// the right size, the equivalent-inverse schedule the unpack kernel
// reads, and the key check value. Host code only. Built and run under
// AddressSanitizer and UBSan by `make crypt-test`.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hipstore/crypt.h"

using namespace hipstore;

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

static std::vector<uint8_t> from_hex(const char* hex) {
  std::vector<uint8_t> out;
  for (; hex[0] != '\0' && hex[1] != '\0'; hex += 2) {
    unsigned v = 0;
    CHECK(sscanf(hex, "%2x", &v) == 1);
    out.push_back(static_cast<uint8_t>(v));
  }
  return out;
}

static std::vector<uint8_t> counting(size_t n) {
  std::vector<uint8_t> out(n);
  for (size_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(i);
  return out;
}

// GF(2^8) helpers for the schedule check, written out again here.
static uint8_t mul(uint8_t a, uint8_t b) {
  uint8_t r = 0;
  for (; b != 0; b >>= 1) {
    if (b & 1) r ^= a;
    a = static_cast<uint8_t>(a << 1 ^ (a >> 7) * 0x1B);
  }
  return r;
}

int main() {
  // FIPS-197 C.3.
  const std::vector<uint8_t> key = counting(64);
  std::vector<uint8_t> rk(kAesScheduleBytes);
  aes256_expand(key.data(), rk.data());
  const std::vector<uint8_t> plain = from_hex("00112233445566778899aabbccddeeff");
  std::vector<uint8_t> block(16);
  aes256_encrypt_block(rk.data(), plain.data(), block.data());
  CHECK(block == from_hex("8ea2b7ca516745bfeafc49904b496089"));
  aes256_decrypt_block(rk.data(), block.data(), block.data());
  CHECK(block == plain);

  // XTS, unit 5, 48 bytes (OpenSSL 3.0.2 EVP_aes_256_xts).
  CHECK(xts_key_ok(key.data(), key.size()));
  const XtsSchedules keys(key.data());
  const std::vector<uint8_t> text = counting(48);
  std::vector<uint8_t> cipher(48);
  xts_encrypt_unit(keys, 5, text.data(), cipher.data(), 48);
  CHECK(cipher ==
        from_hex("f87ca2f29b117c1b024a6ec8e8c5994e76f7d16b43eed21e6936126969e0"
                 "0dab9d57dfb999d8d20535e3b2b7a51fab52"));
  std::vector<uint8_t> back(48);
  xts_decrypt_unit(keys, 5, cipher.data(), back.data(), 48);
  CHECK(back == text);

  // Round trips in place; neighbouring units and keys differ.
  for (uint32_t bytes : {16u, 512u, 1536u, 4096u}) {
    const std::vector<uint8_t> in = counting(bytes);
    std::vector<uint8_t> a = in;
    std::vector<uint8_t> b = in;
    xts_encrypt_unit(keys, 0xFFFFFFFFull, a.data(), a.data(), bytes);
    xts_encrypt_unit(keys, 0x100000000ull, b.data(), b.data(), bytes);
    CHECK(a != in && a != b);
    xts_decrypt_unit(keys, 0xFFFFFFFFull, a.data(), a.data(), bytes);
    CHECK(a == in);
  }

  // k1_dec: round keys reversed, InvMixColumns on the inner thirteen.
  for (int round = 0; round <= 14; ++round) {
    const uint8_t* from = keys.k1_enc + 16 * (14 - round);
    const uint8_t* got = keys.k1_dec + 16 * round;
    for (int c = 0; c < 4; ++c) {
      for (int r = 0; r < 4; ++r) {
        const uint8_t* col = from + 4 * c;
        const uint8_t want =
            round == 0 || round == 14
                ? col[r]
                : mul(col[r], 14) ^ mul(col[(r + 1) % 4], 11) ^
                      mul(col[(r + 2) % 4], 13) ^ mul(col[(r + 3) % 4], 9);
        CHECK(got[4 * c + r] == want);
      }
    }
  }

  // Keys and their check value.
  std::vector<uint8_t> equal(64, 7);
  CHECK(!xts_key_ok(equal.data(), equal.size()));
  CHECK(!xts_key_ok(key.data(), 63) && !xts_key_ok(nullptr, 64));
  std::vector<uint8_t> zero(16, 0);
  xts_encrypt_unit(keys, kXtsKcvUnit, zero.data(), zero.data(), 16);
  uint32_t first = 0;
  for (int i = 3; i >= 0; --i) first = first << 8 | zero[i];
  CHECK(xts_kcv(key.data()) == first);
  std::vector<uint8_t> other = key;
  other[63] ^= 1;
  CHECK(xts_kcv(other.data()) != first);
  CHECK(xts_granule_ok(16) && xts_granule_ok(1u << 24));
  CHECK(!xts_granule_ok(0) && !xts_granule_ok(24) &&
        !xts_granule_ok((1u << 24) + 16));

  printf("crypt_test: ok\n");
  return 0;
}
