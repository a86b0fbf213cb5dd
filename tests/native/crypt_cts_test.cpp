// Stand-alone check of the HSXTS2 host codec (native/src/crypt.cpp,
// ciphertext stealing): round trips on heap buffers of exactly the
// unit's length, in place and out of place, and agreement with the unit
// functions at multiples of 16. Host code only. Built and run under
// AddressSanitizer and UBSan by `make crypt-cts-test`.

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hipstore/crypt.h"

using namespace hipstore;

#define CHECK(cond)                                                       \
  if (!(cond)) {                                                          \
    fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
    exit(1);                                                              \
  }

int main() {
  std::vector<uint8_t> key(64);
  for (size_t i = 0; i < key.size(); ++i) key[i] = static_cast<uint8_t>(i);
  const XtsSchedules keys(key.data());
  for (uint32_t n : {16u, 17u, 31u, 32u, 33u, 1023u, 1024u, 1025u, 1039u,
                     1040u}) {
    std::vector<uint8_t> in(n);
    for (uint32_t i = 0; i < n; ++i) in[i] = static_cast<uint8_t>(i * 7 + n);
    std::vector<uint8_t> out(n);
    xts_encrypt_var(keys, 9, in.data(), out.data(), n);
    std::vector<uint8_t> place = in;
    xts_encrypt_var(keys, 9, place.data(), place.data(), n);
    CHECK(place == out && out != in);
    if (n % 16 == 0) {
      std::vector<uint8_t> unit(n);
      xts_encrypt_unit(keys, 9, in.data(), unit.data(), n);
      CHECK(unit == out);
    }
    std::vector<uint8_t> back(n);
    xts_decrypt_var(keys, 9, out.data(), back.data(), n);
    CHECK(back == in);
    xts_decrypt_var(keys, 9, place.data(), place.data(), n);
    CHECK(place == in);
  }
  printf("crypt_cts_test: ok\n");
  return 0;
}
