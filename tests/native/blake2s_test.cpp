// Stand-alone check of the HSFP2 host code (native/src/fingerprint.cpp):
// the RFC 7693 "abc" vector, and the per-granule hasher cut at every
// 16-byte boundary against the one-shot call, on heap buffers of exactly
// the right size. Under AddressSanitizer and UBSan by `make blake2s-test`.

#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hipstore/fingerprint.h"

using namespace hipstore;

int main() {
  // RFC 7693, appendix B.
  {
    const std::vector<uint8_t> abc = {'a', 'b', 'c'};
    const std::vector<uint8_t> want = {
        0x50, 0x8c, 0x5e, 0x8c, 0x32, 0x7c, 0x14, 0xe2, 0xe1, 0xa7, 0x2b,
        0xa3, 0x4e, 0xeb, 0x45, 0x2f, 0x37, 0x45, 0x8b, 0x20, 0x9e, 0xd6,
        0x3a, 0x29, 0x4d, 0x99, 0x9b, 0x4c, 0x86, 0x67, 0x59, 0x82};
    std::vector<uint8_t> digest(32);
    Blake2s hash(32, nullptr, 0);
    hash.update(abc.data(), abc.size());
    hash.finish(digest.data());
    assert(digest == want);
  }
  // 208 bytes: three full blocks and a quarter. Every cut gives the
  // one-shot fingerprint.
  std::vector<uint8_t> key(kBlake2sKeyBytes);
  for (size_t i = 0; i < key.size(); ++i) key[i] = static_cast<uint8_t>(0xA0 + i);
  const FingerprintKind kinds[2] = {
      {kFingerprintBlake2s, nullptr, 0},
      {kFingerprintBlake2sKeyed, key.data(), key.size()}};
  const uint32_t granule = 208;
  std::vector<uint8_t> data(2 * granule);
  for (size_t i = 0; i < data.size(); ++i) {
    data[i] = static_cast<uint8_t>(i * 37 + 11);
  }
  std::vector<uint8_t> whole[2];
  for (int k = 0; k < 2; ++k) {
    whole[k].resize(2 * kFingerprintBytes);
    const bool ok = fingerprint_granules(data.data(), 2, granule, kinds[k],
                                         whole[k].data());
    assert(ok);
    Blake2sMidstate start;
    blake2s_granule_midstate(kinds[k], &start);
    assert(start.t0 == (k == 0 ? 0u : 64u));
    Blake2sGranuleHasher hasher(start);
    for (uint32_t cut = 0; cut <= granule; cut += 16) {
      for (uint32_t g = 0; g < 2; ++g) {
        // pieces copied out, so that a read past one is seen
        const uint8_t* p = data.data() + g * granule;
        const std::vector<uint8_t> a(p, p + cut);
        const std::vector<uint8_t> b(p + cut, p + granule);
        hasher.update(a.data(), a.size());
        hasher.update(b.data(), b.size());
        std::vector<uint8_t> fp(kFingerprintBytes);
        hasher.finish(fp.data());
        assert(memcmp(fp.data(), whole[k].data() + g * kFingerprintBytes,
                     kFingerprintBytes) == 0);
      }
    }
  }
  assert(whole[0] != whole[1]);
  printf("blake2s_test: ok\n");
  return 0;
}
