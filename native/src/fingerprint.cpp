// Host implementation of granule fingerprints (fingerprint.h).

#include "hipstore/fingerprint.h"

#include <string.h>

namespace hipstore {

namespace {

inline uint64_t rotl64(uint64_t v, int r) { return (v << r) | (v >> (64 - r)); }

inline uint64_t fp_round(uint64_t acc, uint64_t q) {
  return rotl64(acc + q * kFingerprintP2, 31) * kFingerprintP1;
}

inline uint64_t fp_mix(uint64_t h) {
  h ^= h >> 33;
  h *= kFingerprintP2;
  h ^= h >> 29;
  h *= kFingerprintP3;
  h ^= h >> 32;
  return h;
}

inline uint64_t load_le64(const uint8_t* p) {
#if __BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__
  uint64_t v;
  memcpy(&v, p, 8);
  return v;
#else
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  return v;
#endif
}

inline void store_le64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}

}  // namespace

void GranuleHasher::reset() {
  for (uint32_t s = 0; s < kFingerprintStreams; ++s) {
    a_[s] = kFingerprintP1 * (s + 1);
    b_[s] = kFingerprintP2 * (s + 1);
  }
  next_ = 0;
}

void GranuleHasher::update(const void* data, uint64_t len) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  uint64_t left = len / 16;
  // Up to the next row boundary, whole rows, then the rest.
  for (; left > 0 && next_ != 0; --left, p += 16) {
    a_[next_] = fp_round(a_[next_], load_le64(p));
    b_[next_] = fp_round(b_[next_], load_le64(p + 8));
    next_ = (next_ + 1) % kFingerprintStreams;
  }
  for (; left >= kFingerprintStreams;
       left -= kFingerprintStreams, p += 16 * kFingerprintStreams) {
    for (uint32_t s = 0; s < kFingerprintStreams; ++s) {
      a_[s] = fp_round(a_[s], load_le64(p + 16 * s));
      b_[s] = fp_round(b_[s], load_le64(p + 16 * s + 8));
    }
  }
  for (; left > 0; --left, p += 16) {
    a_[next_] = fp_round(a_[next_], load_le64(p));
    b_[next_] = fp_round(b_[next_], load_le64(p + 8));
    next_ = (next_ + 1) % kFingerprintStreams;
  }
}

void GranuleHasher::finish(uint8_t out[kFingerprintBytes]) {
  uint64_t f0 = 0;
  uint64_t f1 = 0;
  for (uint32_t s = 0; s < kFingerprintStreams; ++s) {
    f0 += fp_mix(a_[s] ^ fp_mix(b_[s]));
    f1 += fp_mix(b_[s] + fp_mix(a_[s]));
  }
  store_le64(out, f0);
  store_le64(out + 8, f1);
  reset();
}

void fingerprint_granules(const void* data, uint64_t n, uint32_t granule,
                          uint8_t* out) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  GranuleHasher hasher;
  for (uint64_t g = 0; g < n; ++g) {
    hasher.update(p + g * granule, granule);
    hasher.finish(out + g * kFingerprintBytes);
  }
}

}  // namespace hipstore
