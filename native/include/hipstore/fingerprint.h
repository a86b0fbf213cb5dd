// Granule fingerprints ("HSFP1", algorithm id 1): 16 bytes per granule,
// a function of the granule's bytes only. The host implementation here
// and hipstore::k_fingerprint_granules (bulk_ops.hip) compute the same
// value.
//
// A granule of G bytes (G % 16 == 0) is n16 = G / 16 vectors; vector i
// is two little-endian u64, q0 at byte 16i and q1 at byte 16i + 8. All
// arithmetic is mod 2^64.
//   P1 = 0x9E3779B185EBCA87  P2 = 0xC2B2AE3D27D4EB4F  P3 = 0x165667B19E3779F9
//   round(acc, q) = rotl64(acc + q * P2, 31) * P1          (the XXH64 round)
//   mix(h): h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32
//   stream s in 0..63 owns vectors s, s + 64, s + 128, ... in that order:
//     A = P1 * (s + 1); B = P2 * (s + 1)
//     for each of its vectors: A = round(A, q0); B = round(B, q1)
//     d0[s] = mix(A ^ mix(B)); d1[s] = mix(B + mix(A))
//   F0 = sum of d0[s], F1 = sum of d1[s] over all 64 streams (also those
//   without a vector); the fingerprint is F0 then F1, 8 LE bytes each.
// A changed granule is missed with probability about 2^-64. The hash is
// not cryptographic: whoever controls the data can construct collisions.

#pragma once

#include <cstdint>

namespace hipstore {

constexpr uint32_t kFingerprintBytes = 16;
constexpr uint32_t kFingerprintAlgorithm = 1;
constexpr uint32_t kFingerprintStreams = 64;

constexpr uint64_t kFingerprintP1 = 0x9E3779B185EBCA87ull;
constexpr uint64_t kFingerprintP2 = 0xC2B2AE3D27D4EB4Full;
constexpr uint64_t kFingerprintP3 = 0x165667B19E3779F9ull;

// Incremental hasher of one granule at a time. update() takes any
// multiple of 16 bytes, so a granule may arrive cut anywhere on a
// 16-byte boundary; finish() writes the fingerprint of what arrived
// since the last finish() and starts the next granule.
class GranuleHasher {
 public:
  GranuleHasher() { reset(); }
  void reset();
  void update(const void* data, uint64_t len);
  void finish(uint8_t out[kFingerprintBytes]);

 private:
  uint64_t a_[kFingerprintStreams];
  uint64_t b_[kFingerprintStreams];
  uint32_t next_;  // stream of the next vector
};

// Fingerprints of `n` consecutive granules of `granule` bytes each
// (granule % 16 == 0) into out[0 .. n * 16).
void fingerprint_granules(const void* data, uint64_t n, uint32_t granule,
                          uint8_t* out);

}  // namespace hipstore
