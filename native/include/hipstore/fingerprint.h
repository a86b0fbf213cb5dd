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
// HSFP2 below is the choice where that matters.
//
// "HSFP2" (algorithm ids 2 and 3): BLAKE2s (RFC 7693, sequential mode)
// with a 16-byte digest per granule,
//   fp(granule) = blake2s(granule, digest_size = 16, key = K,
//                         person = "HSFP2\0\0\0")
// fanout 1, depth 1, no salt. K is empty for algorithm 2 (a
// collision-resistant drop-in for HSFP1: 64-bit collision resistance) and
// kBlake2sKeyBytes = 32 bytes for algorithm 3 (BLAKE2s' own keyed mode, a
// MAC: a map cannot be forged without K). G % 16 == 0 as above; the
// fingerprint depends on the granule's bytes and on K only. The key check
// value of a keyed map is the first four bytes, little-endian, of
//   blake2s("", digest_size = 16, key = K, person = "HSFP2kcv").
// The chaining value after the parameter block (and, keyed, after the key
// block) is the same for every granule: blake2s_granule_midstate computes
// it once per call, and it is all hipstore::k_blake2s_granules
// (blake2s_ops.hip) and Blake2sGranuleHasher start from. It is
// key-equivalent: clear copies of it like a key.

#pragma once

#include <cstddef>
#include <cstdint>

namespace hipstore {

constexpr uint32_t kFingerprintBytes = 16;
constexpr uint32_t kFingerprintAlgorithm = 1;
constexpr uint32_t kFingerprintBlake2s = 2;
constexpr uint32_t kFingerprintBlake2sKeyed = 3;
constexpr uint32_t kBlake2sKeyBytes = 32;
constexpr uint32_t kBlake2sBlockBytes = 64;
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

// Which fingerprint a call computes: the algorithm id and, for id 3 only,
// the key. The default is HSFP1.
struct FingerprintKind {
  uint32_t algorithm = kFingerprintAlgorithm;
  const uint8_t* key = nullptr;
  size_t key_bytes = 0;
};

// Algorithm 1 or 2 without a key, or 3 with a key of 32 bytes.
bool fingerprint_kind_ok(const FingerprintKind& kind);

// Where every HSFP2 granule starts: h after the parameter block and, when
// keyed, the key block; t0 is 0 or 64.
struct Blake2sMidstate {
  uint32_t h[8];
  uint32_t t0;
};

// Plain scalar BLAKE2s straight from RFC 7693: out_bytes 1..32, key of
// 0..32 bytes, an optional 8-byte personalisation. update() takes any
// length; the last block is held back until finish(), which may be called
// once.
class Blake2s {
 public:
  Blake2s(uint32_t out_bytes, const uint8_t* key, size_t key_bytes,
          const uint8_t* person8 = nullptr);
  // Continues from a chaining value reached after start.t0 bytes.
  Blake2s(uint32_t out_bytes, const Blake2sMidstate& start);
  ~Blake2s();
  void update(const void* data, uint64_t len);
  void finish(uint8_t* out);

 private:
  uint32_t h_[8];
  uint64_t t_ = 0;
  uint8_t buf_[kBlake2sBlockBytes];
  uint32_t fill_ = 0;
  uint32_t out_bytes_;
};

// `kind` must be fingerprint_kind_ok with algorithm 2 or 3.
void blake2s_granule_midstate(const FingerprintKind& kind,
                              Blake2sMidstate* out);

// The key check value of a keyed map.
uint32_t blake2s_kcv(const uint8_t key[kBlake2sKeyBytes]);

// GranuleHasher's contract for HSFP2.
class Blake2sGranuleHasher {
 public:
  explicit Blake2sGranuleHasher(const Blake2sMidstate& start);
  ~Blake2sGranuleHasher();
  void update(const void* data, uint64_t len) { cur_.update(data, len); }
  void finish(uint8_t out[kFingerprintBytes]);

 private:
  Blake2sMidstate start_;
  Blake2s cur_;
};

// fingerprint_granules for any algorithm; false when `kind` is not
// fingerprint_kind_ok.
bool fingerprint_granules(const void* data, uint64_t n, uint32_t granule,
                          const FingerprintKind& kind, uint8_t* out);

}  // namespace hipstore
