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

// --- HSFP2: BLAKE2s, written after RFC 7693 section 3 ----------------------
// v[16], the sigma table and G as the RFC prints them; the kernel keeps
// the state by columns in a quad of lanes instead.

namespace {

const uint32_t kBlake2sIv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u,
                                0xA54FF53Au, 0x510E527Fu, 0x9B05688Cu,
                                0x1F83D9ABu, 0x5BE0CD19u};

const uint8_t kBlake2sSigma[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
    {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
    {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
    {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
    {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
    {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

const uint8_t kHsfp2Person[8] = {'H', 'S', 'F', 'P', '2', 0, 0, 0};
const uint8_t kHsfp2KcvPerson[8] = {'H', 'S', 'F', 'P', '2', 'k', 'c', 'v'};

inline uint32_t rotr32(uint32_t v, int r) { return (v >> r) | (v << (32 - r)); }

inline uint32_t load_le32(const uint8_t* p) {
  return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 |
         static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}

inline void blake2s_g(uint32_t v[16], int a, int b, int c, int d, uint32_t x,
                      uint32_t y) {
  v[a] = v[a] + v[b] + x;
  v[d] = rotr32(v[d] ^ v[a], 16);
  v[c] = v[c] + v[d];
  v[b] = rotr32(v[b] ^ v[c], 12);
  v[a] = v[a] + v[b] + y;
  v[d] = rotr32(v[d] ^ v[a], 8);
  v[c] = v[c] + v[d];
  v[b] = rotr32(v[b] ^ v[c], 7);
}

// F(h, block, t, final) of the RFC.
void blake2s_compress(uint32_t h[8], const uint8_t block[kBlake2sBlockBytes],
                      uint64_t t, bool last) {
  uint32_t m[16];
  uint32_t v[16];
  for (int i = 0; i < 16; ++i) m[i] = load_le32(block + 4 * i);
  for (int i = 0; i < 8; ++i) {
    v[i] = h[i];
    v[i + 8] = kBlake2sIv[i];
  }
  v[12] ^= static_cast<uint32_t>(t);
  v[13] ^= static_cast<uint32_t>(t >> 32);
  if (last) v[14] = ~v[14];
  for (int r = 0; r < 10; ++r) {
    const uint8_t* s = kBlake2sSigma[r];
    blake2s_g(v, 0, 4, 8, 12, m[s[0]], m[s[1]]);
    blake2s_g(v, 1, 5, 9, 13, m[s[2]], m[s[3]]);
    blake2s_g(v, 2, 6, 10, 14, m[s[4]], m[s[5]]);
    blake2s_g(v, 3, 7, 11, 15, m[s[6]], m[s[7]]);
    blake2s_g(v, 0, 5, 10, 15, m[s[8]], m[s[9]]);
    blake2s_g(v, 1, 6, 11, 12, m[s[10]], m[s[11]]);
    blake2s_g(v, 2, 7, 8, 13, m[s[12]], m[s[13]]);
    blake2s_g(v, 3, 4, 9, 14, m[s[14]], m[s[15]]);
  }
  for (int i = 0; i < 8; ++i) h[i] ^= v[i] ^ v[i + 8];
  explicit_bzero(m, sizeof(m));
  explicit_bzero(v, sizeof(v));
}

}  // namespace

bool fingerprint_kind_ok(const FingerprintKind& kind) {
  if (kind.algorithm == kFingerprintAlgorithm ||
      kind.algorithm == kFingerprintBlake2s) {
    return kind.key == nullptr && kind.key_bytes == 0;
  }
  return kind.algorithm == kFingerprintBlake2sKeyed && kind.key != nullptr &&
         kind.key_bytes == kBlake2sKeyBytes;
}

Blake2s::Blake2s(uint32_t out_bytes, const uint8_t* key, size_t key_bytes,
                 const uint8_t* person8)
    : out_bytes_(out_bytes) {
  // The parameter block: digest length, key length, fanout 1, depth 1,
  // then zeros up to the personalisation in its last 8 bytes.
  for (int i = 0; i < 8; ++i) h_[i] = kBlake2sIv[i];
  h_[0] ^= 0x01010000u ^ static_cast<uint32_t>(key_bytes) << 8 ^ out_bytes;
  if (person8 != nullptr) {
    h_[6] ^= load_le32(person8);
    h_[7] ^= load_le32(person8 + 4);
  }
  memset(buf_, 0, sizeof(buf_));
  if (key_bytes > 0) {
    memcpy(buf_, key, key_bytes);
    fill_ = kBlake2sBlockBytes;
  }
}

Blake2s::Blake2s(uint32_t out_bytes, const Blake2sMidstate& start)
    : t_(start.t0), out_bytes_(out_bytes) {
  memcpy(h_, start.h, sizeof(h_));
  memset(buf_, 0, sizeof(buf_));
}

Blake2s::~Blake2s() {
  explicit_bzero(h_, sizeof(h_));
  explicit_bzero(buf_, sizeof(buf_));
}

void Blake2s::update(const void* data, uint64_t len) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  while (len > 0) {
    if (fill_ == kBlake2sBlockBytes) {  // more follows: not the last block
      t_ += kBlake2sBlockBytes;
      blake2s_compress(h_, buf_, t_, false);
      fill_ = 0;
    }
    const uint64_t n = len < kBlake2sBlockBytes - fill_
                           ? len
                           : kBlake2sBlockBytes - fill_;
    memcpy(buf_ + fill_, p, n);
    fill_ += static_cast<uint32_t>(n);
    p += n;
    len -= n;
  }
}

void Blake2s::finish(uint8_t* out) {
  t_ += fill_;
  memset(buf_ + fill_, 0, kBlake2sBlockBytes - fill_);
  blake2s_compress(h_, buf_, t_, true);
  for (uint32_t i = 0; i < out_bytes_; ++i) {
    out[i] = static_cast<uint8_t>(h_[i / 4] >> (8 * (i % 4)));
  }
}

void blake2s_granule_midstate(const FingerprintKind& kind,
                              Blake2sMidstate* out) {
  for (int i = 0; i < 8; ++i) out->h[i] = kBlake2sIv[i];
  out->h[0] ^= 0x01010000u ^ static_cast<uint32_t>(kind.key_bytes) << 8 ^
               kFingerprintBytes;
  out->h[6] ^= load_le32(kHsfp2Person);
  out->h[7] ^= load_le32(kHsfp2Person + 4);
  out->t0 = 0;
  if (kind.key_bytes > 0) {
    uint8_t block[kBlake2sBlockBytes] = {0};
    memcpy(block, kind.key, kind.key_bytes);
    out->t0 = kBlake2sBlockBytes;
    blake2s_compress(out->h, block, out->t0, false);
    explicit_bzero(block, sizeof(block));
  }
}

uint32_t blake2s_kcv(const uint8_t key[kBlake2sKeyBytes]) {
  uint8_t digest[kFingerprintBytes];
  Blake2s hash(kFingerprintBytes, key, kBlake2sKeyBytes, kHsfp2KcvPerson);
  hash.finish(digest);
  return load_le32(digest);
}

Blake2sGranuleHasher::Blake2sGranuleHasher(const Blake2sMidstate& start)
    : start_(start), cur_(kFingerprintBytes, start) {}

Blake2sGranuleHasher::~Blake2sGranuleHasher() {
  explicit_bzero(&start_, sizeof(start_));
}

void Blake2sGranuleHasher::finish(uint8_t out[kFingerprintBytes]) {
  cur_.finish(out);
  cur_ = Blake2s(kFingerprintBytes, start_);
}

bool fingerprint_granules(const void* data, uint64_t n, uint32_t granule,
                          const FingerprintKind& kind, uint8_t* out) {
  if (!fingerprint_kind_ok(kind)) return false;
  if (kind.algorithm == kFingerprintAlgorithm) {
    fingerprint_granules(data, n, granule, out);
    return true;
  }
  const uint8_t* p = static_cast<const uint8_t*>(data);
  Blake2sMidstate start;
  blake2s_granule_midstate(kind, &start);
  Blake2sGranuleHasher hasher(start);
  for (uint64_t g = 0; g < n; ++g) {
    hasher.update(p + g * granule, granule);
    hasher.finish(out + g * kFingerprintBytes);
  }
  explicit_bzero(&start, sizeof(start));
  return true;
}

}  // namespace hipstore
