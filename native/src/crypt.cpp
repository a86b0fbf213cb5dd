// The HSXTS1 and HSXTS2 host codec (hipstore/crypt.h): AES-256 byte by
// byte and XTS over one data unit, with ciphertext stealing for HSXTS2. It is the byte model of the kernels in
// crypt_ops.hip and shares nothing with them: the S-box is derived from
// the field inverse here and written out there, rounds are S-box,
// ShiftRows and xtime here and T-tables there, decryption is the
// straight inverse cipher here and the equivalent one there. Plain host
// code; the marked calls and the kernels are in crypt_ops.hip.

#include "hipstore/crypt.h"

#include <string.h>

namespace hipstore {

namespace {

uint8_t xtime(uint8_t a) {
  return static_cast<uint8_t>(a << 1 ^ (a >> 7) * 0x1B);
}

uint8_t gf_mul(uint8_t a, uint8_t b) {
  uint8_t r = 0;
  for (; b != 0; b >>= 1, a = xtime(a)) {
    if (b & 1) r ^= a;
  }
  return r;
}

struct Sboxes {
  uint8_t fwd[256];
  uint8_t inv[256];
  // S(x) = affine(x^-1): x^254 by multiplication, then the bit matrix.
  Sboxes() {
    for (int x = 0; x < 256; ++x) {
      uint8_t y = 1;
      for (int i = 0; i < 254; ++i) y = gf_mul(y, static_cast<uint8_t>(x));
      if (x == 0) y = 0;
      uint8_t s = 0x63;
      for (int r = 0; r < 5; ++r) {
        s ^= static_cast<uint8_t>(y << r | y >> (8 - r));
      }
      fwd[x] = s;
      inv[s] = static_cast<uint8_t>(x);
    }
  }
};

const Sboxes& sboxes() {
  static const Sboxes boxes;
  return boxes;
}

void add_round_key(uint8_t s[16], const uint8_t* rk) {
  for (int i = 0; i < 16; ++i) s[i] ^= rk[i];
}

// State byte 4 * c + r is row r of column c. Row r moves left by r
// columns (right for the inverse).
void shift_rows(uint8_t s[16], bool inverse) {
  uint8_t t[16];
  for (int c = 0; c < 4; ++c) {
    for (int r = 0; r < 4; ++r) {
      const int from = inverse ? (c + 4 - r) % 4 : (c + r) % 4;
      t[4 * c + r] = s[4 * from + r];
    }
  }
  memcpy(s, t, 16);
}

// Column times the circulant of (m0, m1, m2, m3): (2, 3, 1, 1) forward,
// (14, 11, 13, 9) inverse.
void mix_columns(uint8_t s[16], const uint8_t m[4]) {
  for (int c = 0; c < 4; ++c) {
    uint8_t col[4];
    memcpy(col, s + 4 * c, 4);
    for (int r = 0; r < 4; ++r) {
      uint8_t v = 0;
      for (int k = 0; k < 4; ++k) v ^= gf_mul(col[(r + k) % 4], m[k]);
      s[4 * c + r] = v;
    }
  }
}

const uint8_t kMix[4] = {2, 3, 1, 1};
const uint8_t kInvMix[4] = {14, 11, 13, 9};

// The tweak block times alpha: a little-endian 128-bit shift with the
// carry folded back as 0x87.
void tweak_double(uint8_t t[16]) {
  uint8_t carry = 0;
  for (int i = 0; i < 16; ++i) {
    const uint8_t next = t[i] >> 7;
    t[i] = static_cast<uint8_t>(t[i] << 1 | carry);
    carry = next;
  }
  if (carry) t[0] ^= 0x87;
}

void first_tweak(const XtsSchedules& keys, uint64_t unit, uint8_t t[16]) {
  memset(t, 0, 16);
  for (int i = 0; i < 8; ++i) t[i] = static_cast<uint8_t>(unit >> (8 * i));
  aes256_encrypt_block(keys.k2_enc, t, t);
}

template <typename Block>
void xts_unit(const XtsSchedules& keys, uint64_t unit, const uint8_t* in,
              uint8_t* out, uint32_t bytes, Block block) {
  uint8_t t[16];
  uint8_t x[16];
  first_tweak(keys, unit, t);
  for (uint32_t at = 0; at + 16 <= bytes; at += 16, tweak_double(t)) {
    for (int i = 0; i < 16; ++i) x[i] = in[at + i] ^ t[i];
    block(keys.k1_enc, x, x);
    for (int i = 0; i < 16; ++i) out[at + i] = x[i] ^ t[i];
  }
  explicit_bzero(t, sizeof(t));
  explicit_bzero(x, sizeof(x));
}

}  // namespace

bool xts_key_ok(const uint8_t* key, size_t len) {
  return key != nullptr && len == kXtsKeyBytes &&
         memcmp(key, key + 32, 32) != 0;
}

void aes256_expand(const uint8_t key[32], uint8_t rk[kAesScheduleBytes]) {
  const uint8_t* sbox = sboxes().fwd;
  memcpy(rk, key, 32);
  uint8_t rcon = 1;
  for (int w = 8; w < 60; ++w) {
    uint8_t t[4];
    memcpy(t, rk + 4 * (w - 1), 4);
    if (w % 8 == 0) {
      const uint8_t first = t[0];
      t[0] = sbox[t[1]] ^ rcon;
      t[1] = sbox[t[2]];
      t[2] = sbox[t[3]];
      t[3] = sbox[first];
      rcon = xtime(rcon);
    } else if (w % 8 == 4) {
      for (uint8_t& b : t) b = sbox[b];
    }
    for (int i = 0; i < 4; ++i) rk[4 * w + i] = rk[4 * (w - 8) + i] ^ t[i];
  }
}

void aes256_encrypt_block(const uint8_t rk[kAesScheduleBytes],
                          const uint8_t in[16], uint8_t out[16]) {
  const uint8_t* sbox = sboxes().fwd;
  uint8_t s[16];
  memcpy(s, in, 16);
  add_round_key(s, rk);
  for (int round = 1; round <= 14; ++round) {
    for (uint8_t& b : s) b = sbox[b];
    shift_rows(s, false);
    if (round != 14) mix_columns(s, kMix);
    add_round_key(s, rk + 16 * round);
  }
  memcpy(out, s, 16);
  explicit_bzero(s, sizeof(s));
}

void aes256_decrypt_block(const uint8_t rk[kAesScheduleBytes],
                          const uint8_t in[16], uint8_t out[16]) {
  const uint8_t* inv = sboxes().inv;
  uint8_t s[16];
  memcpy(s, in, 16);
  add_round_key(s, rk + 16 * 14);
  for (int round = 13; round >= 0; --round) {
    shift_rows(s, true);
    for (uint8_t& b : s) b = inv[b];
    add_round_key(s, rk + 16 * round);
    if (round != 0) mix_columns(s, kInvMix);
  }
  memcpy(out, s, 16);
  explicit_bzero(s, sizeof(s));
}

XtsSchedules::XtsSchedules(const uint8_t key[kXtsKeyBytes]) {
  aes256_expand(key, k1_enc);
  aes256_expand(key + 32, k2_enc);
  for (int round = 0; round <= 14; ++round) {
    memcpy(k1_dec + 16 * round, k1_enc + 16 * (14 - round), 16);
    if (round != 0 && round != 14) mix_columns(k1_dec + 16 * round, kInvMix);
  }
}

XtsSchedules::~XtsSchedules() { explicit_bzero(this, sizeof(*this)); }

void xts_encrypt_unit(const XtsSchedules& keys, uint64_t unit,
                      const uint8_t* in, uint8_t* out, uint32_t bytes) {
  xts_unit(keys, unit, in, out, bytes, aes256_encrypt_block);
}

void xts_decrypt_unit(const XtsSchedules& keys, uint64_t unit,
                      const uint8_t* in, uint8_t* out, uint32_t bytes) {
  xts_unit(keys, unit, in, out, bytes, aes256_decrypt_block);
}

namespace {

// HSXTS2 over n = 16 * m + b bytes, m >= 1. The whole blocks but the last
// go through xts_unit; `t` is then doubled up to T_{m-1}, `t_next` is
// T_m. Encryption uses T_{m-1} first and T_m second, decryption the
// other way round.
template <typename Block>
void xts_var(const XtsSchedules& keys, uint64_t unit, const uint8_t* in,
             uint8_t* out, uint32_t bytes, bool encrypt, Block block) {
  const uint32_t b = bytes % 16;
  if (b == 0) {
    xts_unit(keys, unit, in, out, bytes, block);
    return;
  }
  const uint32_t last = bytes - b - 16;  // where block m-1 starts
  xts_unit(keys, unit, in, out, last, block);
  uint8_t t[16];
  uint8_t t_next[16];
  uint8_t x[16];
  uint8_t tail[16];
  first_tweak(keys, unit, t);
  for (uint32_t at = 0; at < last; at += 16) tweak_double(t);
  memcpy(t_next, t, 16);
  tweak_double(t_next);
  const uint8_t* first = encrypt ? t : t_next;
  const uint8_t* second = encrypt ? t_next : t;
  memcpy(tail, in + last + 16, b);  // before out overwrites it (in == out)
  for (int i = 0; i < 16; ++i) x[i] = in[last + i] ^ first[i];
  block(keys.k1_enc, x, x);
  for (int i = 0; i < 16; ++i) x[i] ^= first[i];
  // x is CC (or PP): its head is the stored tail, its rest is stolen.
  memcpy(out + last + 16, x, b);
  memcpy(x, tail, b);
  for (int i = 0; i < 16; ++i) x[i] ^= second[i];
  block(keys.k1_enc, x, x);
  for (int i = 0; i < 16; ++i) out[last + i] = x[i] ^ second[i];
  explicit_bzero(t, sizeof(t));
  explicit_bzero(t_next, sizeof(t_next));
  explicit_bzero(x, sizeof(x));
  explicit_bzero(tail, sizeof(tail));
}

}  // namespace

void xts_encrypt_var(const XtsSchedules& keys, uint64_t unit,
                     const uint8_t* in, uint8_t* out, uint32_t bytes) {
  xts_var(keys, unit, in, out, bytes, true, aes256_encrypt_block);
}

void xts_decrypt_var(const XtsSchedules& keys, uint64_t unit,
                     const uint8_t* in, uint8_t* out, uint32_t bytes) {
  xts_var(keys, unit, in, out, bytes, false, aes256_decrypt_block);
}

uint32_t xts_kcv(const uint8_t key[kXtsKeyBytes]) {
  const XtsSchedules keys(key);
  uint8_t block[16] = {0};
  xts_encrypt_unit(keys, kXtsKcvUnit, block, block, 16);
  return static_cast<uint32_t>(block[0]) | static_cast<uint32_t>(block[1]) << 8 |
         static_cast<uint32_t>(block[2]) << 16 |
         static_cast<uint32_t>(block[3]) << 24;
}

}  // namespace hipstore
