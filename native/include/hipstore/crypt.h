// Encryption of checkpoint granules: "HSXTS1", AES-256-XTS as in
// IEEE 1619 / NIST SP 800-38E, fixed as follows.
//
//   key        64 bytes, K1 || K2: K1 encrypts data, K2 the tweak.
//              K1 == K2 and any other length are refused.
//   data unit  one granule of G bytes, G % 16 == 0, G <= 2^24 (the
//              standard's 2^20 blocks per unit). No ciphertext stealing.
//   unit no.   first_unit + g for granule g of the call's range;
//              first_unit is 0 for every file operation, so a granule's
//              number in a file is its index in the volume.
//   tweak      the number as a little-endian u64 in bytes 0-7 of a block,
//              bytes 8-15 zero; T_0 = AES_K2(that block) and
//              T_j = T_0 * alpha^j in GF(2^128) mod x^128+x^7+x^2+x+1 for
//              16-byte block j of the unit (a block is a little-endian
//              128-bit number).
//   block j    C_j = AES_K1(P_j ^ T_j) ^ T_j.
//   kcv(key)   the first four bytes, as a little-endian u32, of the
//              encryption of a 16-byte all-zero unit with number 2^64-1,
//              which no granule can carry: a wrong key is refused before
//              anything is written, at the price of one ciphertext of one
//              known plaintext.
// With G = 512 this is the aes-xts-plain64 layout.
//
// "HSXTS2" is HSXTS1 with the data unit generalised to any n bytes, 16 <=
// n <= 2^24: IEEE 1619 ciphertext stealing. It encrypts the compressed
// pieces of version-5 delta files (delta.h). Key, unit number, tweak, kcv
// and alpha are unchanged. With n = 16 * m + b, 0 <= b < 16:
//   b == 0     exactly HSXTS1.
//   otherwise  blocks 0 .. m-2 as in HSXTS1; CC = E(P_{m-1}, T_{m-1}); the
//              stored tail C_m is the first b bytes of CC; PP = P_m (b
//              bytes) || CC[b..16); the stored C_{m-1} = E(PP, T_m).
//              Decryption: C_{m-1} under T_m gives PP, then C_m ||
//              PP[b..16) under T_{m-1} gives P_{m-1}.
// The stored length equals the plaintext length. A piece shorter than 16
// bytes (a dictionary piece of a small granule) is zero-padded to one
// block and stored as 16 bytes; its recorded size stays the true one and
// the reader ignores the pad.
//
// The host codec below is the byte model of k_xts_pack_marked,
// k_xts_unpack_marked and k_xts_var (crypt_ops.hip) and a different algorithm on
// purpose: byte-wise S-box, ShiftRows and xtime MixColumns, the straight
// inverse cipher, the tweak doubled block by block. The kernels use
// T-tables, the equivalent inverse cipher and log-step tweaks.

#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "hipstore/engine.h"

namespace hipstore {

constexpr size_t kXtsKeyBytes = 64;
constexpr uint32_t kXtsMaxGranule = 1u << 24;
constexpr size_t kAesScheduleBytes = 240;  // 15 round keys
constexpr uint64_t kXtsKcvUnit = ~0ull;

inline bool xts_granule_ok(uint64_t granule) {
  return granule != 0 && granule % 16 == 0 && granule <= kXtsMaxGranule;
}

// 64 bytes whose halves differ.
bool xts_key_ok(const uint8_t* key, size_t len);

// FIPS-197 key expansion: round key r is rk[16 * r, 16 * r + 16).
void aes256_expand(const uint8_t key[32], uint8_t rk[kAesScheduleBytes]);
void aes256_encrypt_block(const uint8_t rk[kAesScheduleBytes],
                          const uint8_t in[16], uint8_t out[16]);
// The straight inverse cipher, on the encryption schedule.
void aes256_decrypt_block(const uint8_t rk[kAesScheduleBytes],
                          const uint8_t in[16], uint8_t out[16]);

// The three schedules of a key, cleared when the object goes. k1_dec is
// the schedule of the equivalent inverse cipher (round keys reversed,
// InvMixColumns applied to the inner thirteen): what k_xts_unpack_marked
// reads, not what xts_decrypt_unit uses.
struct XtsSchedules {
  uint8_t k1_enc[kAesScheduleBytes];
  uint8_t k1_dec[kAesScheduleBytes];
  uint8_t k2_enc[kAesScheduleBytes];

  explicit XtsSchedules(const uint8_t key[kXtsKeyBytes]);
  ~XtsSchedules();
  XtsSchedules(const XtsSchedules&) = delete;
  XtsSchedules& operator=(const XtsSchedules&) = delete;
};

// One data unit of `bytes` bytes (a multiple of 16); in == out is fine.
void xts_encrypt_unit(const XtsSchedules& keys, uint64_t unit,
                      const uint8_t* in, uint8_t* out, uint32_t bytes);
void xts_decrypt_unit(const XtsSchedules& keys, uint64_t unit,
                      const uint8_t* in, uint8_t* out, uint32_t bytes);

// HSXTS2: one data unit of any `bytes` >= 16; in == out is fine. A
// multiple of 16 gives what the unit functions give.
void xts_encrypt_var(const XtsSchedules& keys, uint64_t unit,
                     const uint8_t* in, uint8_t* out, uint32_t bytes);
void xts_decrypt_var(const XtsSchedules& keys, uint64_t unit,
                     const uint8_t* in, uint8_t* out, uint32_t bytes);

// xts_key_ok(key) required.
uint32_t xts_kcv(const uint8_t key[kXtsKeyBytes]);

// The key argument of the marked calls here and in compress.h: `len`
// bytes at `key` (not owned), and the unit number of granule 0 of the
// call's range.
struct XtsKey {
  const uint8_t* key = nullptr;
  size_t len = 0;
  uint64_t first_unit = 0;
};

// bdev_pack_marked_sync with every granule encrypted: validation, plan,
// windows, staging and the chunks handed to the sink are the same; also
// kIoInvalid unless xts_key_ok, xts_granule_ok and first_unit + the
// range's granules stays below 2^64-1. An HBM bdev with a usable GPU runs
// k_xts_pack_marked per window, which gathers and encrypts in one pass:
// plaintext never crosses PCIe and never sits in pinned host memory.
// Every other bdev goes through bdev_pack_marked_sync and
// xts_encrypt_unit on each chunk. Both paths hand the sink the same
// chunks and the same bytes.
int bdev_xts_pack_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                              uint32_t granule,
                              const std::vector<uint64_t>& bitmap,
                              const XtsKey& key, uint64_t staging_bytes,
                              const PackSink& sink, uint64_t* packed = nullptr);

// The inverse: source fills the next chunk with ciphertext, which is
// decrypted into the marked granules (k_xts_unpack_marked, or
// xts_decrypt_unit and bdev_unpack_marked_sync). Unmarked granules are
// never written.
int bdev_xts_unpack_marked_sync(Bdev* dst, uint64_t dst_offset,
                                uint64_t length, uint32_t granule,
                                const std::vector<uint64_t>& bitmap,
                                const XtsKey& key, uint64_t staging_bytes,
                                const UnpackSource& source,
                                uint64_t* unpacked = nullptr);

}  // namespace hipstore
