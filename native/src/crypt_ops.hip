// MI355X (gfx950) HSXTS1 encryption of marked granules (definition and
// host codec in hipstore/crypt.h, crypt.cpp): k_xts_pack_marked gathers
// and encrypts in one pass, k_xts_unpack_marked decrypts and scatters;
// their window loops and the generic path. Like bulk_ops.hip, each call
// owns its stream, runs to completion and returns. k_xts_var (HSXTS2,
// ciphertext stealing) encrypts and decrypts the variable-length pieces
// of compress_ops.hip, which launches it through crypt_internal.h.
//
// Work split: as compress_ops.hip. A wave takes one whole granule at a
// time and waves grid-stride over the granules of the window's bitmap
// words (wave_window_walk, at most 2048 workgroups of 256 threads), so
// the bit test, the unit number and the first tweak are wave-uniform and
// waves never wait for each other after the tables are up. Lane l owns
// the 16-byte blocks l, l + 64, ... of the granule: one wave instruction
// moves 1 KiB contiguously, and a block goes HBM -> registers -> pinned
// slot (or back) without touching LDS.
//
// Tweaks: T_0 = AES_K2(unit number) is computed by every lane from the
// same inputs, which costs a wave what one lane would cost it and makes
// every table read a broadcast. Lane l then takes T_0 * alpha^l in six
// conditional steps, one per bit of l (a step * alpha^k, k <= 32, is a
// 128-bit shift plus a carry-less multiply of the k overflow bits by
// 0x87, done as four shifted XORs), and every further row is one step
// * alpha^64. No lane doubles in a loop.
//
// Rounds: 32-bit T-table rounds. One table per direction (Te0, Td0) with
// the other three columns taken by rotating the word (v_alignbit, one
// VALU instruction, where a second table would cost 1 KiB per copy), and
// each table stored kTableCopies = 8 times, entry-interleaved
// (t[x * 8 + (lane & 7)]): lanes that differ in their low three bits can
// never meet in a bank, which cuts the expected conflict degree of 64
// random indices into 256 words from about 4 to below 2 for 8 KiB per
// table. The last round reads byte S-boxes (256 bytes, 64 words: lanes
// that share a word are served together). Tables are derived from the
// S-box by the workgroup's 256 threads, one entry each, before the walk:
// 8.5 KiB of LDS for pack, 16.7 KiB for unpack.
//
// Round keys: the schedule of K1 for this direction and the encryption
// schedule of K2, 2 x 60 dwords, travel in the kernel-argument struct.
// Both do not fit the scalar register file (the compiler spilled 98
// SGPRs into VGPR lanes when asked to hold them). K1's is used by every
// block: its rounds are unrolled with constant indices, so it is read
// with scalar loads from the argument segment and stays in SGPRs. K2's is
// used once per granule: table setup copies it into LDS and the tweak's
// rounds read it from there, every lane the same word (a broadcast).
// There is no per-lane key read from global memory and no key in device
// memory of ours.
//
// No branch and no address depends on data or key except the table
// index itself; plain loads and stores, no global atomics, nothing read
// from the dense buffer by pack.

#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "crypt_internal.h"
#include "gpu_internal.h"
#include "hipstore/crypt.h"
#include "hipstore/engine.h"
#include "marked_internal.h"

namespace hipstore {

namespace {

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

constexpr uint32_t kTableCopies = 8;
constexpr uint32_t kXtsThreads = 256;  // one table entry per thread

__constant__ uint8_t kAesSbox[256] = {
    0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b,
    0xfe, 0xd7, 0xab, 0x76, 0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0,
    0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0, 0xb7, 0xfd, 0x93, 0x26,
    0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
    0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2,
    0xeb, 0x27, 0xb2, 0x75, 0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0,
    0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84, 0x53, 0xd1, 0x00, 0xed,
    0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
    0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f,
    0x50, 0x3c, 0x9f, 0xa8, 0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5,
    0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2, 0xcd, 0x0c, 0x13, 0xec,
    0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
    0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14,
    0xde, 0x5e, 0x0b, 0xdb, 0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c,
    0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79, 0xe7, 0xc8, 0x37, 0x6d,
    0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
    0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f,
    0x4b, 0xbd, 0x8b, 0x8a, 0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e,
    0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e, 0xe1, 0xf8, 0x98, 0x11,
    0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
    0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f,
    0xb0, 0x54, 0xbb, 0x16,
};

__device__ __forceinline__ uint32_t gf_double(uint32_t b) {
  return (b << 1 ^ (b >> 7) * 0x1Bu) & 0xFFu;
}

// What a kernel's rounds read, all in LDS. `copy` is lane & 7.
struct XtsTables {
  const uint32_t* te;    // Te0, kTableCopies times
  const uint32_t* td;    // Td0 likewise (unpack only)
  const uint8_t* sbox;
  const uint8_t* isbox;  // unpack only
  const uint32_t* tweak_rk;  // K2's schedule
  uint32_t copy;
};

__device__ __forceinline__ uint32_t look(const uint32_t* table, uint32_t byte,
                                         uint32_t copy) {
  return table[byte * kTableCopies + copy];
}

// Column `a`'s row 0, b's row 1, c's row 2 and d's row 3 through one
// T-table: the other three tables are byte rotations of the first.
__device__ __forceinline__ uint32_t t_column(const uint32_t* table,
                                             uint32_t copy, uint32_t a,
                                             uint32_t b, uint32_t c,
                                             uint32_t d) {
  return look(table, a & 0xFF, copy) ^
         __builtin_rotateleft32(look(table, (b >> 8) & 0xFF, copy), 8) ^
         __builtin_rotateleft32(look(table, (c >> 16) & 0xFF, copy), 16) ^
         __builtin_rotateleft32(look(table, d >> 24, copy), 24);
}

__device__ __forceinline__ uint32_t s_column(const uint8_t* box, uint32_t a,
                                             uint32_t b, uint32_t c,
                                             uint32_t d) {
  return static_cast<uint32_t>(box[a & 0xFF]) |
         static_cast<uint32_t>(box[(b >> 8) & 0xFF]) << 8 |
         static_cast<uint32_t>(box[(c >> 16) & 0xFF]) << 16 |
         static_cast<uint32_t>(box[d >> 24]) << 24;
}

// The state is four little-endian column words, as loaded. ShiftRows
// makes column j take row r from column j + r.
template <typename Schedule>
__device__ __forceinline__ uint4 aes_encrypt(const XtsTables& t,
                                             const Schedule& rk, uint4 s) {
  s.x ^= rk[0];
  s.y ^= rk[1];
  s.z ^= rk[2];
  s.w ^= rk[3];
#pragma unroll
  for (int r = 1; r < 14; ++r) {
    uint4 n;
    n.x = t_column(t.te, t.copy, s.x, s.y, s.z, s.w) ^ rk[4 * r];
    n.y = t_column(t.te, t.copy, s.y, s.z, s.w, s.x) ^ rk[4 * r + 1];
    n.z = t_column(t.te, t.copy, s.z, s.w, s.x, s.y) ^ rk[4 * r + 2];
    n.w = t_column(t.te, t.copy, s.w, s.x, s.y, s.z) ^ rk[4 * r + 3];
    s = n;
  }
  uint4 o;
  o.x = s_column(t.sbox, s.x, s.y, s.z, s.w) ^ rk[56];
  o.y = s_column(t.sbox, s.y, s.z, s.w, s.x) ^ rk[57];
  o.z = s_column(t.sbox, s.z, s.w, s.x, s.y) ^ rk[58];
  o.w = s_column(t.sbox, s.w, s.x, s.y, s.z) ^ rk[59];
  return o;
}

// The equivalent inverse cipher on XtsSchedules::k1_dec. InvShiftRows
// makes column j take row r from column j - r.
__device__ __forceinline__ uint4 aes_decrypt(const XtsTables& t,
                                             const uint32_t (&dk)[60],
                                             uint4 s) {
  s.x ^= dk[0];
  s.y ^= dk[1];
  s.z ^= dk[2];
  s.w ^= dk[3];
#pragma unroll
  for (int r = 1; r < 14; ++r) {
    uint4 n;
    n.x = t_column(t.td, t.copy, s.x, s.w, s.z, s.y) ^ dk[4 * r];
    n.y = t_column(t.td, t.copy, s.y, s.x, s.w, s.z) ^ dk[4 * r + 1];
    n.z = t_column(t.td, t.copy, s.z, s.y, s.x, s.w) ^ dk[4 * r + 2];
    n.w = t_column(t.td, t.copy, s.w, s.z, s.y, s.x) ^ dk[4 * r + 3];
    s = n;
  }
  uint4 o;
  o.x = s_column(t.isbox, s.x, s.w, s.z, s.y) ^ dk[56];
  o.y = s_column(t.isbox, s.y, s.x, s.w, s.z) ^ dk[57];
  o.z = s_column(t.isbox, s.z, s.y, s.x, s.w) ^ dk[58];
  o.w = s_column(t.isbox, s.w, s.z, s.y, s.x) ^ dk[59];
  return o;
}

// A tweak block as a little-endian 128-bit number.
struct Tweak {
  uint64_t lo;
  uint64_t hi;
};

// v * 0x87 without carries, low 64 bits.
__device__ __forceinline__ uint64_t clmul_87(uint64_t v) {
  return v ^ v << 1 ^ v << 2 ^ v << 7;
}

// t * alpha^k for 1 <= k <= 32: the k bits that leave the top come back
// times 0x87, which then fits 40 bits.
template <int k>
__device__ __forceinline__ Tweak tweak_shift(Tweak t) {
  static_assert(k >= 1 && k <= 32, "the folded product must fit 64 bits");
  const uint64_t over = t.hi >> (64 - k);
  return {t.lo << k ^ clmul_87(over), t.hi << k | t.lo >> (64 - k)};
}

template <int k>
__device__ __forceinline__ Tweak tweak_shift_if(Tweak t, uint32_t lane) {
  const Tweak moved = tweak_shift<k>(t);
  const bool take = (lane & k) != 0;
  return {take ? moved.lo : t.lo, take ? moved.hi : t.hi};
}

// t * alpha^64: hi * x^128 = hi * 0x87 = V < 2^71, so
// (hi, lo) -> (lo ^ V >> 64, V mod 2^64).
__device__ __forceinline__ Tweak tweak_next_row(Tweak t) {
  return {clmul_87(t.hi), t.lo ^ t.hi >> 63 ^ t.hi >> 62 ^ t.hi >> 57};
}

// The 256 threads of the workgroup build the tables, one entry each.
// Te0[x] = (2, 1, 1, 3) * S[x] and Td0[x] = (14, 9, 13, 11) * S^-1[x],
// rows 0 to 3 in bytes 0 to 3.
template <bool kEncrypt>
__device__ __forceinline__ void xts_build_tables(uint32_t* te, uint32_t* td,
                                                 uint8_t* sbox,
                                                 uint8_t* isbox,
                                                 uint32_t* tweak_rk,
                                                 const XtsKernelKeys& keys) {
  const uint32_t x = threadIdx.x;
  if (x < 60) tweak_rk[x] = keys.tweak[x];
  const uint32_t s = kAesSbox[x];
  const uint32_t s2 = gf_double(s);
  const uint32_t e = s2 | s << 8 | s << 16 | (s2 ^ s) << 24;
#pragma unroll
  for (uint32_t c = 0; c < kTableCopies; ++c) te[x * kTableCopies + c] = e;
  sbox[x] = static_cast<uint8_t>(s);
  if (!kEncrypt) {
    isbox[s] = static_cast<uint8_t>(x);  // S is a permutation
    __syncthreads();
    const uint32_t i = isbox[x];
    const uint32_t i2 = gf_double(i);
    const uint32_t i4 = gf_double(i2);
    const uint32_t i8 = gf_double(i4);
    const uint32_t d = (i8 ^ i4 ^ i2) | (i8 ^ i) << 8 | (i8 ^ i4 ^ i) << 16 |
                       (i8 ^ i2 ^ i) << 24;
#pragma unroll
    for (uint32_t c = 0; c < kTableCopies; ++c) td[x * kTableCopies + c] = d;
  }
  __syncthreads();
}

// Granule g of the range at `bdev_base` and window slot `slot` of
// `dense`, for every marked granule of the window: encrypt from the
// granule to the slot, or decrypt from the slot to the granule.
template <bool kEncrypt>
__device__ __forceinline__ void xts_window(
    uint8_t* __restrict__ bdev_base, uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, const MarkedWindow win,
    uint32_t granule, uint64_t first_unit, const XtsKernelKeys& keys,
    const XtsTables& tables) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule >> 4;
  wave_window_walk(bitmap, rank_before_word, win, [&](uint64_t g,
                                                      uint32_t slot) {
    const uint64_t unit = first_unit + g;  // wave-uniform
    // K2's round keys are read from LDS here, once per granule, and are
    // not kept in 60 VGPRs across the block loop.
    asm volatile("" ::: "memory");
    const uint4 t0 = aes_encrypt(
        tables, tables.tweak_rk,
        make_uint4(static_cast<uint32_t>(unit),
                   static_cast<uint32_t>(unit >> 32), 0, 0));
    Tweak t = {static_cast<uint64_t>(t0.y) << 32 | t0.x,
               static_cast<uint64_t>(t0.w) << 32 | t0.z};
    t = tweak_shift_if<1>(t, lane);
    t = tweak_shift_if<2>(t, lane);
    t = tweak_shift_if<4>(t, lane);
    t = tweak_shift_if<8>(t, lane);
    t = tweak_shift_if<16>(t, lane);
    t = tweak_shift_if<32>(t, lane);
    uint4* __restrict__ pg =
        reinterpret_cast<uint4*>(bdev_base + g * granule);
    uint4* __restrict__ ps = reinterpret_cast<uint4*>(
        dense + static_cast<uint64_t>(slot) * granule);
    const uint4* __restrict__ from = kEncrypt ? pg : ps;
    uint4* __restrict__ to = kEncrypt ? ps : pg;
    for (uint32_t row = 0; row < n16; row += 64, t = tweak_next_row(t)) {
      const uint32_t i = row + lane;
      if (i >= n16) continue;  // past the granule in its last row
      const uint4 mask = make_uint4(static_cast<uint32_t>(t.lo),
                                    static_cast<uint32_t>(t.lo >> 32),
                                    static_cast<uint32_t>(t.hi),
                                    static_cast<uint32_t>(t.hi >> 32));
      uint4 x = from[i];
      x.x ^= mask.x;
      x.y ^= mask.y;
      x.z ^= mask.z;
      x.w ^= mask.w;
      x = kEncrypt ? aes_encrypt(tables, keys.data, x)
                   : aes_decrypt(tables, keys.data, x);
      x.x ^= mask.x;
      x.y ^= mask.y;
      x.z ^= mask.z;
      x.w ^= mask.w;
      to[i] = x;
    }
  });
}

// Marked granule of window rank r -> ciphertext in slot r of `dense`
// (pinned host memory): k_pack_marked's slots, nothing read from `dense`.
__global__ __launch_bounds__(kXtsThreads) void k_xts_pack_marked(
    const uint8_t* __restrict__ src, uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule, uint64_t first_unit, XtsKernelKeys keys) {
  __shared__ uint32_t te[256 * kTableCopies];
  __shared__ uint8_t sbox[256];
  __shared__ uint32_t tweak_rk[60];
  xts_build_tables<true>(te, nullptr, sbox, nullptr, tweak_rk, keys);
  const XtsTables tables = {te, nullptr, sbox, nullptr, tweak_rk,
                            threadIdx.x & (kTableCopies - 1)};
  xts_window<true>(const_cast<uint8_t*>(src), dense, bitmap, rank_before_word,
                   win, granule, first_unit, keys, tables);
}

// The way back; unmarked granules are never written.
__global__ __launch_bounds__(kXtsThreads) void k_xts_unpack_marked(
    uint8_t* __restrict__ dst, const uint8_t* __restrict__ dense,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule, uint64_t first_unit, XtsKernelKeys keys) {
  __shared__ uint32_t te[256 * kTableCopies];
  __shared__ uint32_t td[256 * kTableCopies];
  __shared__ uint8_t sbox[256];
  __shared__ uint8_t isbox[256];
  __shared__ uint32_t tweak_rk[60];
  xts_build_tables<false>(te, td, sbox, isbox, tweak_rk, keys);
  const XtsTables tables = {te, td, sbox, isbox, tweak_rk,
                            threadIdx.x & (kTableCopies - 1)};
  xts_window<false>(dst, const_cast<uint8_t*>(dense), bitmap, rank_before_word,
                    win, granule, first_unit, keys, tables);
}

// --- HSXTS2: units of any length, for compressed pieces ---------------------

// 0xFF in the first n bytes of a block (n <= 16), 0 in the rest.
__device__ __forceinline__ uint4 head_mask(uint32_t n) {
  const uint64_t lo = n >= 8 ? ~0ull : (1ull << (8 * n)) - 1;
  const uint64_t hi = n >= 16 ? ~0ull : n <= 8 ? 0 : (1ull << (8 * (n - 8))) - 1;
  return make_uint4(static_cast<uint32_t>(lo), static_cast<uint32_t>(lo >> 32),
                    static_cast<uint32_t>(hi), static_cast<uint32_t>(hi >> 32));
}

// The first n bytes of `head`, then `rest` from byte n on.
__device__ __forceinline__ uint4 splice(uint4 head, uint4 rest, uint32_t n) {
  const uint4 m = head_mask(n);
  return make_uint4((head.x & m.x) | (rest.x & ~m.x),
                    (head.y & m.y) | (rest.y & ~m.y),
                    (head.z & m.z) | (rest.z & ~m.z),
                    (head.w & m.w) | (rest.w & ~m.w));
}

// One XTS block under tweak t.
template <bool kEncrypt>
__device__ __forceinline__ uint4 xts_block(const XtsTables& tables,
                                           const XtsKernelKeys& keys, uint4 x,
                                           Tweak t) {
  const uint4 mask = make_uint4(static_cast<uint32_t>(t.lo),
                                static_cast<uint32_t>(t.lo >> 32),
                                static_cast<uint32_t>(t.hi),
                                static_cast<uint32_t>(t.hi >> 32));
  x.x ^= mask.x;
  x.y ^= mask.y;
  x.z ^= mask.z;
  x.w ^= mask.w;
  x = kEncrypt ? aes_encrypt(tables, keys.data, x)
               : aes_decrypt(tables, keys.data, x);
  x.x ^= mask.x;
  x.y ^= mask.y;
  x.z ^= mask.z;
  x.w ^= mask.w;
  return x;
}

// The pieces of a window, each one HSXTS2 unit (crypt.h): wave per piece
// over the window's bitmap, because the unit number is the granule's
// index, not its rank. Encrypt reads piece r from slot r of `from`
// (stride G, device scratch of the compress kernels) and writes
// ciphertext to to + offsets[r] (pinned): it takes k_gather_var's place
// and plaintext pieces never leave device memory. Decrypt reads
// ciphertext at from + offsets[r] (pinned) and writes plaintext to to +
// offsets[r] (device scratch), where the LZ decode kernels find their
// pieces as if they were the dense buffer.
//
// Lane l owns blocks l, l + 64, ... and their tweaks as in xts_window.
// With n = 16 * m + b, b != 0, the pair (m-1, m) belongs to the lane that
// owns block m-1: it loads the partial block m as well, T_m is one more
// step * alpha from its own tweak, and it runs the second cipher call
// after its first, so CC never leaves its registers. Nothing crosses
// lanes or the row step, so m % 64 == 0 (block m in the next row, which
// is then never entered) is no special case, and decryption is the same
// code with the two tweaks swapped; giving block m to the next lane
// instead would make decryption send C_{m-1} up a lane and CC back down,
// across rows when m % 64 == 0. The price is that the pair's lane runs
// two cipher calls in sequence while its row's other lanes wait: one
// block time per piece.
//
// Every global access is 16 bytes per lane. Tails are cut and spliced in
// registers; the stored tail block is written with its pad as zero, and a
// piece of fewer than 16 bytes is one zero-padded block. The size is cut
// to G, so with G % 16 == 0 block m of a piece with b != 0 ends inside
// the slot; nothing depends on data or key except the table index.
template <bool kEncrypt>
__global__ __launch_bounds__(kXtsThreads) void k_xts_var(
    const uint8_t* __restrict__ from, uint8_t* __restrict__ to,
    const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule, uint64_t first_unit, XtsKernelKeys keys) {
  __shared__ uint32_t te[256 * kTableCopies];
  __shared__ uint32_t td[kEncrypt ? 1 : 256 * kTableCopies];
  __shared__ uint8_t sbox[256];
  __shared__ uint8_t isbox[kEncrypt ? 1 : 256];
  __shared__ uint32_t tweak_rk[60];
  xts_build_tables<kEncrypt>(te, td, sbox, isbox, tweak_rk, keys);
  const XtsTables tables = {te, td, sbox, isbox, tweak_rk,
                            threadIdx.x & (kTableCopies - 1)};
  const uint32_t lane = threadIdx.x & 63;
  wave_window_walk(bitmap, rank_before_word, win, [&](uint64_t g,
                                                      uint32_t slot) {
    const uint32_t size = min(uniform(sizes[slot]), granule);
    if (size == 0) return;  // no such piece: nothing to move
    const uint32_t n = max(size, 16u);
    const uint32_t m = n >> 4;  // whole blocks, >= 1
    const uint32_t b = n & 15;  // bytes of block m
    const uint64_t unit = first_unit + g;  // wave-uniform
    asm volatile("" ::: "memory");  // K2's schedule stays in LDS
    const uint4 t0 = aes_encrypt(
        tables, tables.tweak_rk,
        make_uint4(static_cast<uint32_t>(unit),
                   static_cast<uint32_t>(unit >> 32), 0, 0));
    Tweak t = {static_cast<uint64_t>(t0.y) << 32 | t0.x,
               static_cast<uint64_t>(t0.w) << 32 | t0.z};
    t = tweak_shift_if<1>(t, lane);
    t = tweak_shift_if<2>(t, lane);
    t = tweak_shift_if<4>(t, lane);
    t = tweak_shift_if<8>(t, lane);
    t = tweak_shift_if<16>(t, lane);
    t = tweak_shift_if<32>(t, lane);
    const uint64_t at = offsets[slot];
    const uint4* __restrict__ pin = reinterpret_cast<const uint4*>(
        kEncrypt ? from + static_cast<uint64_t>(slot) * granule : from + at);
    uint4* __restrict__ pout = reinterpret_cast<uint4*>(to + at);
    for (uint32_t row = 0; row < m; row += 64, t = tweak_next_row(t)) {
      const uint32_t i = row + lane;
      if (i >= m) continue;  // past the whole blocks in the last row
      uint4 x = pin[i];
      if (kEncrypt) x = splice(x, make_uint4(0, 0, 0, 0), min(size, 16u));
      const bool steal = b != 0 && i == m - 1;
      const Tweak t_next = tweak_shift<1>(t);
      // Encryption runs block m-1 under T_{m-1}, then the spliced block
      // under T_m; decryption the other way round.
      x = xts_block<kEncrypt>(tables, keys, x,
                              steal && !kEncrypt ? t_next : t);
      if (steal) {
        const uint4 tail = pin[m];
        pout[m] = splice(x, make_uint4(0, 0, 0, 0), b);
        x = xts_block<kEncrypt>(tables, keys, splice(tail, x, b),
                                kEncrypt ? t_next : t);
      }
      if (!kEncrypt) x = splice(x, make_uint4(0, 0, 0, 0), min(size, 16u));
      pout[i] = x;
    }
  });
}

// ---------------------------------------------------------------------------
// Window loops
// ---------------------------------------------------------------------------

// The dense stream of this family: ciphertext only, two halves.
PinnedBuf<uint8_t>& xts_staging() {
  thread_local PinnedBuf<uint8_t> staging;
  return staging;
}

void load_words(const uint8_t* schedule, uint32_t* words) {
  for (int i = 0; i < 60; ++i) {
    words[i] = static_cast<uint32_t>(schedule[4 * i]) |
               static_cast<uint32_t>(schedule[4 * i + 1]) << 8 |
               static_cast<uint32_t>(schedule[4 * i + 2]) << 16 |
               static_cast<uint32_t>(schedule[4 * i + 3]) << 24;
  }
}

// What both GPU window loops run on: the window stream with the keys.
// The copy of the schedules here is cleared with the object; what a
// launch copied into the runtime's argument memory is not ours.
struct XtsStream : WindowStream {
  uint64_t first_unit;
  XtsKernelKeys keys;

  XtsStream(int device, Bdev* bdev, uint64_t offset, uint32_t granule_bytes,
            const MarkedPlan& plan, const XtsSchedules& schedules,
            bool encrypt, uint64_t first)
      : WindowStream(device, bdev, offset, granule_bytes, plan, xts_staging()),
        first_unit(first) {
    xts_load_kernel_keys(schedules, encrypt, &keys);
  }
  ~XtsStream() { explicit_bzero(&keys, sizeof(keys)); }

  template <typename Kernel>
  void launch(Kernel kernel, const MarkedWindow& win, int half) {
    WindowStream::launch(kernel, wave_window_grid(win, kXtsThreads / 64),
                         kXtsThreads, win, half, first_unit, keys);
  }
};

// k_xts_pack_marked per window on the shared pack loop.
int xts_gpu(XtsStream& xs, const MarkedPlan& plan, const PackSink& sink,
            uint64_t* packed) {
  return pack_windows(
      xs, plan,
      [&](const MarkedWindow& win, int half) {
        xs.launch(k_xts_pack_marked, win, half);
      },
      [](const MarkedWindow&, int) {},
      [&](const MarkedWindow& win, int half) {
        return sink(xs.half_of(half), win.first_rank, win.count);
      },
      packed);
}

// k_xts_unpack_marked per window on the shared unpack loop.
int xts_gpu(XtsStream& xs, const MarkedPlan& plan, const UnpackSource& source,
            uint64_t* unpacked) {
  return unpack_windows(
      xs, plan, [](int) { return 0; },
      [&](const MarkedWindow& win, int half) {
        return source(xs.half_of(half), win.first_rank, win.count);
      },
      [&](const MarkedWindow& win, int half) {
        xs.launch(k_xts_unpack_marked, win, half);
      },
      unpacked);
}

// Generic paths: bdev_pack_marked_sync / bdev_unpack_marked_sync cut the
// chunks, the host codec does the rest. Chunks arrive in rank order, so
// one MarkCursor over the bitmap gives every granule its unit number.
int xts_generic(Bdev* src, uint64_t offset, uint64_t length, uint32_t granule,
                const std::vector<uint64_t>& bitmap, const XtsSchedules& keys,
                uint64_t first_unit, uint64_t staging_bytes,
                const PackSink& sink, uint64_t* packed) {
  std::vector<uint8_t> out;
  MarkCursor marks{bitmap, length / granule};
  return bdev_pack_marked_sync(
      src, offset, length, granule, bitmap, staging_bytes,
      [&](const uint8_t* data, uint64_t first_rank, uint64_t count) {
        out.resize(count * granule);
        for (uint64_t i = 0; i < count; ++i) {
          xts_encrypt_unit(keys, first_unit + marks.next(), data + i * granule,
                           out.data() + i * granule, granule);
        }
        return sink(out.data(), first_rank, count);
      },
      packed);
}

int xts_generic(Bdev* dst, uint64_t offset, uint64_t length, uint32_t granule,
                const std::vector<uint64_t>& bitmap, const XtsSchedules& keys,
                uint64_t first_unit, uint64_t staging_bytes,
                const UnpackSource& source, uint64_t* unpacked) {
  MarkCursor marks{bitmap, length / granule};
  return bdev_unpack_marked_sync(
      dst, offset, length, granule, bitmap, staging_bytes,
      [&](uint8_t* data, uint64_t first_rank, uint64_t count) {
        const int status = source(data, first_rank, count);
        if (status != 0) return status;
        for (uint64_t i = 0; i < count; ++i) {
          uint8_t* unit = data + i * granule;
          xts_decrypt_unit(keys, first_unit + marks.next(), unit, unit,
                           granule);
        }
        return 0;
      },
      unpacked);
}

// bdev_xts_pack_marked_sync (Chunk = PackSink) and
// bdev_xts_unpack_marked_sync (Chunk = UnpackSource): what is the key's
// to check, then the shared plan, then the GPU or the generic path.
template <typename Chunk>
int xts_marked_sync(Bdev* bdev, uint64_t offset, uint64_t length,
                    uint32_t granule, const std::vector<uint64_t>& bitmap,
                    const XtsKey& key, uint64_t staging_bytes,
                    const Chunk& chunk, uint64_t* moved_out) {
  return marked_call(moved_out, [&](uint64_t* moved) -> int {
    if (!xts_key_ok(key.key, key.len) || !xts_granule_ok(granule) ||
        length / granule > kXtsKcvUnit - key.first_unit) {
      return kIoInvalid;
    }
    MarkedPlan plan;
    const int status =
        plan_marked_windows(bdev, offset, length, granule, bitmap,
                            staging_bytes, static_cast<bool>(chunk), &plan);
    if (status != kIoOk || plan.marked == 0) return status;
    const XtsSchedules schedules(key.key);
    const int device = granule_kernel_device(bdev, bdev);
    if (device < 0) {
      return xts_generic(bdev, offset, length, granule, bitmap, schedules,
                         key.first_unit, staging_bytes, chunk, moved);
    }
    XtsStream xs(device, bdev, offset, granule, plan, schedules,
                 std::is_same<Chunk, PackSink>::value, key.first_unit);
    return xts_gpu(xs, plan, chunk, moved);
  });
}

}  // namespace

void xts_load_kernel_keys(const XtsSchedules& schedules, bool encrypt,
                          XtsKernelKeys* keys) {
  load_words(encrypt ? schedules.k1_enc : schedules.k1_dec, keys->data);
  load_words(schedules.k2_enc, keys->tweak);
}

void xts_var_launch(bool encrypt, hipStream_t stream, const uint8_t* from,
                    uint8_t* to, const uint32_t* sizes, const uint64_t* offsets,
                    const unsigned long long* bitmap,
                    const uint32_t* rank_before_word, const MarkedWindow& win,
                    uint32_t granule, uint64_t first_unit,
                    const XtsKernelKeys& keys) {
  hipLaunchKernelGGL(encrypt ? k_xts_var<true> : k_xts_var<false>,
                     dim3(wave_window_grid(win, kXtsThreads / 64)),
                     dim3(kXtsThreads), 0, stream, from, to, sizes, offsets,
                     bitmap, rank_before_word, win, granule, first_unit, keys);
  HIP_CHECK(hipGetLastError());
}

int bdev_xts_pack_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                              uint32_t granule,
                              const std::vector<uint64_t>& bitmap,
                              const XtsKey& key, uint64_t staging_bytes,
                              const PackSink& sink, uint64_t* packed) {
  return xts_marked_sync(src, src_offset, length, granule, bitmap, key,
                         staging_bytes, sink, packed);
}

int bdev_xts_unpack_marked_sync(Bdev* dst, uint64_t dst_offset,
                                uint64_t length, uint32_t granule,
                                const std::vector<uint64_t>& bitmap,
                                const XtsKey& key, uint64_t staging_bytes,
                                const UnpackSource& source,
                                uint64_t* unpacked) {
  return xts_marked_sync(dst, dst_offset, length, granule, bitmap, key,
                         staging_bytes, source, unpacked);
}

}  // namespace hipstore
