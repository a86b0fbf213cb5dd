// P+Q parity across bdevs: encode, check (scrub), rebuild and update as
// bulk operations, SnapRAID-like: encode while a set of volumes is
// quiescent, scrub whenever wanted, rebuild onto fresh volumes after a
// loss, update from clones of the members' earlier state. There is no
// live composite bdev here; the only read-modify-write of parity is the
// update call, offline like the rest.
//
// Definitions (every path produces exactly these bytes):
//   - Field: GF(2^8), polynomial x^8+x^4+x^3+x^2+1 (0x11D), generator
//     g = 2.
//   - Data member i (0 <= i < k, 1 <= k <= 32) contributes the range
//     [offset_i, offset_i + length) of its bdev.
//   - Per byte position: P = D_0 ^ D_1 ^ ... ^ D_{k-1},
//     Q = sum over i of g^i * D_i.
//   - Rebuild: S_P = stored P ^ P of the surviving data, S_Q likewise.
//       one data member x lost, P usable:  D_x = S_P
//       one data member x lost, Q only:    D_x = g^-x * S_Q
//       two data members x < y lost:       d = (g^(y-x) ^ 1)^-1,
//         A = g^(y-x) * d, B = g^-x * d,
//         D_x = A * S_P ^ B * S_Q, D_y = S_P ^ D_x
//     Lost parity is recomputed by an encode pass once the data is back.
//   - Update: `bases` has one slot per data member, a bdev range or
//     absent. A member with a base is tracked: its base holds the
//     member's bytes as of the moment the stored parity was last right.
//     At least one member is tracked; untracked members are taken as
//     unchanged and are not read. Per byte position, over the tracked
//     members i with d_i = D_i ^ B_i:
//       P ^= XOR of the d_i,  Q ^= XOR of g^i * d_i
//     Bit g of the result's bitmap is set iff some tracked member differs
//     from its base anywhere in granule g, which is not "the parity delta
//     is non-zero": three or more members can change so that both deltas
//     cancel, and such a granule is still reported (and refreshed).
//     Parity bytes of a granule whose bit is clear are not written. With
//     `refresh`, a tracked member's bytes are also stored into its base
//     wherever the two differ, so afterwards every base equals its member
//     over the range and a second call is a no-op (0 granules, parity
//     untouched). Without it the bases keep their bytes and a second call
//     XORs the same deltas in again, which undoes the first: by
//     definition, the caller re-clones or refreshes between cycles.
//
// When every member is HBM-resident, 16-byte aligned and reachable from
// one device, the call runs on the GPU (parity_ops.hip: Horner form,
// packed doubling, no tables). Every other set goes through
// bdev_read_sync / bdev_write_sync in spans of at most 1 MiB with
// byte-wise log/exp table arithmetic (parity.cpp), a different algorithm
// on purpose. Both give identical bytes and bitmaps. A set that spans
// GPUs reads its remote members over peer access; that path has not been
// executed (single-GPU test machines), like composite.cpp's peer paths.

#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hipstore/bdev.h"
#include "hipstore/engine.h"

namespace hipstore {

constexpr uint32_t kParityMaxData = 32;

// GF(2^8) over 0x11D, log/exp tables (parity.cpp).
uint8_t gf256_mul(uint8_t a, uint8_t b);
uint8_t gf256_inv(uint8_t a);    // a != 0
uint8_t gf256_pow2(int exponent);  // g^exponent, any sign

// out_a = a * S_P ^ b * S_Q is the lower of the lost data members.
struct ParityCoeffs {
  uint8_t a = 0;
  uint8_t b = 0;
};
ParityCoeffs parity_coeffs_one_by_q(uint32_t x);         // (0, g^-x)
ParityCoeffs parity_coeffs_two(uint32_t x, uint32_t y);  // x < y: (A, B)

struct ParityMember {
  Bdev* bdev = nullptr;  // nullptr = absent (P or Q only)
  uint64_t offset = 0;
};

// Entries of `lost`: a data index, or one of these.
constexpr int kParityLostP = -1;
constexpr int kParityLostQ = -2;

// Filled on every return: the rule that was broken when the status is
// not kIoOk, and whether the GPU path carried the call.
struct ParityReport {
  std::string error;
  bool on_gpu = false;
};

// All four calls return IoStatus and never throw. kIoInvalid unless:
// 1 <= k <= 32; P or Q given; all members share a block size; length is
// non-zero and a multiple of the block size and of 16; offsets are
// multiples of the block size; every range is in bounds; no bdev and no
// backing store appears twice. A call that would write a claimed() bdev
// returns kIoFailed (offline only, the rule of replica scrub repair).

// Writes P and / or Q of the data members.
int bdev_parity_encode_sync(const std::vector<ParityMember>& data,
                            ParityMember p, ParityMember q, uint64_t length,
                            ParityReport* report = nullptr);

// Recomputes the given parity and compares it with what is stored,
// granule by granule (DiffStats and bitmap layout of bdev_diff_sync; bit
// g is set iff granule g of the stored parity differs from the parity of
// the data). Also kIoInvalid unless `granule` is a multiple of the block
// size and of 16, length is a multiple of it and the granule count is
// within bdev_diff_sync's limit. An absent parity reports 0 granules.
struct ParityCheck {
  DiffStats p;
  DiffStats q;
  std::vector<uint64_t> p_bitmap;
  std::vector<uint64_t> q_bitmap;
};
int bdev_parity_check_sync(const std::vector<ParityMember>& data,
                           ParityMember p, ParityMember q, uint64_t length,
                           uint32_t granule, uint32_t max_report,
                           ParityCheck* out, ParityReport* report = nullptr);

// Rewrites the one or two members named by `lost`; the bdevs passed in
// those slots are the targets, every other member is only read. Also
// kIoInvalid for an empty `lost`, more than two entries, a duplicate, a
// data index >= k, a lost parity that is not given, or a loss the
// remaining parity cannot cover (a lost data member needs one usable
// parity, two need both).
int bdev_parity_rebuild_sync(const std::vector<ParityMember>& data,
                             ParityMember p, ParityMember q, uint64_t length,
                             const std::vector<int>& lost,
                             ParityReport* report = nullptr);

// Brings the stored P and / or Q up to date from the tracked members and
// their bases (definitions above); `changed` and `bitmap` have the layout
// of bdev_diff_sync, tail bits 0, under the granule rules of the check
// call. Also kIoInvalid unless bases.size() == k with at least one base
// present, every base has the set's block size, a block-aligned offset
// and its range in bounds, and no base shares a bdev or backing store
// with a member, a parity or another base. A claimed P or Q, and with
// `refresh` a claimed base, returns kIoFailed. Data members are only
// read: claimed ones are allowed and advisory.
int bdev_parity_update_sync(const std::vector<ParityMember>& data,
                            ParityMember p, ParityMember q,
                            const std::vector<ParityMember>& bases,
                            uint64_t length, uint32_t granule,
                            uint32_t max_report, bool refresh,
                            DiffStats* changed, std::vector<uint64_t>* bitmap,
                            ParityReport* report = nullptr);

// Default extent of the RPC and Python front ends: what is left of the
// shortest member after its offset, rounded down to a multiple of
// `unit`; 0 when an offset lies past its device.
uint64_t parity_common_length(const std::vector<ParityMember>& data,
                              ParityMember p, ParityMember q, uint64_t unit);

// --- GPU path (parity_ops.hip); parity.cpp calls these after validation ---

// Member base pointers with the offsets applied, by value in the kernel
// arguments. A null slot is a lost member (rebuild) or, in the bases of
// an update, an untracked one.
struct ParitySet {
  const uint8_t* data[kParityMaxData];
  uint32_t k;
};

// Device to run on, or -1 for the generic path: every member
// HBM-resident and reachable from the device of `members[0]` (peer
// access enabled on the way).
int parity_kernel_device(const std::vector<Bdev*>& members);

// Null `p` / `q`: that parity is not written / checked / read.
int parity_encode_gpu(int device, const ParitySet& set, uint8_t* p, uint8_t* q,
                      uint64_t length);
int parity_check_gpu(int device, const ParitySet& set, const uint8_t* p,
                     const uint8_t* q, uint64_t n_granules, uint32_t granule,
                     std::vector<uint64_t>* p_words,
                     std::vector<uint64_t>* q_words);
// out_a = a * S_P ^ b * S_Q; out_b (may be null) = S_P ^ out_a.
int parity_rebuild_gpu(int device, const ParitySet& set, const uint8_t* p,
                       const uint8_t* q, ParityCoeffs coeffs, uint8_t* out_a,
                       uint8_t* out_b, uint64_t length);
// `bases`: slot i is member i's base or null, k as in `set`; written
// only with `refresh`. Null `p` / `q`: that parity is not updated.
int parity_update_gpu(int device, const ParitySet& set, const ParitySet& bases,
                      uint8_t* p, uint8_t* q, uint64_t n_granules,
                      uint32_t granule, bool refresh,
                      std::vector<uint64_t>* words);

}  // namespace hipstore
