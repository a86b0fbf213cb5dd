// Compressed checkpoints: the HSLZ1 and HSLZD1 granule codecs and the
// marked compress / decompress calls under version-2 and version-4 delta
// files (delta.h).
//
// HSLZ1. A granule of G bytes (512 <= G <= 16384, G % 16 == 0) is
// compressed on its own and stored either as a legal LZ4 block (token,
// literal-length extension bytes, literals, 2-byte little-endian offset,
// match-length extension bytes; minimum match 4; the last 5 bytes are
// literals; no match starts after G - 12) or, when that block would not
// be smaller than G, as the G raw bytes. A stored size of G means raw.
// Any LZ4 block decoder decodes a stored block.
//
// The parse is normative: the host compressor below and
// k_lz_compress_marked (compress_ops.hip) emit identical bytes, so a
// file is fully determined by the content whichever path wrote it.
//   - table: 2048 slots, each empty or a position; hash(v) =
//     (v * 2654435761 mod 2^32) >> 21 of the little-endian u32 v.
//   - anchor = p = 0. While p <= G - 12, take the window of positions
//     q = p + l, 0 <= l < 64, q <= G - 12.
//   - Every q reads its candidate c = table[hash(u32 at q)] before any
//     position of the window is inserted. c is valid iff the slot is not
//     empty and the u32 at c equals the u32 at q (c < q and q - c <=
//     65535 hold by construction).
//   - The winner is the lowest q with a valid candidate. The positions
//     of the window up to and including the winner (all of them without
//     a winner) are inserted; a slot takes the greatest position
//     inserted into it, so the table never depends on an order.
//   - No winner: p += 64. Otherwise the match (q, c) of length 4 is
//     extended byte by byte while q + length < G - 5 and the bytes are
//     equal; the sequence (literals [anchor, q), offset q - c, length) is
//     emitted; anchor = p = q + length.
//   - The bytes from anchor to G are emitted as the final literals.
//
// HSLZD1 (version-4 delta files) compresses a granule X against a
// dictionary D of the same G bytes: the base granule of an incremental
// checkpoint. The image is B = D || X, positions 0 .. 2G - 1 (all fit 16
// bits). A stored piece is a legal LZ4 block that a decoder with D as
// prefix history turns into X (offsets reach back up to G + the bytes
// produced so far) or, when that block would not be smaller than G, the
// raw X. A stored size of G means raw, as in HSLZ1.
//
// The parse is HSLZ1's over B with these changes and no others:
//   - seeding: before the scan every position q < G is inserted into the
//     table under hash(u32 of B at q), so the last three read into X; a
//     slot takes the greatest position inserted.
//   - anchor = p = G; a window is q = p + l, 0 <= l < 64, q <= 2G - 12.
//   - the candidate of q is the aligned position q - G when the u32
//     there equals the u32 at q; otherwise the table candidate under
//     HSLZ1's rule. The aligned candidate needs no table and collisions
//     cannot displace it: a dictionary position i survives the seeding
//     only with probability about exp(-(G - i) / 2048).
//   - winner, inserts, extension (while q + length < 2G - 5), emission
//     and final literals are HSLZ1's with 2G for G; literal lengths and
//     the stored-size bound are relative to G (the output is X alone).
// lz_dict_compress_granule and k_lz_compress_marked<true> emit identical
// bytes.

#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "hipstore/bdev.h"
#include "hipstore/crypt.h"

namespace hipstore {

constexpr uint32_t kLzMinGranule = 512;
constexpr uint32_t kLzMaxGranule = 16384;
constexpr uint32_t kLzHashBits = 11;
constexpr uint32_t kLzHashMul = 2654435761u;
constexpr uint32_t kLzWindow = 64;

inline bool lz_granule_ok(uint64_t granule) {
  return granule >= kLzMinGranule && granule <= kLzMaxGranule &&
         granule % 16 == 0;
}

// A stored piece of `size` bytes starts 16-byte aligned in a window's
// dense stream and takes this much of it.
inline uint64_t lz_padded(uint64_t size) { return (size + 15) & ~15ull; }

// Compresses in[0, granule) into out[0, granule) and returns the stored
// size, 1 .. granule (granule = raw copy). lz_granule_ok required.
uint32_t lz_compress_granule(const uint8_t* in, uint32_t granule, uint8_t* out);

// Token walk without copying: true iff `piece` of `size` bytes is the raw
// granule (size == granule) or a block whose every offset is >= 1 and <=
// the bytes produced so far, whose reads stay inside the piece, whose
// output ends at exactly `granule` and which keeps the end-of-block
// rules (last sequence literals only, at least 5 of them unless the
// block is one literal run; no match starts after granule - 12). `why`
// receives the broken rule.
bool lz_validate_granule(const uint8_t* piece, uint64_t size, uint32_t granule,
                         std::string* why = nullptr);

// Decodes a stored piece into out[0, granule); false (with `why`) for
// exactly the pieces lz_validate_granule refuses. Never reads outside
// the piece or writes outside out.
bool lz_decompress_granule(const uint8_t* piece, uint64_t size,
                           uint32_t granule, uint8_t* out,
                           std::string* why = nullptr);

// The same three for HSLZD1. in, dict and out hold `granule` bytes each
// and out overlaps neither. The validator is the same token walk with
// offsets >= 1 and <= granule + the bytes produced so far: it needs no
// dictionary bytes. The decoder never reads outside the piece or dict[0,
// granule) and never writes outside out; with another dictionary than
// the compressor's it gives other bytes, not an error.
uint32_t lz_dict_compress_granule(const uint8_t* in, const uint8_t* dict,
                                  uint32_t granule, uint8_t* out);
bool lz_dict_validate_granule(const uint8_t* piece, uint64_t size,
                              uint32_t granule, std::string* why = nullptr);
bool lz_dict_decompress_granule(const uint8_t* piece, uint64_t size,
                                uint32_t granule, const uint8_t* dict,
                                uint8_t* out, std::string* why = nullptr);

// What the two marked calls below take besides their range.
struct LzOptions {
  // As bdev_pack_marked_sync's: 0 for the default, else at least a granule.
  uint64_t staging_bytes = 0;
  // Set (key or len) for a keyed call, see below.
  XtsKey key;
  // HSLZD1, compress: granule g of the range is compressed against
  // granule g of the range of `base` at base_offset. Null for HSLZ1.
  Bdev* base = nullptr;
  uint64_t base_offset = 0;
  // HSLZD1, decompress: the target is its own dictionary.
  bool dictionary = false;
};

// bdev_pack_marked_sync with every granule compressed: sink(data, sizes,
// first_rank, count) receives the stored sizes of marked granules
// first_rank .. first_rank + count - 1 and their pieces in `data`, piece
// i at the sum of lz_padded(sizes[j]) over j < i, pad bytes 0. Same
// chunks, validation and path selection as bdev_pack_marked_sync; also
// kIoInvalid unless lz_granule_ok. An HBM bdev with a usable GPU runs
// k_lz_compress_marked and k_gather_var per window, so only stored bytes
// cross PCIe; every other bdev goes through bdev_pack_marked_sync's
// generic path and lz_compress_granule. Both paths hand the sink the
// same chunks and the same bytes.
//
// With options.base (HSLZD1): `base` has the same block size and both
// ranges are valid. The kernel path (k_lz_compress_marked<true>) applies
// when both bdevs are HBM-resident and reachable from one device, as for
// bdev_diff_sync; otherwise both are read through the bdev interface in
// spans of at most 1 MiB and lz_dict_compress_granule does the work. Same
// chunks and bytes on both paths. Ranges that overlap in one backing
// store are kIoInvalid, as in bdev_copy_marked_sync.
using CompressSink = std::function<int(const uint8_t* data,
                                       const uint32_t* sizes,
                                       uint64_t first_rank, uint64_t count)>;
int bdev_compress_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                              uint32_t granule,
                              const std::vector<uint64_t>& bitmap,
                              const LzOptions& options,
                              const CompressSink& sink,
                              uint64_t* packed = nullptr,
                              std::string* error = nullptr);

// The inverse: source(data, sizes, first_rank, count) fills the stored
// sizes and the pieces of the next chunk in the layout above (`data` has
// room for count * granule bytes). Every piece is checked with
// lz_validate_granule on the host before anything is decoded or reaches
// the GPU; a bad piece is kIoInvalid and `error` names the granule.
// Chunks delivered before it stay written. HBM bdevs decode in
// k_lz_decompress_marked, which bounds every index on its own and
// reports a piece it had to give up in a per-window flag array: such a
// piece is kIoFailed. options.base is not used.
//
// With options.dictionary (HSLZD1): the dictionary of a granule is what
// the target holds there when the call reaches it, so the target must be
// at the base state and the call is not idempotent. Pieces are checked
// with lz_dict_validate_granule first. k_lz_decompress_marked<true, ...>
// reads a granule into LDS before it overwrites it and touches no other.
using DecompressSource = std::function<int(uint8_t* data, uint32_t* sizes,
                                           uint64_t first_rank,
                                           uint64_t count)>;
int bdev_decompress_marked_sync(Bdev* dst, uint64_t dst_offset,
                                uint64_t length, uint32_t granule,
                                const std::vector<uint64_t>& bitmap,
                                const LzOptions& options,
                                const DecompressSource& source,
                                uint64_t* unpacked = nullptr,
                                std::string* error = nullptr);

// Keyed calls. With options.key (the 64 bytes of crypt.h and a first unit
// number), with or without a dictionary, every piece is one HSXTS2 unit
// whose number is first_unit + the granule's index in the range, and only
// ciphertext reaches the sink or comes from the source. `sizes` stay the
// true stored sizes; piece i sits at the sum of lz_padded(max(sizes[j],
// 16)) over j < i, because a piece shorter than a cipher block is stored
// as one zero-padded block. kIoInvalid unless xts_key_ok and first_unit +
// the range's granules stays below 2^64-1, before anything runs.
//   compress, HBM: k_xts_var takes k_gather_var's place and encrypts the
//     pieces on their way from device scratch to pinned memory, so no
//     plaintext crosses PCIe or sits in pinned host memory.
//   decompress, HBM: the host sees only ciphertext and checks the sizes
//     alone. k_xts_var decrypts the window into device scratch and the
//     decode kernels run in strict mode, where they accept exactly the
//     pieces lz_validate_granule (lz_dict_validate_granule) accepts; a
//     piece they refuse is kIoInvalid, `error` names the granule and the
//     granule is left alone.
//   every other bdev: xts_encrypt_var / xts_decrypt_var on the host, then
//     the host validators as without a key. Both paths hand over the same
//     chunks and bytes and refuse the same pieces.

}  // namespace hipstore
