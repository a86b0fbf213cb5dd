// Incremental checkpoints of bdevs to files ("hipstore delta file,
// version 1"): the third persistence escape next to save_config
// (topology only) and AIO bdevs (never in HBM). A file holds the marked
// granules of a volume as one dense stream (bdev_pack_marked_sync), so
// an HBM volume leaves the GPU in one launch per staging window.
//
// Layout, little-endian, fully determined by the content:
//   header, 64 bytes:
//     "HSDELTA1", u32 version = 1, u32 block_size, u32 granule,
//     u32 flags (bit 0 = full: no base, every granule present),
//     u64 volume_bytes, u64 n_granules, u64 n_marked, u32 bitmap_crc,
//     u32 0, u32 0, u32 header_crc (CRC32C of bytes 0-59)
//   bitmap: ceil(n_granules / 64) * 8 bytes, bdev_diff_sync layout,
//     tail bits 0
//   records, each the next min(remaining, max(1, 2^20 / granule)) marked
//     granules: u32 count, u32 crc32c(payload), count * granule bytes
//   trailer, 16 bytes: "HSDEND1\0", u64 n_marked
// All CRCs are crc32c_sw(0, ...).
//
// "hipstore delta file, version 2" holds the same granules compressed
// (HSLZ1, compress.h) and is what an export with `compress` writes;
// without it every file is version 1, byte for byte as above. Version 2
// differs in three places:
//   - version = 2 and flags bit 1 (kDeltaFlagLz) set; one implies the other
//   - the two spare header words are one u64 record_area_bytes, the
//     length of the record stream, so the exact file length still follows
//     from the header
//   - records, cut as in version 1: u32 count, u32 crc32c(payload),
//     u32 payload_bytes, u32 0, then the payload: count u32 stored sizes
//     (1 .. granule; granule = raw), then the pieces back to back,
//     unpadded
// Import tells the versions apart by itself. A version-2 record's CRC,
// its sizes and then every piece (lz_validate_granule) are checked
// before a byte of it is decoded or reaches the GPU.
//
// "hipstore delta file, version 3" holds the same granules encrypted
// (HSXTS1, crypt.h; the data unit is the granule and its number the
// granule's index in the volume) and is what an export with a key
// writes. XTS preserves length, so it is the version-1 layout with three
// differences:
//   - version = 3 and flags bit 2 (kDeltaFlagXts) set; one implies the other
//   - the first spare header word is xts_kcv(key), the second stays 0
//   - record payloads are ciphertext
// Record CRCs, the bitmap CRC and the exact-length rule are computed over
// the file as stored, so the structural pass and a dry run need no key.
// There is no authentication (a CRC is not a MAC), and a key together
// with `compress` is refused unless `cts` asks for version 5:
// compress-then-encrypt needs ciphertext stealing, which older readers
// do not have.
//
// "hipstore delta file, version 4" holds the granules of an incremental
// compressed against the base (HSLZD1, compress.h: the dictionary of a
// granule is the same granule of the base volume) and is what an export
// with `compress`, `dictionary` and a clone as `base` writes. The layout
// is exactly version 2's (header, bitmap, var records, record_area_bytes,
// trailer) with
//   - version = 4 and flags bit 1 (kDeltaFlagLz) and bit 3
//     (kDeltaFlagDict) both set; version 4 if and only if bit 3, and bit 3
//     implies bit 1
// and the import checks are version 2's too: the validator needs no
// dictionary bytes, so the structural pass, the record CRCs, the host
// validation of every piece before it reaches the GPU and dry_run work as
// for version 2. The dictionary of a granule at import is what the target
// holds there, so a version-4 import is NOT idempotent: after a bad
// record or a second application the granules already written are no
// longer the dictionary. The file does not identify its base (as no delta
// file does), with sharper consequences: applied to a volume that is not
// at the base state it decodes memory-safely into wrong data. A map_out
// map of the export plus bdev_verify_fingerprints after the import is the
// check.
//
// "hipstore delta file, version 5" holds the granules compressed and then
// encrypted (HSLZ1 or HSLZD1 pieces, each one HSXTS2 data unit, crypt.h:
// XTS with ciphertext stealing; the unit number is the granule's index in
// the volume) and is what an export with `compress`, a key and `cts`
// writes. The layout is version 2's with
//   - version = 5 and flags bit 1 (kDeltaFlagLz) and bit 2 (kDeltaFlagXts)
//     both set; version 5 if and only if both; bit 3 (kDeltaFlagDict) says
//     whether the pieces are HSLZD1, with version 4's rules for the base
//   - a 16-byte key block directly after the bitmap: "HSKC", u32
//     xts_kcv(key), u32 0, u32 crc32c of those 12 bytes; record_area_bytes
//     does not count it, and the exact file length still follows from the
//     header
//   - in a record's payload a piece occupies max(size, 16) bytes: a piece
//     shorter than one cipher block is stored as one zero-padded encrypted
//     block. The sizes stay the true stored sizes, 1 .. granule.
// Record CRCs, the bitmap CRC, the range check of the sizes and the
// exact-length rule are computed over the file as stored, so the
// structural pass and a dry run need no key; a wrong key is refused by
// kcv before the target is touched. The pieces can be validated only
// after decryption: on an HBM target that happens on the GPU, in the
// strict decode (compress.h), otherwise on the host; both refuse the same
// files, name the granule and leave it unwritten. Stored sizes are in the
// clear, so the file shows how compressible every granule is; equal
// granule index, key and plaintext give equal ciphertext across files, as
// in version 3; and there is still no authentication.

#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hipstore/bdev.h"

namespace hipstore {

constexpr uint32_t kDeltaVersion = 1;
constexpr uint32_t kDeltaVersionLz = 2;
constexpr uint32_t kDeltaFlagFull = 1;
constexpr uint32_t kDeltaVersionXts = 3;
constexpr uint32_t kDeltaFlagLz = 2;
constexpr uint32_t kDeltaFlagXts = 4;
constexpr uint32_t kDeltaVersionDict = 4;
constexpr uint32_t kDeltaFlagDict = 8;
constexpr uint32_t kDeltaVersionCts = 5;
constexpr uint64_t kDeltaHeaderBytes = 64;
constexpr uint64_t kDeltaTrailerBytes = 16;
constexpr uint64_t kDeltaRecordBytes = 1ull << 20;

struct DeltaInfo {
  uint32_t version = 0;
  uint32_t block_size = 0;
  uint32_t granule = 0;
  bool full = false;
  uint64_t volume_bytes = 0;
  uint64_t n_granules = 0;
  uint64_t n_marked = 0;  // granules in the file (saved / applied)
  uint64_t file_bytes = 0;
  bool compressed = false;  // versions 2, 4 and 5
  // Bytes the granules take in the file: n_marked * granule, or the sum
  // of the stored sizes of a compressed file.
  uint64_t stored_bytes = 0;
  bool encrypted = false;  // versions 3 and 5
  bool dictionary = false;  // version 4, or 5 with bit 3 (then also compressed)
};

// Every call returns an IoStatus and, on failure, a one-line reason in
// `error`: kIoInvalid for bad parameters, mismatched geometry and
// malformed or corrupt files; kIoFailed for I/O failures, a claimed
// import target and an existing file without `overwrite`.

// Writes the granules of `src` that differ from `base` (whole device,
// bdev_diff_sync; equal block size and size required), or every granule
// when `base` is null, to `path`. granule 0 = the block size. The file
// appears under its final name only complete: it is written to
// path + ".tmp", synced and renamed. Exporting a claimed volume is
// allowed and advisory (crash-consistent at best).
int bdev_export_delta(Bdev* src, Bdev* base, const std::string& path,
                      uint32_t granule, bool overwrite, DeltaInfo* stats,
                      std::string* error);

// Applies a delta file to `dst` from offset 0. A structural pass
// (magic, version, both header CRCs, popcount, tail bits, exact file
// length, trailer, block size, volume_bytes <= size of dst) runs before
// the target is touched; records are then streamed through
// bdev_unpack_marked_sync, each CRC checked before its bytes are handed
// on. A bad record stops the import with the target partly updated.
// dry_run runs every check and writes nothing. A claimed target is
// refused.
//
// `key` (the 64 bytes of crypt.h) is required for a version-3 or
// version-5 file and kIoInvalid for any other; a key whose xts_kcv differs
// from the file's is kIoInvalid before the target is touched. dry_run of
// such a file works without a key (structure and CRCs, so a file can be
// vetted where the key is not) and with one also checks the kcv and, for
// version 5, decrypts and validates every piece.
int bdev_import_delta(Bdev* dst, const std::string& path, bool dry_run,
                      DeltaInfo* stats, std::string* error,
                      const std::vector<uint8_t>* key = nullptr);

// Header fields of a file after the structural pass.
int delta_file_info(const std::string& path, DeltaInfo* info,
                    std::string* error);

// --- fingerprint maps ("hipstore fingerprint map, version 1") ---------------
//
// The fingerprints (fingerprint.h) of every granule of a volume, kept in
// a file next to a checkpoint so that the next incremental checkpoint
// needs no live clone of its base, and so that a restored volume can be
// verified, or a volume scrubbed, without a second copy.
//
// Layout, little-endian, fully determined by the content:
//   header, 64 bytes:
//     "HSFPMAP1", u32 version = 1, u32 block_size, u32 granule,
//     u32 algorithm = 1, u64 volume_bytes, u64 n_granules, 20 reserved
//     bytes of 0 (the delta header's n_marked, bitmap_crc and two spare
//     words), u32 header_crc (CRC32C of bytes 0-59)
//   records, each the next min(remaining, 65536) fingerprints:
//     u32 count, u32 crc32c(payload), count * 16 bytes
//   trailer, 16 bytes: "HSFPEND1", u64 n_granules
// Reading starts with a structural pass (magic, version, algorithm,
// header CRC, zero reserved fields, consistent geometry, exact file
// length, trailer); every record's CRC is then checked before its bytes
// are used.
//
// "hipstore fingerprint map, version 2" holds HSFP2 fingerprints
// (fingerprint.h: BLAKE2s, 16 bytes each) and is what a call with
// map_algorithm "blake2s" writes; without it every map is version 1, byte
// for byte as above. Same magics, same layout; it differs in the header:
//   - version = 2 and algorithm = 2 (unkeyed) or 3 (keyed); version 2
//     implies one of these and they imply version 2
//   - algorithm 3: the first reserved u32 (header bytes 40-43) is
//     blake2s_kcv(key); every other reserved byte stays 0
// A keyed map is a MAC over the volume: whoever rewrites a delta file or
// the volume cannot write a map that matches without the key. The record
// CRCs and the structural pass need no key.

constexpr uint32_t kFingerprintMapVersion = 1;
constexpr uint32_t kFingerprintMapVersionBlake2s = 2;
constexpr uint64_t kFingerprintMapRecord = 65536;  // fingerprints per record

// What a caller says about the fingerprints of the maps of a call.
// `algorithm` 0 leaves it open: HSFP1 for a new map, whatever an existing
// map holds otherwise. kMapBlake2s with a key is algorithm id 3, without
// one id 2. The key is 32 bytes (kBlake2sKeyBytes).
constexpr uint32_t kMapHsfp1 = 1;
constexpr uint32_t kMapBlake2s = 2;
struct MapKind {
  uint32_t algorithm = 0;
  const std::vector<uint8_t>* key = nullptr;
};

struct FingerprintMapInfo {
  uint32_t version = 0;
  uint32_t block_size = 0;
  uint32_t granule = 0;
  uint32_t algorithm = 0;
  uint64_t volume_bytes = 0;
  uint64_t n_granules = 0;
  uint64_t file_bytes = 0;
  bool keyed = false;  // algorithm 3
};

// Writes the fingerprint map of the whole of `bdev` to `path` (tmp file,
// sync, rename; an existing file is refused without `overwrite`).
// granule 0 = the block size. `kind`: a key of another length than 32, or
// a key without kMapBlake2s, is kIoInvalid before the volume is read.
int bdev_fingerprint_file(Bdev* bdev, const std::string& path,
                          uint32_t granule, bool overwrite,
                          FingerprintMapInfo* stats, std::string* error,
                          const MapKind& kind = MapKind());

// Header fields of a map after the structural pass and every record CRC.
int fingerprint_map_info(const std::string& path, FingerprintMapInfo* info,
                         std::string* error);

// Recomputes the fingerprints of `bdev` over the map's range (from
// offset 0, the map's granule) and compares. Requires equal block size
// and the map's volume_bytes <= the size of `bdev`. Only reads: allowed
// on a claimed volume and advisory there, like bdev_diff_sync.
struct FingerprintVerify {
  uint32_t granule = 0;
  uint64_t granules = 0;
  uint64_t mismatched = 0;
  // First max_report mismatching granule indices, ascending.
  std::vector<uint64_t> first_mismatches;
};
// The map decides the algorithm: a `kind` that names the other one, a
// keyed map without a key, a key for an unkeyed map and a key whose kcv
// differs from the header's are kIoInvalid before the volume is read.
int bdev_verify_fingerprints(Bdev* bdev, const std::string& path,
                             uint32_t max_report, FingerprintVerify* stats,
                             std::string* error,
                             const MapKind& kind = MapKind());

// bdev_export_delta with fingerprint maps. `base_map` names the map of
// the base state and replaces `base` (giving both is kIoInvalid): one
// fingerprint pass of `src`, then granule g is exported when it lies at
// or past the map's n_granules (a grown volume) or its fingerprint
// differs. The file is a normal delta (flags 0), byte for byte what a
// clone of that state as `base` gives, up to the fingerprint's 2^-64
// miss probability. granule 0 = the map's granule; any other
// granule than the map's, another block size or a map larger than `src`
// is kIoInvalid.
//
// `map_out` names where to write the map of `src` as exported: the
// base_map pass is reused, otherwise a pass of its own runs before the
// pack. It is renamed into place only after the delta file is, and may
// name the same file as `base_map` when `overwrite` is set. A write
// that lands between the fingerprint pass and the pack pass of a claimed
// volume leaves the new map older than the exported data, so the next
// delta exports that granule again: the safe direction.
//
// `compress` writes a version-2 file; the granule must then satisfy
// lz_granule_ok (kIoInvalid otherwise). Maps are unaffected: they
// describe the volume, not the file.
//
// `key` writes a version-3 file (granule <= 2^24; a key of another
// length, with equal halves, or together with `compress` is kIoInvalid).
// `base`, `base_map` and `map_out` work unchanged with it.
//
// `dictionary` writes a version-4 file: every granule is compressed
// against the same granule of `base`. It needs `compress` and `base` (a
// clone, whose bytes are the dictionaries): without `compress`, without
// `base` (a full export or `base_map`, which has no base bytes) or
// together with `key` it is kIoInvalid before anything is written.
//
// `cts` writes a version-5 file: `compress` and `key` together, with or
// without `dictionary`. It is opt-in because older readers cannot read
// version 5: without it `key` with `compress` and `dictionary` with `key`
// stay refused. `cts` without both `key` and `compress` is kIoInvalid.
//
// `kind` says which fingerprints the maps hold. With `base_map`, the pass
// and `map_out` take the base map's algorithm and the rules of
// bdev_verify_fingerprints apply; without, `map_out` is written as `kind`
// says (default HSFP1, version 1). A kind without either map is
// kIoInvalid. All of this is settled before anything is written.
struct DeltaMaps {
  std::string base_map;
  std::string map_out;
  uint64_t map_bytes = 0;  // out: size of the file written to map_out
  MapKind kind;
};
int bdev_export_delta(Bdev* src, Bdev* base, const std::string& path,
                      uint32_t granule, bool overwrite, DeltaMaps* maps,
                      DeltaInfo* stats, std::string* error,
                      bool compress = false,
                      const std::vector<uint8_t>* key = nullptr,
                      bool dictionary = false, bool cts = false);

}  // namespace hipstore
