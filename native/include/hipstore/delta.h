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

#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hipstore/bdev.h"

namespace hipstore {

constexpr uint32_t kDeltaVersion = 1;
constexpr uint32_t kDeltaFlagFull = 1;
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
int bdev_import_delta(Bdev* dst, const std::string& path, bool dry_run,
                      DeltaInfo* stats, std::string* error);

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

constexpr uint32_t kFingerprintMapVersion = 1;
constexpr uint64_t kFingerprintMapRecord = 65536;  // fingerprints per record

struct FingerprintMapInfo {
  uint32_t version = 0;
  uint32_t block_size = 0;
  uint32_t granule = 0;
  uint32_t algorithm = 0;
  uint64_t volume_bytes = 0;
  uint64_t n_granules = 0;
  uint64_t file_bytes = 0;
};

// Writes the fingerprint map of the whole of `bdev` to `path` (tmp file,
// sync, rename; an existing file is refused without `overwrite`).
// granule 0 = the block size.
int bdev_fingerprint_file(Bdev* bdev, const std::string& path,
                          uint32_t granule, bool overwrite,
                          FingerprintMapInfo* stats, std::string* error);

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
int bdev_verify_fingerprints(Bdev* bdev, const std::string& path,
                             uint32_t max_report, FingerprintVerify* stats,
                             std::string* error);

// bdev_export_delta with fingerprint maps. `base_map` names the map of
// the base state and replaces `base` (giving both is kIoInvalid): one
// fingerprint pass of `src`, then granule g is exported when it lies at
// or past the map's n_granules (a grown volume) or its fingerprint
// differs. The file is a normal version-1 delta (flags 0), byte for byte
// what a clone of that state as `base` gives, up to the fingerprint's
// 2^-64 miss probability. granule 0 = the map's granule; any other
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
struct DeltaMaps {
  std::string base_map;
  std::string map_out;
  uint64_t map_bytes = 0;  // out: size of the file written to map_out
};
int bdev_export_delta(Bdev* src, Bdev* base, const std::string& path,
                      uint32_t granule, bool overwrite, DeltaMaps* maps,
                      DeltaInfo* stats, std::string* error);

}  // namespace hipstore
