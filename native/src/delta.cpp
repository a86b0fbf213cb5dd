// hipstore delta files: export / import of marked granules, and
// fingerprint maps (delta.h). Both formats sit on checked_file.h; here
// is what each format owns, and the passes over the volume.

#include "hipstore/delta.h"

#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <vector>

#include "checked_file.h"
#include "hipstore/engine.h"
#include "hipstore/fingerprint.h"

namespace hipstore {

using namespace checked_file;

namespace {

static_assert(kDeltaHeaderBytes == kHeaderBytes &&
                  kDeltaTrailerBytes == kTrailerBytes,
              "delta.h documents the core's header and trailer");

const Format kDelta = {{'H', 'S', 'D', 'E', 'L', 'T', 'A', '1'},
                       {'H', 'S', 'D', 'E', 'N', 'D', '1', '\0'},
                       kDeltaVersion, "delta file"};
const Format kMap = {{'H', 'S', 'F', 'P', 'M', 'A', 'P', '1'},
                     {'H', 'S', 'F', 'P', 'E', 'N', 'D', '1'},
                     kFingerprintMapVersion, "fingerprint map"};

const char kBadGranule[] =
    "invalid granule (a multiple of the block size and of 16 that divides "
    "the volume size)";

uint64_t record_granules(uint32_t granule) {
  return std::max<uint64_t>(1, kDeltaRecordBytes / granule);
}

uint64_t popcount(const std::vector<uint64_t>& bitmap) {
  uint64_t n = 0;
  for (uint64_t word : bitmap) {
    n += static_cast<uint64_t>(__builtin_popcountll(word));
  }
  return n;
}

// The first max_report set bits, ascending.
std::vector<uint64_t> first_set_bits(const std::vector<uint64_t>& bitmap,
                                     uint32_t max_report) {
  std::vector<uint64_t> out;
  for (uint64_t w = 0; w < bitmap.size() && out.size() < max_report; ++w) {
    for (uint64_t word = bitmap[w]; word != 0 && out.size() < max_report;
         word &= word - 1) {
      out.push_back(w * 64 + static_cast<uint64_t>(__builtin_ctzll(word)));
    }
  }
  return out;
}

int refuse_existing(const std::string& path, bool overwrite,
                    std::string* error) {
  struct stat st;
  if (!overwrite && lstat(path.c_str(), &st) == 0) {
    return fail(error, kIoFailed, path + " exists (overwrite not set)");
  }
  return kIoOk;
}

// --- delta files --------------------------------------------------------------

struct ParsedDelta {
  InFile in;
  DeltaInfo info;
  std::vector<uint64_t> bitmap;
  uint64_t records_offset = 0;
};

// The structural pass: everything that can be checked without reading
// a record payload.
int parse_delta(const std::string& path, ParsedDelta* out,
                std::string* error) {
  InFile& in = out->in;
  int status = in.open(path, kDelta, error);
  if (status != kIoOk) return status;
  const Header& h = in.header;
  DeltaInfo& info = out->info;
  info.version = kDeltaVersion;
  info.block_size = h.block_size;
  info.granule = h.granule;
  info.full = (h.word & kDeltaFlagFull) != 0;
  info.volume_bytes = h.volume_bytes;
  info.n_granules = h.n_granules;
  info.n_marked = get_u64(h.owned);
  info.file_bytes = in.file_bytes;
  if ((h.word & ~kDeltaFlagFull) != 0 || get_u32(h.owned + 12) != 0 ||
      get_u32(h.owned + 16) != 0) {
    return fail(error, kIoInvalid, "unknown flags or non-zero reserved field");
  }
  if (!geometry_ok(h.block_size, h.granule, h.volume_bytes, h.n_granules) ||
      info.n_marked > info.n_granules ||
      (info.full && info.n_marked != info.n_granules)) {
    return fail(error, kIoInvalid, "inconsistent geometry in header");
  }
  const uint64_t n_words = (info.n_granules + 63) / 64;
  status = in.check_length(
      n_words * 8 + record_stream_bytes(info.n_marked, info.granule,
                                        record_granules(info.granule)),
      error);
  if (status != kIoOk) return status;
  std::vector<uint8_t> raw(n_words * 8);
  if (!in.read(raw.data(), raw.size(), kHeaderBytes)) {
    return fail(error, kIoFailed, "cannot read bitmap");
  }
  if (crc32c_sw(0, raw.data(), raw.size()) != get_u32(h.owned + 8)) {
    return fail(error, kIoInvalid, "bitmap CRC mismatch");
  }
  out->bitmap.resize(n_words);
  for (uint64_t w = 0; w < n_words; ++w) {
    out->bitmap[w] = get_u64(&raw[w * 8]);
  }
  if (info.n_granules % 64 != 0 &&
      (out->bitmap.back() >> (info.n_granules % 64)) != 0) {
    return fail(error, kIoInvalid, "bitmap has bits past the last granule");
  }
  if (popcount(out->bitmap) != info.n_marked) {
    return fail(error, kIoInvalid, "n_marked disagrees with the bitmap");
  }
  out->records_offset = kHeaderBytes + raw.size();
  return in.check_trailer(info.n_marked, error);
}

// Header, bitmap, the marked granules of `src` as records, trailer, all
// synced. Fills info->file_bytes.
int write_delta(OutFile* out, Bdev* src, const std::vector<uint64_t>& bitmap,
                DeltaInfo* info, std::string* error) {
  std::vector<uint8_t> raw(bitmap.size() * 8);
  for (size_t w = 0; w < bitmap.size(); ++w) put_u64(&raw[w * 8], bitmap[w]);
  Header h = {info->block_size, info->granule,
              info->full ? kDeltaFlagFull : 0, info->volume_bytes,
              info->n_granules, {0}};
  put_u64(h.owned, info->n_marked);
  put_u32(h.owned + 8, crc32c_sw(0, raw.data(), raw.size()));
  int status = out->begin(kDelta, h, error);
  if (status != kIoOk) return status;
  if (out->write(raw.data(), raw.size())) {  // else end() reports it
    RecordWriter writer(out, info->granule, record_granules(info->granule),
                        info->n_marked);
    uint64_t packed = 0;
    status = bdev_pack_marked_sync(
        src, 0, info->volume_bytes, info->granule, bitmap, 0,
        [&writer](const uint8_t* data, uint64_t, uint64_t count) {
          return writer.add(data, count);
        },
        &packed);
    if (status != kIoOk || packed != info->n_marked || !writer.complete()) {
      return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed,
                  "reading the volume or writing " + out->tmp() + " failed");
    }
  }
  status = out->end(info->n_marked, error);
  info->file_bytes = out->bytes();
  return status;
}

// --- fingerprint maps --------------------------------------------------------

struct LoadedMap {
  FingerprintMapInfo info;
  std::vector<uint8_t> fps;  // n_granules * 16 bytes
};

// Structural pass, then every record with its CRC checked before its
// bytes are kept.
int load_map(const std::string& path, LoadedMap* out, std::string* error) {
  InFile in;
  int status = in.open(path, kMap, error);
  if (status != kIoOk) return status;
  const Header& h = in.header;
  FingerprintMapInfo& info = out->info;
  info.version = kFingerprintMapVersion;
  info.block_size = h.block_size;
  info.granule = h.granule;
  info.algorithm = h.word;
  info.volume_bytes = h.volume_bytes;
  info.n_granules = h.n_granules;
  info.file_bytes = in.file_bytes;
  if (info.algorithm != kFingerprintAlgorithm) {
    return fail(error, kIoInvalid, "unknown fingerprint algorithm");
  }
  if (std::any_of(h.owned, h.owned + sizeof(h.owned),
                  [](uint8_t b) { return b != 0; })) {
    return fail(error, kIoInvalid, "non-zero reserved field");
  }
  if (!geometry_ok(h.block_size, h.granule, h.volume_bytes, h.n_granules)) {
    return fail(error, kIoInvalid, "inconsistent geometry in header");
  }
  status = in.check_length(
      record_stream_bytes(info.n_granules, kFingerprintBytes,
                          kFingerprintMapRecord),
      error);
  if (status == kIoOk) status = in.check_trailer(info.n_granules, error);
  if (status != kIoOk) return status;
  out->fps.resize(info.n_granules * kFingerprintBytes);
  RecordReader reader(&in, kHeaderBytes, kFingerprintBytes,
                      kFingerprintMapRecord, info.n_granules);
  return reader.take(out->fps.data(), info.n_granules, error);
}

// The complete, synced map of a volume of `length` bytes whose
// fingerprints are `fps`. Fills *info.
int write_map(OutFile* out, uint64_t block_size, uint32_t granule,
              uint64_t length, const std::vector<uint8_t>& fps,
              FingerprintMapInfo* info, std::string* error) {
  info->version = kFingerprintMapVersion;
  info->block_size = static_cast<uint32_t>(block_size);
  info->granule = granule;
  info->algorithm = kFingerprintAlgorithm;
  info->volume_bytes = length;
  info->n_granules = fps.size() / kFingerprintBytes;
  const Header h = {info->block_size, granule, kFingerprintAlgorithm, length,
                    info->n_granules, {0}};
  int status = out->begin(kMap, h, error);
  if (status != kIoOk) return status;
  RecordWriter writer(out, kFingerprintBytes, kFingerprintMapRecord,
                      info->n_granules);
  writer.add(fps.data(), info->n_granules);  // a failure shows in end()
  status = out->end(info->n_granules, error);
  info->file_bytes = out->bytes();
  return status;
}

// One fingerprint pass over [0, length) of `bdev`. With `stored`, bit g
// of `bitmap` is set when granule g has no stored fingerprint or differs
// from it; with `keep`, the fingerprints are kept.
int fingerprint_pass(Bdev* bdev, uint64_t length, uint32_t granule,
                     const std::vector<uint8_t>* stored,
                     std::vector<uint64_t>* bitmap,
                     std::vector<uint8_t>* keep) {
  if (granule == 0 || length % granule != 0) return kIoInvalid;
  const uint64_t n_granules = length / granule;
  if (n_granules > kMaxGranules) return kIoInvalid;
  if (bitmap != nullptr) bitmap->assign((n_granules + 63) / 64, 0);
  if (keep != nullptr) keep->resize(n_granules * kFingerprintBytes);
  const uint64_t n_stored =
      stored != nullptr ? stored->size() / kFingerprintBytes : 0;
  uint64_t done = 0;
  const int status = bdev_fingerprint_sync(
      bdev, 0, length, granule, 0,
      [&](const uint8_t* fps, uint64_t first, uint64_t count) {
        if (keep != nullptr) {
          memcpy(&(*keep)[first * kFingerprintBytes], fps,
                 count * kFingerprintBytes);
        }
        if (bitmap != nullptr) {
          for (uint64_t i = 0; i < count; ++i) {
            const uint64_t g = first + i;
            if (g >= n_stored ||
                memcmp(fps + i * kFingerprintBytes,
                       &(*stored)[g * kFingerprintBytes],
                       kFingerprintBytes) != 0) {
              (*bitmap)[g / 64] |= 1ull << (g % 64);
            }
          }
        }
        return 0;
      },
      &done);
  if (status == kIoOk && done != n_granules) return kIoFailed;
  return status;
}

// --- export: which granules ---------------------------------------------------

struct Marked {
  std::vector<uint64_t> bitmap;
  uint64_t n_marked = 0;
  std::vector<uint8_t> fps;  // of src, where a pass kept them for map_out
};

// Against the fingerprint map `base_map`, whose granule the export takes.
int mark_against_map(Bdev* src, const std::string& base_map, bool keep_fps,
                     uint32_t* granule, Marked* out, std::string* error) {
  LoadedMap stored;
  int status = load_map(base_map, &stored, error);
  if (status != kIoOk) return status;
  if (*granule != 0 && *granule != stored.info.granule) {
    return fail(error, kIoInvalid,
                "granule differs from the base map's (" +
                    std::to_string(stored.info.granule) + ")");
  }
  *granule = stored.info.granule;
  if (stored.info.block_size != src->block_size() ||
      stored.info.volume_bytes > src->size_bytes()) {
    return fail(error, kIoInvalid,
                "base map has another block size or a larger volume");
  }
  status = fingerprint_pass(src, src->size_bytes(), *granule, &stored.fps,
                            &out->bitmap, keep_fps ? &out->fps : nullptr);
  if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
  if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
  out->n_marked = popcount(out->bitmap);
  return kIoOk;
}

// Against the clone `base`.
int mark_against_clone(Bdev* src, Bdev* base, uint32_t granule, Marked* out,
                       std::string* error) {
  if (base->block_size() != src->block_size() ||
      base->size_bytes() != src->size_bytes()) {
    return fail(error, kIoInvalid,
                "base and volume differ in block size or size");
  }
  DiffStats diff;
  const int status = bdev_diff_sync(base, 0, src, 0, src->size_bytes(),
                                    granule, 0, &out->bitmap, &diff);
  if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
  if (status != kIoOk) return fail(error, kIoFailed, "compare failed");
  out->n_marked = diff.mismatched;
  return kIoOk;
}

// Every granule: a full file.
int mark_all(Bdev* src, uint32_t granule, Marked* out, std::string* error) {
  const uint64_t n = src->size_bytes() / granule;
  if (!geometry_ok(src->block_size(), granule, src->size_bytes(), n)) {
    return fail(error, kIoInvalid, kBadGranule);
  }
  out->n_marked = n;
  out->bitmap.assign((n + 63) / 64, ~0ull);
  if (n % 64 != 0) out->bitmap.back() = (1ull << (n % 64)) - 1;
  return kIoOk;
}

}  // namespace

int bdev_export_delta(Bdev* src, Bdev* base, const std::string& path,
                      uint32_t granule, bool overwrite, DeltaInfo* stats,
                      std::string* error) {
  return bdev_export_delta(src, base, path, granule, overwrite, nullptr, stats,
                           error);
}

int bdev_export_delta(Bdev* src, Bdev* base, const std::string& path,
                      uint32_t granule, bool overwrite, DeltaMaps* maps,
                      DeltaInfo* stats, std::string* error) {
  if (src == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  const std::string base_map = maps != nullptr ? maps->base_map : "";
  const std::string map_out = maps != nullptr ? maps->map_out : "";
  if (maps != nullptr) maps->map_bytes = 0;
  if (base != nullptr && !base_map.empty()) {
    return fail(error, kIoInvalid, "base and base_map exclude each other");
  }
  if (map_out == path) {
    return fail(error, kIoInvalid, "map_out names the delta file");
  }
  if (src->block_size() > UINT32_MAX) {
    return fail(error, kIoInvalid, "block size too large");
  }
  if (granule == 0 && base_map.empty()) {
    granule = static_cast<uint32_t>(src->block_size());
  }
  Marked marked;
  int status;
  if (!base_map.empty()) {
    status = mark_against_map(src, base_map, !map_out.empty(), &granule,
                              &marked, error);
  } else if (base != nullptr) {
    status = mark_against_clone(src, base, granule, &marked, error);
  } else {
    status = mark_all(src, granule, &marked, error);
  }
  if (status != kIoOk) return status;
  DeltaInfo info;
  info.version = kDeltaVersion;
  info.block_size = static_cast<uint32_t>(src->block_size());
  info.granule = granule;
  info.full = base == nullptr && base_map.empty();
  info.volume_bytes = src->size_bytes();
  info.n_granules = info.volume_bytes / granule;
  info.n_marked = marked.n_marked;

  status = refuse_existing(path, overwrite, error);
  if (status == kIoOk && !map_out.empty()) {
    status = refuse_existing(map_out, overwrite, error);
  }
  if (status != kIoOk) return status;
  // The map is taken before the pack pass: a write in between leaves it
  // older than the exported data, never newer.
  if (!map_out.empty() && base_map.empty() &&
      fingerprint_pass(src, info.volume_bytes, granule, nullptr, nullptr,
                       &marked.fps) != kIoOk) {
    return fail(error, kIoFailed, "fingerprint pass failed");
  }
  // Both files are complete under their .tmp names before either
  // appears, and the map follows the delta it belongs to. What was
  // written and not published goes away with its OutFile.
  OutFile delta(path);
  OutFile map(map_out);
  FingerprintMapInfo map_info;
  status = write_delta(&delta, src, marked.bitmap, &info, error);
  if (status == kIoOk && !map_out.empty()) {
    status = write_map(&map, src->block_size(), granule, info.volume_bytes,
                       marked.fps, &map_info, error);
  }
  if (status == kIoOk) status = delta.publish(error);
  if (status != kIoOk) return status;
  std::string why;
  if (!map_out.empty() && map.publish(&why) != kIoOk) {
    return fail(error, kIoFailed, why + " (" + path + " was written)");
  }
  if (maps != nullptr) maps->map_bytes = map_info.file_bytes;
  if (stats != nullptr) *stats = info;
  return kIoOk;
}

int delta_file_info(const std::string& path, DeltaInfo* info,
                    std::string* error) {
  ParsedDelta file;
  const int status = parse_delta(path, &file, error);
  if (status == kIoOk && info != nullptr) *info = file.info;
  return status;
}

int bdev_import_delta(Bdev* dst, const std::string& path, bool dry_run,
                      DeltaInfo* stats, std::string* error) {
  if (dst == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  ParsedDelta file;
  int status = parse_delta(path, &file, error);
  if (status != kIoOk) return status;
  const DeltaInfo& info = file.info;
  if (info.block_size != dst->block_size()) {
    return fail(error, kIoInvalid,
                "file block size " + std::to_string(info.block_size) +
                    " differs from the target's");
  }
  if (info.volume_bytes > dst->size_bytes()) {
    return fail(error, kIoInvalid, "file volume is larger than the target");
  }
  if (!dry_run && dst->claimed()) {
    return fail(error, kIoFailed,
                "bdev " + dst->name() +
                    " is claimed; import runs offline only");
  }
  RecordReader reader(&file.in, file.records_offset, info.granule,
                      record_granules(info.granule), info.n_marked);
  std::string why;
  if (dry_run) {
    status = reader.take(nullptr, info.n_marked, &why);
    if (status != kIoOk) return fail(error, status, why);
  } else if (info.n_marked > 0) {
    uint64_t applied = 0;
    status = bdev_unpack_marked_sync(
        dst, 0, info.volume_bytes, info.granule, file.bitmap, 0,
        [&reader, &why](uint8_t* data, uint64_t, uint64_t count) {
          return reader.take(data, count, &why);
        },
        &applied);
    if (status != kIoOk) {
      if (why.empty()) why = "writing the target failed";
      return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed,
                  why + "; " + std::to_string(applied) + " of " +
                      std::to_string(info.n_marked) +
                      " granules were applied, the target may be partly "
                      "updated");
    }
  }
  if (reader.left() != 0) {
    return fail(error, kIoInvalid, "records left over after the last granule");
  }
  if (stats != nullptr) *stats = info;
  return kIoOk;
}

int bdev_fingerprint_file(Bdev* bdev, const std::string& path,
                          uint32_t granule, bool overwrite,
                          FingerprintMapInfo* stats, std::string* error) {
  if (bdev == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  if (bdev->block_size() > UINT32_MAX) {
    return fail(error, kIoInvalid, "block size too large");
  }
  if (granule == 0) granule = static_cast<uint32_t>(bdev->block_size());
  int status = refuse_existing(path, overwrite, error);
  if (status != kIoOk) return status;
  std::vector<uint8_t> fps;
  status = fingerprint_pass(bdev, bdev->size_bytes(), granule, nullptr,
                            nullptr, &fps);
  if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
  if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
  OutFile out(path);
  FingerprintMapInfo info;
  status = write_map(&out, bdev->block_size(), granule, bdev->size_bytes(),
                     fps, &info, error);
  if (status == kIoOk) status = out.publish(error);
  if (status == kIoOk && stats != nullptr) *stats = info;
  return status;
}

int fingerprint_map_info(const std::string& path, FingerprintMapInfo* info,
                         std::string* error) {
  LoadedMap map;
  const int status = load_map(path, &map, error);
  if (status == kIoOk && info != nullptr) *info = map.info;
  return status;
}

int bdev_verify_fingerprints(Bdev* bdev, const std::string& path,
                             uint32_t max_report, FingerprintVerify* stats,
                             std::string* error) {
  if (bdev == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  LoadedMap map;
  int status = load_map(path, &map, error);
  if (status != kIoOk) return status;
  if (map.info.block_size != bdev->block_size()) {
    return fail(error, kIoInvalid,
                "map block size " + std::to_string(map.info.block_size) +
                    " differs from the volume's");
  }
  if (map.info.volume_bytes > bdev->size_bytes()) {
    return fail(error, kIoInvalid, "map volume is larger than the bdev");
  }
  std::vector<uint64_t> bitmap;
  status = fingerprint_pass(bdev, map.info.volume_bytes, map.info.granule,
                            &map.fps, &bitmap, nullptr);
  if (status != kIoOk) {
    return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed,
                "fingerprint pass failed");
  }
  if (stats != nullptr) {
    stats->granule = map.info.granule;
    stats->granules = map.info.n_granules;
    stats->mismatched = popcount(bitmap);
    stats->first_mismatches = first_set_bits(bitmap, max_report);
  }
  return kIoOk;
}

}  // namespace hipstore
