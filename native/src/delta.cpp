// hipstore delta files: export / import of marked granules, and
// fingerprint maps (delta.h). Both formats sit on checked_file.h; here
// is what each format owns, and the passes over the volume.

#include "hipstore/delta.h"

#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <memory>
#include <vector>

#include "checked_file.h"
#include "hipstore/compress.h"
#include "hipstore/crypt.h"
#include "hipstore/engine.h"
#include "hipstore/fingerprint.h"

namespace hipstore {

using namespace checked_file;

namespace {

static_assert(kDeltaHeaderBytes == kHeaderBytes &&
                  kDeltaTrailerBytes == kTrailerBytes,
              "delta.h documents the core's header and trailer");

// The versions of a format differ in the version alone. The magics are
// eight bytes; a shorter literal is padded with NULs.
Format make_format(const char* magic, const char* end_magic, uint32_t version,
                   const char* noun) {
  Format f = {{0}, {0}, version, noun};
  strncpy(f.magic, magic, sizeof(f.magic));
  strncpy(f.end_magic, end_magic, sizeof(f.end_magic));
  return f;
}

Format delta_format(uint32_t version) {
  return make_format("HSDELTA1", "HSDEND1", version, "delta file");
}

Format map_format(uint32_t version) {
  return make_format("HSFPMAP1", "HSFPEND1", version, "fingerprint map");
}

// Indexed by version - 1.
const Format kDeltaFormats[] = {
    delta_format(kDeltaVersion), delta_format(kDeltaVersionLz),
    delta_format(kDeltaVersionXts), delta_format(kDeltaVersionDict),
    delta_format(kDeltaVersionCts)};
const Format kMap = map_format(kFingerprintMapVersion);
const Format kMapBlake2s2 = map_format(kFingerprintMapVersionBlake2s);

// The version of a file with these properties. A dictionary needs
// compression; compressed and encrypted is version 5 with or without one.
uint32_t delta_version(bool compressed, bool dictionary, bool encrypted) {
  if (compressed && encrypted) return kDeltaVersionCts;
  if (dictionary) return kDeltaVersionDict;
  if (compressed) return kDeltaVersionLz;
  return encrypted ? kDeltaVersionXts : kDeltaVersion;
}

// Header bytes 20-23 of such a file.
uint32_t delta_flags(const DeltaInfo& info) {
  return (info.full ? kDeltaFlagFull : 0) |
         (info.compressed ? kDeltaFlagLz : 0) |
         (info.dictionary ? kDeltaFlagDict : 0) |
         (info.encrypted ? kDeltaFlagXts : 0);
}

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
  uint64_t record_area = 0;  // compressed files
  uint32_t kcv = 0;          // encrypted files
};

// The key block of a version-5 file, directly after the bitmap: "HSKC",
// u32 xts_kcv(key), u32 0, u32 crc32c of those 12 bytes.
constexpr uint64_t kKeyBlockBytes = 16;
const char kKeyBlockMagic[4] = {'H', 'S', 'K', 'C'};

void put_key_block(uint8_t* block, uint32_t kcv) {
  memcpy(block, kKeyBlockMagic, 4);
  put_u32(block + 4, kcv);
  put_u32(block + 8, 0);
  put_u32(block + 12, crc32c_sw(0, block, 12));
}

// The structural pass: everything that can be checked without reading
// a record payload.
int parse_delta(const std::string& path, ParsedDelta* out,
                std::string* error) {
  InFile& in = out->in;
  int status =
      in.open(path, kDeltaFormats[0], error,
              {&kDeltaFormats[1], &kDeltaFormats[2], &kDeltaFormats[3],
               &kDeltaFormats[4]});
  if (status != kIoOk) return status;
  const Header& h = in.header;
  DeltaInfo& info = out->info;
  info.version = in.format().version;
  // Version 5 is compressed and encrypted, with or without dictionaries:
  // there the flag decides, everywhere else the version does.
  const bool cts = info.version == kDeltaVersionCts;
  info.dictionary = cts ? (h.word & kDeltaFlagDict) != 0
                        : info.version == kDeltaVersionDict;
  info.compressed = info.version == kDeltaVersionLz || info.dictionary || cts;
  info.encrypted = info.version == kDeltaVersionXts || cts;
  info.block_size = h.block_size;
  info.granule = h.granule;
  info.full = (h.word & kDeltaFlagFull) != 0;
  info.volume_bytes = h.volume_bytes;
  info.n_granules = h.n_granules;
  info.n_marked = get_u64(h.owned);
  info.file_bytes = in.file_bytes;
  // The flag word is exactly what the version stands for: no unknown bit,
  // and each known one as the version says. The spare words: version 1
  // none, versions 2, 4 and 5 both, version 3 the first.
  if (h.word != delta_flags(info) ||
      (!info.compressed && get_u32(h.owned + 16) != 0) ||
      (!info.compressed && !info.encrypted && get_u32(h.owned + 12) != 0)) {
    return fail(error, kIoInvalid, "unknown flags or non-zero reserved field");
  }
  if (info.encrypted) {
    if (!xts_granule_ok(info.granule)) {
      return fail(error, kIoInvalid, "granule outside the encrypted range");
    }
    if (!cts) out->kcv = get_u32(h.owned + 12);
  }
  if (!geometry_ok(h.block_size, h.granule, h.volume_bytes, h.n_granules) ||
      info.n_marked > info.n_granules ||
      (info.full && info.n_marked != info.n_granules)) {
    return fail(error, kIoInvalid, "inconsistent geometry in header");
  }
  const uint64_t n_words = (info.n_granules + 63) / 64;
  uint64_t records = record_stream_bytes(info.n_marked, info.granule,
                                         record_granules(info.granule));
  info.stored_bytes = info.n_marked * info.granule;
  if (info.compressed) {
    if (!lz_granule_ok(info.granule)) {
      return fail(error, kIoInvalid, "granule outside the compressed range");
    }
    // Record heads and sizes, then 1 .. granule bytes per piece: with
    // that, neither the length below nor stored_bytes wraps.
    const uint64_t fixed =
        (records - info.stored_bytes) * 2 + info.n_marked * 4;
    out->record_area = get_u64(h.owned + 12);
    if (out->record_area < fixed + info.n_marked * (cts ? 16 : 1) ||
        out->record_area > fixed + info.stored_bytes) {
      return fail(error, kIoInvalid, "record_area_bytes out of range");
    }
    info.stored_bytes = out->record_area - fixed;
    records = out->record_area;
  }
  const uint64_t key_block = cts ? kKeyBlockBytes : 0;
  status = in.check_length(n_words * 8 + key_block + records, error);
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
  out->records_offset = kHeaderBytes + raw.size() + key_block;
  if (cts) {
    uint8_t block[kKeyBlockBytes];
    if (!in.read(block, sizeof(block), kHeaderBytes + raw.size())) {
      return fail(error, kIoFailed, "cannot read key block");
    }
    if (memcmp(block, kKeyBlockMagic, 4) != 0 || get_u32(block + 8) != 0 ||
        crc32c_sw(0, block, 12) != get_u32(block + 12)) {
      return fail(error, kIoInvalid, "bad key block");
    }
    out->kcv = get_u32(block + 4);
  }
  return in.check_trailer(info.n_marked, error);
}

// The marked calls' key argument for a file's records: unit 0 is granule
// 0 of the volume. No key for a file that is not encrypted.
XtsKey record_key(const DeltaInfo& info, const std::vector<uint8_t>* key) {
  if (!info.encrypted) return {};
  return {key->data(), key->size(), 0};
}

// Header, bitmap, the marked granules of `src` as records, trailer, all
// synced. Fills info->file_bytes and info->stored_bytes. The records are
// fixed (versions 1 and 3: bdev_pack_marked_sync, or with `key`, which
// info->encrypted goes with, what bdev_xts_pack_marked_sync delivers, and
// the key check value in the header) or variable (info->compressed,
// versions 2, 4 and 5: bdev_compress_marked_sync, with info->dictionary
// against `base`, and record_area_bytes put into the header once the
// records are out). A compressed file with `key` is version 5: the key
// block follows the bitmap and the records hold what the keyed calls
// deliver, every piece in max(size, 16) bytes.
int write_delta(OutFile* out, Bdev* src, Bdev* base,
                const std::vector<uint64_t>& bitmap,
                const std::vector<uint8_t>* key, DeltaInfo* info,
                std::string* error) {
  const bool key_block = info->compressed && info->encrypted;
  std::vector<uint8_t> raw(bitmap.size() * 8);
  for (size_t w = 0; w < bitmap.size(); ++w) put_u64(&raw[w * 8], bitmap[w]);
  Header h = {info->block_size, info->granule, delta_flags(*info),
              info->volume_bytes, info->n_granules, {0}};
  put_u64(h.owned, info->n_marked);
  put_u32(h.owned + 8, crc32c_sw(0, raw.data(), raw.size()));
  uint8_t block[kKeyBlockBytes];
  if (key_block) {
    put_key_block(block, xts_kcv(key->data()));
  } else if (info->encrypted) {
    put_u32(h.owned + 12, xts_kcv(key->data()));
  }
  int status = out->begin(kDeltaFormats[info->version - 1], h, error);
  if (status != kIoOk) return status;
  info->stored_bytes = info->n_marked * info->granule;
  if (out->write(raw.data(), raw.size()) &&  // else end() reports it
      (!key_block || out->write(block, sizeof(block)))) {
    const XtsKey xts = record_key(*info, key);
    uint64_t packed = 0;
    bool complete = false;
    std::string why;
    if (info->compressed) {
      const uint32_t min_piece = info->encrypted ? 16 : 1;
      VarRecordWriter writer(out, info->granule,
                             record_granules(info->granule), info->n_marked,
                             min_piece);
      LzOptions options;
      options.key = xts;
      if (info->dictionary) options.base = base;
      status = bdev_compress_marked_sync(
          src, 0, info->volume_bytes, info->granule, bitmap, options,
          [&writer, min_piece](const uint8_t* data, const uint32_t* sizes,
                               uint64_t, uint64_t count) {
            int added = kIoOk;
            for (uint64_t i = 0; i < count && added == kIoOk; ++i) {
              added = writer.add(data, sizes[i]);
              data += lz_padded(std::max(sizes[i], min_piece));
            }
            return added;
          },
          &packed, &why);
      complete = writer.complete();
      put_u64(h.owned + 12, writer.area());
      info->stored_bytes = writer.unit_bytes();
    } else {
      RecordWriter writer(out, info->granule, record_granules(info->granule),
                          info->n_marked);
      const PackSink sink = [&writer](const uint8_t* data, uint64_t,
                                      uint64_t count) {
        return writer.add(data, count);
      };
      status = info->encrypted
                   ? bdev_xts_pack_marked_sync(src, 0, info->volume_bytes,
                                               info->granule, bitmap, xts, 0,
                                               sink, &packed)
                   : bdev_pack_marked_sync(src, 0, info->volume_bytes,
                                           info->granule, bitmap, 0, sink,
                                           &packed);
      complete = writer.complete();
    }
    if (status != kIoOk || packed != info->n_marked || !complete) {
      if (why.empty()) {
        why = "reading the volume or writing " + out->tmp() + " failed";
      }
      return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed, why);
    }
    if (info->compressed) out->rewrite_header(h);
  }
  status = out->end(info->n_marked, error);
  info->file_bytes = out->bytes();
  return status;
}

// --- fingerprint maps --------------------------------------------------------

struct LoadedMap {
  FingerprintMapInfo info;
  std::vector<uint8_t> fps;  // n_granules * 16 bytes
  uint32_t kcv = 0;          // algorithm 3
};

// The fingerprint of a call's maps, settled: the kind points into the
// caller's key.
struct MapChoice {
  FingerprintKind kind;
  uint32_t kcv = 0;
};

// For a map that the call writes from nothing.
int choose_new(const MapKind& want, MapChoice* out, std::string* error) {
  if (want.algorithm > kMapBlake2s) {
    return fail(error, kIoInvalid, "unknown map_algorithm");
  }
  if (want.key != nullptr && want.algorithm != kMapBlake2s) {
    return fail(error, kIoInvalid, "map_key needs map_algorithm blake2s");
  }
  if (want.key != nullptr && want.key->size() != kBlake2sKeyBytes) {
    return fail(error, kIoInvalid, "the map key must be 32 bytes");
  }
  *out = MapChoice();
  if (want.algorithm == kMapBlake2s) {
    out->kind.algorithm = kFingerprintBlake2s;
    if (want.key != nullptr) {
      out->kind = {kFingerprintBlake2sKeyed, want.key->data(),
                   want.key->size()};
      out->kcv = blake2s_kcv(want.key->data());
    }
  }
  return kIoOk;
}

// For a pass against the map `stored`, which decides the algorithm.
int choose_stored(const MapKind& want, const LoadedMap& stored,
                  MapChoice* out, std::string* error) {
  const uint32_t family =
      stored.info.algorithm == kFingerprintAlgorithm ? kMapHsfp1 : kMapBlake2s;
  if (want.algorithm != 0 && want.algorithm != family) {
    return fail(error, kIoInvalid, "map_algorithm differs from the map's");
  }
  if (want.key != nullptr && !stored.info.keyed) {
    return fail(error, kIoInvalid, "a map key was given for an unkeyed map");
  }
  if (want.key == nullptr && stored.info.keyed) {
    return fail(error, kIoInvalid, "the map is keyed: a map key is required");
  }
  MapKind same = want;
  same.algorithm = family;
  const int status = choose_new(same, out, error);
  if (status != kIoOk) return status;
  if (stored.info.keyed && out->kcv != stored.kcv) {
    return fail(error, kIoInvalid,
                "wrong map key (key check value differs from the map's)");
  }
  return kIoOk;
}

// Structural pass, then every record with its CRC checked before its
// bytes are kept.
int load_map(const std::string& path, LoadedMap* out, std::string* error) {
  InFile in;
  int status = in.open(path, kMap, error, {&kMapBlake2s2});
  if (status != kIoOk) return status;
  const Header& h = in.header;
  FingerprintMapInfo& info = out->info;
  info.version = in.format().version;
  info.block_size = h.block_size;
  info.granule = h.granule;
  info.algorithm = h.word;
  info.volume_bytes = h.volume_bytes;
  info.n_granules = h.n_granules;
  info.file_bytes = in.file_bytes;
  // Version 1 holds algorithm 1, version 2 algorithm 2 or 3.
  const bool blake = info.algorithm == kFingerprintBlake2s ||
                     info.algorithm == kFingerprintBlake2sKeyed;
  if (info.version == kFingerprintMapVersion
          ? info.algorithm != kFingerprintAlgorithm
          : !blake) {
    return fail(error, kIoInvalid, "unknown fingerprint algorithm");
  }
  info.keyed = info.algorithm == kFingerprintBlake2sKeyed;
  if (info.keyed) out->kcv = get_u32(h.owned);
  if (std::any_of(h.owned + (info.keyed ? 4 : 0), h.owned + sizeof(h.owned),
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
              const MapChoice& choice, FingerprintMapInfo* info,
              std::string* error) {
  const bool blake = choice.kind.algorithm != kFingerprintAlgorithm;
  info->version =
      blake ? kFingerprintMapVersionBlake2s : kFingerprintMapVersion;
  info->block_size = static_cast<uint32_t>(block_size);
  info->granule = granule;
  info->algorithm = choice.kind.algorithm;
  info->keyed = choice.kind.algorithm == kFingerprintBlake2sKeyed;
  info->volume_bytes = length;
  info->n_granules = fps.size() / kFingerprintBytes;
  Header h = {info->block_size, granule, info->algorithm, length,
              info->n_granules, {0}};
  if (info->keyed) put_u32(h.owned, choice.kcv);
  int status = out->begin(blake ? kMapBlake2s2 : kMap, h, error);
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
                     const FingerprintKind& kind,
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
      &done, kind);
  if (status == kIoOk && done != n_granules) return kIoFailed;
  return status;
}

// --- export: which granules ---------------------------------------------------

struct Marked {
  std::vector<uint64_t> bitmap;
  uint64_t n_marked = 0;
  std::vector<uint8_t> fps;  // of src, where a pass kept them for map_out
};

// Against the fingerprint map `base_map`, whose granule and algorithm the
// export takes.
int mark_against_map(Bdev* src, const std::string& base_map,
                     const MapKind& want, bool keep_fps, uint32_t* granule,
                     MapChoice* choice, Marked* out, std::string* error) {
  LoadedMap stored;
  int status = load_map(base_map, &stored, error);
  if (status == kIoOk) status = choose_stored(want, stored, choice, error);
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
  status = fingerprint_pass(src, src->size_bytes(), *granule, choice->kind,
                            &stored.fps, &out->bitmap,
                            keep_fps ? &out->fps : nullptr);
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

// The dry run over the variable records of a compressed file: every
// piece is validated here. A version-5 file's pieces are ciphertext in
// max(size, 16) bytes each: without the key only records and sizes are
// checked, with it every piece is decrypted and validated.
int check_pieces(const ParsedDelta& file, VarRecordReader* reader,
                 const std::vector<uint8_t>* key, std::string* why) {
  const DeltaInfo& info = file.info;
  std::unique_ptr<XtsSchedules> keys;
  if (info.encrypted && key != nullptr) {
    keys.reset(new XtsSchedules(key->data()));
  }
  std::vector<uint8_t> plain(info.granule);
  const uint8_t* piece = nullptr;
  uint32_t size = 0;
  int status = kIoOk;
  for (uint64_t w = 0; w < file.bitmap.size() && status == kIoOk; ++w) {
    for (uint64_t word = file.bitmap[w]; word != 0 && status == kIoOk;
         word &= word - 1) {
      const uint64_t g = w * 64 + static_cast<uint64_t>(__builtin_ctzll(word));
      status = reader->next(&piece, &size, why);
      if (info.encrypted) {
        if (keys == nullptr) continue;  // structure and CRCs only
        if (status != kIoOk) break;
        xts_decrypt_var(*keys, g, piece, plain.data(), std::max(size, 16u));
        piece = plain.data();
      }
      std::string rule;
      if (status == kIoOk &&
          !(info.dictionary
                ? lz_dict_validate_granule(piece, size, info.granule, &rule)
                : lz_validate_granule(piece, size, info.granule, &rule))) {
        status = kIoInvalid;
        *why = "granule " + std::to_string(g) + ": bad compressed piece (" +
               rule + ")";
      }
    }
  }
  return status;
}

// The record pass of an import. dry_run checks every record and writes
// nothing: the fixed records by their CRCs, the variable ones in
// check_pieces. Otherwise the marked calls apply them: fixed records
// through bdev_unpack_marked_sync or, encrypted, bdev_xts_unpack_marked_sync;
// compressed pieces through bdev_decompress_marked_sync, which validates
// each before it decodes (a version-4 file's dictionaries are the target's
// granules; a version-5 file's pieces are validated on the GPU while
// decoding, or on the host).
int import_records(Bdev* dst, ParsedDelta* file, bool dry_run,
                   const std::vector<uint8_t>* key, std::string* error) {
  const DeltaInfo& info = file->info;
  const bool apply = !dry_run && info.n_marked > 0;
  std::string why;
  uint64_t applied = 0;
  uint64_t left = 0;
  int status = kIoOk;
  if (info.compressed) {
    const uint32_t min_piece = info.encrypted ? 16 : 1;
    VarRecordReader reader(&file->in, file->records_offset, file->record_area,
                           info.granule, record_granules(info.granule),
                           info.n_marked, min_piece);
    if (dry_run) {
      status = check_pieces(*file, &reader, key, &why);
    } else if (apply) {
      const DecompressSource source = [&](uint8_t* data, uint32_t* sizes,
                                          uint64_t, uint64_t count) {
        const uint8_t* piece = nullptr;
        for (uint64_t i = 0; i < count; ++i) {
          const int got = reader.next(&piece, &sizes[i], &why);
          if (got != kIoOk) return got;
          const uint32_t stored = std::max(sizes[i], min_piece);
          memcpy(data, piece, stored);
          memset(data + stored, 0, lz_padded(stored) - stored);
          data += lz_padded(stored);
        }
        return static_cast<int>(kIoOk);
      };
      LzOptions options;
      options.key = record_key(info, key);
      options.dictionary = info.dictionary;
      status = bdev_decompress_marked_sync(dst, 0, info.volume_bytes,
                                           info.granule, file->bitmap, options,
                                           source, &applied, &why);
    }
    left = reader.left();
  } else {
    RecordReader reader(&file->in, file->records_offset, info.granule,
                        record_granules(info.granule), info.n_marked);
    if (dry_run) {
      status = reader.take(nullptr, info.n_marked, &why);
    } else if (apply) {
      const UnpackSource source = [&reader, &why](uint8_t* data, uint64_t,
                                                  uint64_t count) {
        return reader.take(data, count, &why);
      };
      status = info.encrypted
                   ? bdev_xts_unpack_marked_sync(dst, 0, info.volume_bytes,
                                                 info.granule, file->bitmap,
                                                 record_key(info, key), 0,
                                                 source, &applied)
                   : bdev_unpack_marked_sync(dst, 0, info.volume_bytes,
                                             info.granule, file->bitmap, 0,
                                             source, &applied);
    }
    left = reader.left();
  }
  if (status != kIoOk && dry_run) return fail(error, status, why);
  if (status != kIoOk) {
    if (why.empty()) why = "writing the target failed";
    return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed,
                why + "; " + std::to_string(applied) + " of " +
                    std::to_string(info.n_marked) +
                    " granules were applied, the target may be partly "
                    "updated");
  }
  if (left != 0) {
    return fail(error, kIoInvalid, "records left over after the last granule");
  }
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
                      DeltaInfo* stats, std::string* error, bool compress,
                      const std::vector<uint8_t>* key, bool dictionary,
                      bool cts) {
  if (src == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  if (cts && (key == nullptr || !compress)) {
    return fail(error, kIoInvalid, "cts needs key and compress");
  }
  if (dictionary &&
      (!compress || base == nullptr || (key != nullptr && !cts))) {
    return fail(error, kIoInvalid,
                "dictionary needs compress and base (a clone), and no key");
  }
  if (key != nullptr && !xts_key_ok(key->data(), key->size())) {
    return fail(error, kIoInvalid,
                "the key must be 64 bytes whose halves differ");
  }
  if (key != nullptr && compress && !cts) {
    return fail(error, kIoInvalid, "key and compress exclude each other");
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
  const MapKind want = maps != nullptr ? maps->kind : MapKind();
  MapChoice choice;
  if (base_map.empty()) {
    if (map_out.empty() && (want.algorithm != 0 || want.key != nullptr)) {
      return fail(error, kIoInvalid,
                  "map_algorithm and map_key need base_map or map_out");
    }
    const int chosen = choose_new(want, &choice, error);
    if (chosen != kIoOk) return chosen;
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
    status = mark_against_map(src, base_map, want, !map_out.empty(), &granule,
                              &choice, &marked, error);
  } else if (base != nullptr) {
    status = mark_against_clone(src, base, granule, &marked, error);
  } else {
    status = mark_all(src, granule, &marked, error);
  }
  if (status != kIoOk) return status;
  if (compress && !lz_granule_ok(granule)) {
    return fail(error, kIoInvalid,
                "compress needs 512 <= granule <= 16384 (granule " +
                    std::to_string(granule) + ")");
  }
  if (key != nullptr && !xts_granule_ok(granule)) {
    return fail(error, kIoInvalid, "a key needs granule <= 16777216");
  }
  DeltaInfo info;
  info.version = delta_version(compress, dictionary, key != nullptr);
  info.compressed = compress;
  info.dictionary = dictionary;
  info.encrypted = key != nullptr;
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
      fingerprint_pass(src, info.volume_bytes, granule, choice.kind, nullptr,
                       nullptr, &marked.fps) != kIoOk) {
    return fail(error, kIoFailed, "fingerprint pass failed");
  }
  // Both files are complete under their .tmp names before either
  // appears, and the map follows the delta it belongs to. What was
  // written and not published goes away with its OutFile.
  OutFile delta(path);
  OutFile map(map_out);
  FingerprintMapInfo map_info;
  status = write_delta(&delta, src, base, marked.bitmap, key, &info, error);
  if (status == kIoOk && !map_out.empty()) {
    status = write_map(&map, src->block_size(), granule, info.volume_bytes,
                       marked.fps, choice, &map_info, error);
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
                      DeltaInfo* stats, std::string* error,
                      const std::vector<uint8_t>* key) {
  if (dst == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  if (key != nullptr && !xts_key_ok(key->data(), key->size())) {
    return fail(error, kIoInvalid,
                "the key must be 64 bytes whose halves differ");
  }
  ParsedDelta file;
  int status = parse_delta(path, &file, error);
  if (status != kIoOk) return status;
  const DeltaInfo& info = file.info;
  if (key != nullptr && !info.encrypted) {
    return fail(error, kIoInvalid, "a key was given for an unencrypted file");
  }
  if (info.encrypted && key == nullptr && !dry_run) {
    return fail(error, kIoInvalid, "the file is encrypted: a key is required");
  }
  if (key != nullptr && xts_kcv(key->data()) != file.kcv) {
    return fail(error, kIoInvalid,
                "wrong key (key check value differs from the file's)");
  }
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
  status = import_records(dst, &file, dry_run, key, error);
  if (status == kIoOk && stats != nullptr) *stats = info;
  return status;
}

int bdev_fingerprint_file(Bdev* bdev, const std::string& path,
                          uint32_t granule, bool overwrite,
                          FingerprintMapInfo* stats, std::string* error,
                          const MapKind& kind) {
  if (bdev == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  if (bdev->block_size() > UINT32_MAX) {
    return fail(error, kIoInvalid, "block size too large");
  }
  if (granule == 0) granule = static_cast<uint32_t>(bdev->block_size());
  MapChoice choice;
  int status = choose_new(kind, &choice, error);
  if (status == kIoOk) status = refuse_existing(path, overwrite, error);
  if (status != kIoOk) return status;
  std::vector<uint8_t> fps;
  status = fingerprint_pass(bdev, bdev->size_bytes(), granule, choice.kind,
                            nullptr, nullptr, &fps);
  if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
  if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
  OutFile out(path);
  FingerprintMapInfo info;
  status = write_map(&out, bdev->block_size(), granule, bdev->size_bytes(),
                     fps, choice, &info, error);
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
                             std::string* error, const MapKind& kind) {
  if (bdev == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  LoadedMap map;
  MapChoice choice;
  int status = load_map(path, &map, error);
  if (status == kIoOk) status = choose_stored(kind, map, &choice, error);
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
                            choice.kind, &map.fps, &bitmap, nullptr);
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
