// hipstore delta files: export / import of marked granules, and
// fingerprint maps (delta.h).

#include "hipstore/delta.h"

#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <vector>

#include "hipstore/crc32c.h"
#include "hipstore/engine.h"
#include "hipstore/fingerprint.h"

namespace hipstore {

namespace {

const char kMagic[8] = {'H', 'S', 'D', 'E', 'L', 'T', 'A', '1'};
const char kEndMagic[8] = {'H', 'S', 'D', 'E', 'N', 'D', '1', '\0'};
// Same bound as the granule calls: 256 MiB of bitmap.
constexpr uint64_t kMaxGranules = 1ull << 31;

void put_u32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}
void put_u64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}
uint32_t get_u32(const uint8_t* p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) v |= static_cast<uint32_t>(p[i]) << (8 * i);
  return v;
}
uint64_t get_u64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  return v;
}

int fail(std::string* error, int status, const std::string& what) {
  if (error != nullptr) *error = what;
  return status;
}

std::string errno_text(const std::string& what) {
  return what + ": " + strerror(errno);
}

struct Fd {
  int fd = -1;
  ~Fd() {
    if (fd >= 0) close(fd);
  }
};

bool write_all(int fd, const void* data, size_t len) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  while (len > 0) {
    const ssize_t n = write(fd, p, len);
    if (n < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    p += n;
    len -= static_cast<size_t>(n);
  }
  return true;
}

// Reads exactly `len` bytes at `offset`; false on error or a short file.
bool read_all(int fd, void* data, size_t len, uint64_t offset) {
  uint8_t* p = static_cast<uint8_t*>(data);
  while (len > 0) {
    const ssize_t n = pread(fd, p, len, static_cast<off_t>(offset));
    if (n < 0) {
      if (errno == EINTR) continue;
      return false;
    }
    if (n == 0) return false;
    p += n;
    len -= static_cast<size_t>(n);
    offset += static_cast<uint64_t>(n);
  }
  return true;
}

uint64_t record_granules(uint32_t granule) {
  return std::max<uint64_t>(1, kDeltaRecordBytes / granule);
}

std::vector<uint8_t> bitmap_bytes(const std::vector<uint64_t>& words) {
  std::vector<uint8_t> raw(words.size() * 8);
  for (size_t w = 0; w < words.size(); ++w) put_u64(&raw[w * 8], words[w]);
  return raw;
}

// Cuts the dense stream into the format's records, whatever chunks the
// sink receives.
class RecordWriter {
 public:
  RecordWriter(int fd, uint32_t granule, uint64_t n_marked)
      : fd_(fd), granule_(granule), left_(n_marked),
        per_record_(record_granules(granule)) {
    buf_.resize(8 + std::min(per_record_, std::max<uint64_t>(n_marked, 1)) *
                        granule);
  }

  int add(const uint8_t* data, uint64_t count) {
    while (count > 0) {
      const uint64_t want = std::min(per_record_, left_);
      if (want == 0) return kIoFailed;  // more granules than announced
      const uint64_t take = std::min(count, want - have_);
      memcpy(&buf_[8 + have_ * granule_], data, take * granule_);
      have_ += take;
      data += take * granule_;
      count -= take;
      if (have_ == want) {
        const uint64_t payload = have_ * granule_;
        put_u32(&buf_[0], static_cast<uint32_t>(have_));
        put_u32(&buf_[4], crc32c_sw(0, &buf_[8], payload));
        if (!write_all(fd_, buf_.data(), 8 + payload)) return kIoFailed;
        bytes_ += 8 + payload;
        left_ -= have_;
        have_ = 0;
      }
    }
    return kIoOk;
  }

  bool complete() const { return left_ == 0 && have_ == 0; }
  uint64_t bytes() const { return bytes_; }

 private:
  int fd_;
  uint32_t granule_;
  uint64_t left_;  // granules not yet written
  uint64_t per_record_;
  uint64_t have_ = 0;  // granules in buf_
  uint64_t bytes_ = 0;
  std::vector<uint8_t> buf_;
};

struct ParsedFile {
  DeltaInfo info;
  std::vector<uint64_t> bitmap;
  uint64_t records_offset = 0;
};

// The structural pass: everything that can be checked without reading
// a record payload.
int parse_file(int fd, ParsedFile* out, std::string* error) {
  struct stat st;
  if (fstat(fd, &st) != 0) return fail(error, kIoFailed, errno_text("fstat"));
  if (!S_ISREG(st.st_mode)) {
    return fail(error, kIoInvalid, "not a regular file");
  }
  const uint64_t file_bytes = static_cast<uint64_t>(st.st_size);
  uint8_t h[kDeltaHeaderBytes];
  if (file_bytes < kDeltaHeaderBytes + kDeltaTrailerBytes ||
      !read_all(fd, h, sizeof(h), 0)) {
    return fail(error, kIoInvalid, "file shorter than header and trailer");
  }
  if (memcmp(h, kMagic, 8) != 0) {
    return fail(error, kIoInvalid, "not a hipstore delta file (bad magic)");
  }
  if (get_u32(h + 60) != crc32c_sw(0, h, 60)) {
    return fail(error, kIoInvalid, "header CRC mismatch");
  }
  DeltaInfo& info = out->info;
  info.version = get_u32(h + 8);
  info.block_size = get_u32(h + 12);
  info.granule = get_u32(h + 16);
  const uint32_t flags = get_u32(h + 20);
  info.full = (flags & kDeltaFlagFull) != 0;
  info.volume_bytes = get_u64(h + 24);
  info.n_granules = get_u64(h + 32);
  info.n_marked = get_u64(h + 40);
  info.file_bytes = file_bytes;
  const uint32_t bitmap_crc = get_u32(h + 48);
  if (info.version != kDeltaVersion) {
    return fail(error, kIoInvalid, "unsupported delta file version");
  }
  if ((flags & ~kDeltaFlagFull) != 0 || get_u32(h + 52) != 0 ||
      get_u32(h + 56) != 0) {
    return fail(error, kIoInvalid, "unknown flags or non-zero reserved field");
  }
  if (info.block_size == 0 || info.granule == 0 ||
      info.granule % info.block_size != 0 || info.granule % 16 != 0 ||
      info.n_granules == 0 || info.n_granules > kMaxGranules ||
      info.volume_bytes / info.granule != info.n_granules ||
      info.volume_bytes % info.granule != 0 ||
      info.n_marked > info.n_granules ||
      (info.full && info.n_marked != info.n_granules)) {
    return fail(error, kIoInvalid, "inconsistent geometry in header");
  }
  // n_marked <= n_granules <= 2^31 and granule < 2^32: no sum wraps.
  const uint64_t n_words = (info.n_granules + 63) / 64;
  const uint64_t per_record = record_granules(info.granule);
  const uint64_t n_records = (info.n_marked + per_record - 1) / per_record;
  const uint64_t expected = kDeltaHeaderBytes + n_words * 8 + n_records * 8 +
                            info.n_marked * info.granule + kDeltaTrailerBytes;
  if (file_bytes != expected) {
    return fail(error, kIoInvalid,
                "file length " + std::to_string(file_bytes) +
                    " does not follow from the header (" +
                    std::to_string(expected) + ")");
  }
  std::vector<uint8_t> raw(n_words * 8);
  if (!read_all(fd, raw.data(), raw.size(), kDeltaHeaderBytes)) {
    return fail(error, kIoFailed, "cannot read bitmap");
  }
  if (crc32c_sw(0, raw.data(), raw.size()) != bitmap_crc) {
    return fail(error, kIoInvalid, "bitmap CRC mismatch");
  }
  out->bitmap.resize(n_words);
  uint64_t marked = 0;
  for (uint64_t w = 0; w < n_words; ++w) {
    out->bitmap[w] = get_u64(&raw[w * 8]);
    marked += static_cast<uint64_t>(__builtin_popcountll(out->bitmap[w]));
  }
  if (info.n_granules % 64 != 0 &&
      (out->bitmap.back() >> (info.n_granules % 64)) != 0) {
    return fail(error, kIoInvalid, "bitmap has bits past the last granule");
  }
  if (marked != info.n_marked) {
    return fail(error, kIoInvalid, "n_marked disagrees with the bitmap");
  }
  uint8_t t[kDeltaTrailerBytes];
  if (!read_all(fd, t, sizeof(t), file_bytes - kDeltaTrailerBytes)) {
    return fail(error, kIoFailed, "cannot read trailer");
  }
  if (memcmp(t, kEndMagic, 8) != 0 || get_u64(t + 8) != info.n_marked) {
    return fail(error, kIoInvalid, "bad trailer");
  }
  out->records_offset = kDeltaHeaderBytes + n_words * 8;
  return kIoOk;
}

// Reads records in order and hands out their granules in whatever
// chunks the caller asks for; a record's CRC is checked before any of
// its bytes leave.
class RecordReader {
 public:
  RecordReader(int fd, const ParsedFile& file)
      : fd_(fd), granule_(file.info.granule), left_(file.info.n_marked),
        per_record_(record_granules(file.info.granule)),
        offset_(file.records_offset) {
    buf_.resize(std::min(per_record_, std::max<uint64_t>(left_, 1)) *
                granule_);
  }

  // data == nullptr: verify only.
  int take(uint8_t* data, uint64_t count, std::string* error) {
    while (count > 0) {
      if (pos_ == have_) {
        const int status = next_record(error);
        if (status != kIoOk) return status;
      }
      const uint64_t n = std::min(count, have_ - pos_);
      if (data != nullptr) {
        memcpy(data, &buf_[pos_ * granule_], n * granule_);
        data += n * granule_;
      }
      pos_ += n;
      count -= n;
    }
    return kIoOk;
  }

  uint64_t left() const { return left_ + (have_ - pos_); }

 private:
  int next_record(std::string* error) {
    const uint64_t want = std::min(per_record_, left_);
    if (want == 0) return fail(error, kIoInvalid, "record stream exhausted");
    uint8_t head[8];
    if (!read_all(fd_, head, 8, offset_)) {
      return fail(error, kIoFailed, "cannot read record header");
    }
    if (get_u32(head) != want) {
      return fail(error, kIoInvalid,
                  "record " + std::to_string(index_) + " has a wrong count");
    }
    if (!read_all(fd_, buf_.data(), want * granule_, offset_ + 8)) {
      return fail(error, kIoFailed, "cannot read record payload");
    }
    if (crc32c_sw(0, buf_.data(), want * granule_) != get_u32(head + 4)) {
      return fail(error, kIoInvalid,
                  "record " + std::to_string(index_) + " CRC mismatch");
    }
    offset_ += 8 + want * granule_;
    left_ -= want;
    have_ = want;
    pos_ = 0;
    ++index_;
    return kIoOk;
  }

  int fd_;
  uint32_t granule_;
  uint64_t left_;  // granules in records not yet read
  uint64_t per_record_;
  uint64_t offset_;
  uint64_t have_ = 0;
  uint64_t pos_ = 0;
  uint64_t index_ = 0;
  std::vector<uint8_t> buf_;
};

// --- fingerprint maps --------------------------------------------------------

const char kMapMagic[8] = {'H', 'S', 'F', 'P', 'M', 'A', 'P', '1'};
const char kMapEndMagic[8] = {'H', 'S', 'F', 'P', 'E', 'N', 'D', '1'};

struct LoadedMap {
  FingerprintMapInfo info;
  std::vector<uint8_t> fps;  // n_granules * 16 bytes
};

// Structural pass, then every record with its CRC checked before its
// bytes are kept.
int load_map(const std::string& path, LoadedMap* out, std::string* error) {
  Fd in;
  in.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (in.fd < 0) return fail(error, kIoFailed, errno_text("open " + path));
  struct stat st;
  if (fstat(in.fd, &st) != 0) {
    return fail(error, kIoFailed, errno_text("fstat"));
  }
  if (!S_ISREG(st.st_mode)) {
    return fail(error, kIoInvalid, "not a regular file");
  }
  const uint64_t file_bytes = static_cast<uint64_t>(st.st_size);
  uint8_t h[kDeltaHeaderBytes];
  if (file_bytes < kDeltaHeaderBytes + kDeltaTrailerBytes ||
      !read_all(in.fd, h, sizeof(h), 0)) {
    return fail(error, kIoInvalid, "file shorter than header and trailer");
  }
  if (memcmp(h, kMapMagic, 8) != 0) {
    return fail(error, kIoInvalid,
                "not a hipstore fingerprint map (bad magic)");
  }
  if (get_u32(h + 60) != crc32c_sw(0, h, 60)) {
    return fail(error, kIoInvalid, "header CRC mismatch");
  }
  FingerprintMapInfo& info = out->info;
  info.version = get_u32(h + 8);
  info.block_size = get_u32(h + 12);
  info.granule = get_u32(h + 16);
  info.algorithm = get_u32(h + 20);
  info.volume_bytes = get_u64(h + 24);
  info.n_granules = get_u64(h + 32);
  info.file_bytes = file_bytes;
  if (info.version != kFingerprintMapVersion) {
    return fail(error, kIoInvalid, "unsupported fingerprint map version");
  }
  if (info.algorithm != kFingerprintAlgorithm) {
    return fail(error, kIoInvalid, "unknown fingerprint algorithm");
  }
  for (int at = 40; at < 60; ++at) {
    if (h[at] != 0) {
      return fail(error, kIoInvalid, "non-zero reserved field");
    }
  }
  if (info.block_size == 0 || info.granule == 0 ||
      info.granule % info.block_size != 0 || info.granule % 16 != 0 ||
      info.n_granules == 0 || info.n_granules > kMaxGranules ||
      info.volume_bytes / info.granule != info.n_granules ||
      info.volume_bytes % info.granule != 0) {
    return fail(error, kIoInvalid, "inconsistent geometry in header");
  }
  // n_granules <= 2^31: no sum wraps.
  const uint64_t n_records =
      (info.n_granules + kFingerprintMapRecord - 1) / kFingerprintMapRecord;
  const uint64_t expected = kDeltaHeaderBytes + n_records * 8 +
                            info.n_granules * kFingerprintBytes +
                            kDeltaTrailerBytes;
  if (file_bytes != expected) {
    return fail(error, kIoInvalid,
                "file length " + std::to_string(file_bytes) +
                    " does not follow from the header (" +
                    std::to_string(expected) + ")");
  }
  uint8_t t[kDeltaTrailerBytes];
  if (!read_all(in.fd, t, sizeof(t), file_bytes - kDeltaTrailerBytes)) {
    return fail(error, kIoFailed, "cannot read trailer");
  }
  if (memcmp(t, kMapEndMagic, 8) != 0 || get_u64(t + 8) != info.n_granules) {
    return fail(error, kIoInvalid, "bad trailer");
  }
  out->fps.resize(info.n_granules * kFingerprintBytes);
  uint64_t offset = kDeltaHeaderBytes;
  for (uint64_t first = 0, index = 0; first < info.n_granules; ++index) {
    const uint64_t want =
        std::min(kFingerprintMapRecord, info.n_granules - first);
    uint8_t head[8];
    uint8_t* payload = &out->fps[first * kFingerprintBytes];
    if (!read_all(in.fd, head, 8, offset) ||
        !read_all(in.fd, payload, want * kFingerprintBytes, offset + 8)) {
      return fail(error, kIoFailed, "cannot read record");
    }
    if (get_u32(head) != want) {
      return fail(error, kIoInvalid,
                  "record " + std::to_string(index) + " has a wrong count");
    }
    if (crc32c_sw(0, payload, want * kFingerprintBytes) != get_u32(head + 4)) {
      return fail(error, kIoInvalid,
                  "record " + std::to_string(index) + " CRC mismatch");
    }
    offset += 8 + want * kFingerprintBytes;
    first += want;
  }
  return kIoOk;
}

// Writes a complete, synced map to `tmp`; the caller renames it.
int write_map_tmp(const std::string& tmp, uint32_t block_size,
                  uint32_t granule, const std::vector<uint8_t>& fps,
                  uint64_t* file_bytes, std::string* error) {
  const uint64_t n_granules = fps.size() / kFingerprintBytes;
  Fd out;
  out.fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (out.fd < 0) return fail(error, kIoFailed, errno_text("open " + tmp));
  uint8_t h[kDeltaHeaderBytes] = {0};
  memcpy(h, kMapMagic, 8);
  put_u32(h + 8, kFingerprintMapVersion);
  put_u32(h + 12, block_size);
  put_u32(h + 16, granule);
  put_u32(h + 20, kFingerprintAlgorithm);
  put_u64(h + 24, n_granules * granule);
  put_u64(h + 32, n_granules);
  put_u32(h + 60, crc32c_sw(0, h, 60));
  bool ok = write_all(out.fd, h, sizeof(h));
  uint64_t bytes = sizeof(h);
  for (uint64_t first = 0; ok && first < n_granules;) {
    const uint64_t count =
        std::min(kFingerprintMapRecord, n_granules - first);
    const uint8_t* payload = &fps[first * kFingerprintBytes];
    uint8_t head[8];
    put_u32(head, static_cast<uint32_t>(count));
    put_u32(head + 4, crc32c_sw(0, payload, count * kFingerprintBytes));
    ok = write_all(out.fd, head, 8) &&
         write_all(out.fd, payload, count * kFingerprintBytes);
    bytes += 8 + count * kFingerprintBytes;
    first += count;
  }
  uint8_t t[kDeltaTrailerBytes];
  memcpy(t, kMapEndMagic, 8);
  put_u64(t + 8, n_granules);
  bytes += sizeof(t);
  if (!ok || !write_all(out.fd, t, sizeof(t)) || fsync(out.fd) != 0) {
    const std::string why = errno_text("write " + tmp);
    unlink(tmp.c_str());
    return fail(error, kIoFailed, why);
  }
  *file_bytes = bytes;
  return kIoOk;
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

const char kBadGranule[] =
    "invalid granule (a multiple of the block size and of 16 that divides "
    "the volume size)";

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
  const uint64_t length = src->size_bytes();
  if (src->block_size() > UINT32_MAX) {
    return fail(error, kIoInvalid, "block size too large");
  }
  LoadedMap stored;
  if (!base_map.empty()) {
    const int status = load_map(base_map, &stored, error);
    if (status != kIoOk) return status;
    if (granule != 0 && granule != stored.info.granule) {
      return fail(error, kIoInvalid,
                  "granule differs from the base map's (" +
                      std::to_string(stored.info.granule) + ")");
    }
    granule = stored.info.granule;
    if (stored.info.block_size != src->block_size() ||
        stored.info.volume_bytes > length) {
      return fail(error, kIoInvalid,
                  "base map has another block size or a larger volume");
    }
  }
  if (granule == 0) granule = static_cast<uint32_t>(src->block_size());
  if (base != nullptr && (base->block_size() != src->block_size() ||
                          base->size_bytes() != length)) {
    return fail(error, kIoInvalid,
                "base and volume differ in block size or size");
  }
  std::vector<uint64_t> bitmap;
  std::vector<uint8_t> fps;  // of src, when map_out asks for them
  uint64_t n_marked = 0;
  if (!base_map.empty()) {
    const int status =
        fingerprint_pass(src, length, granule, &stored.fps, &bitmap,
                         map_out.empty() ? nullptr : &fps);
    if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
    if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
    for (uint64_t word : bitmap) {
      n_marked += static_cast<uint64_t>(__builtin_popcountll(word));
    }
  } else if (base != nullptr) {
    DiffStats diff;
    const int status =
        bdev_diff_sync(base, 0, src, 0, length, granule, 0, &bitmap, &diff);
    if (status == kIoInvalid) {
      return fail(error, kIoInvalid, kBadGranule);
    }
    if (status != kIoOk) return fail(error, kIoFailed, "compare failed");
    n_marked = diff.mismatched;
  } else {
    if (granule % 16 != 0 || granule % src->block_size() != 0 ||
        length == 0 || length % granule != 0 ||
        length / granule > kMaxGranules) {
      return fail(error, kIoInvalid, kBadGranule);
    }
    n_marked = length / granule;
    bitmap.assign((n_marked + 63) / 64, ~0ull);
    if (n_marked % 64 != 0) bitmap.back() = (1ull << (n_marked % 64)) - 1;
  }
  const uint64_t n_granules = length / granule;
  const bool full = base == nullptr && base_map.empty();

  struct stat st;
  if (!overwrite && lstat(path.c_str(), &st) == 0) {
    return fail(error, kIoFailed, path + " exists (overwrite not set)");
  }
  if (!overwrite && !map_out.empty() && lstat(map_out.c_str(), &st) == 0) {
    return fail(error, kIoFailed, map_out + " exists (overwrite not set)");
  }
  // The map is taken before the pack pass: a write in between leaves it
  // older than the exported data, never newer.
  if (!map_out.empty() && base_map.empty()) {
    const int status =
        fingerprint_pass(src, length, granule, nullptr, nullptr, &fps);
    if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
  }
  const std::string tmp = path + ".tmp";
  const std::string map_tmp = map_out + ".tmp";
  Fd out;
  out.fd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
  if (out.fd < 0) return fail(error, kIoFailed, errno_text("open " + tmp));

  const std::vector<uint8_t> raw = bitmap_bytes(bitmap);
  uint8_t h[kDeltaHeaderBytes] = {0};
  memcpy(h, kMagic, 8);
  put_u32(h + 8, kDeltaVersion);
  put_u32(h + 12, static_cast<uint32_t>(src->block_size()));
  put_u32(h + 16, granule);
  put_u32(h + 20, full ? kDeltaFlagFull : 0);
  put_u64(h + 24, length);
  put_u64(h + 32, n_granules);
  put_u64(h + 40, n_marked);
  put_u32(h + 48, crc32c_sw(0, raw.data(), raw.size()));
  put_u32(h + 60, crc32c_sw(0, h, 60));

  int status = kIoOk;
  std::string why;
  uint64_t file_bytes = sizeof(h) + raw.size();
  if (!write_all(out.fd, h, sizeof(h)) ||
      !write_all(out.fd, raw.data(), raw.size())) {
    status = kIoFailed;
    why = errno_text("write " + tmp);
  }
  if (status == kIoOk) {
    RecordWriter writer(out.fd, granule, n_marked);
    uint64_t packed = 0;
    status = bdev_pack_marked_sync(
        src, 0, length, granule, bitmap, 0,
        [&writer](const uint8_t* data, uint64_t, uint64_t count) {
          return writer.add(data, count);
        },
        &packed);
    if (status == kIoOk && (packed != n_marked || !writer.complete())) {
      status = kIoFailed;
    }
    if (status != kIoOk) why = "reading the volume or writing " + tmp + " failed";
    file_bytes += writer.bytes();
  }
  if (status == kIoOk) {
    uint8_t t[kDeltaTrailerBytes];
    memcpy(t, kEndMagic, 8);
    put_u64(t + 8, n_marked);
    file_bytes += sizeof(t);
    if (!write_all(out.fd, t, sizeof(t)) || fsync(out.fd) != 0) {
      status = kIoFailed;
      why = errno_text("write " + tmp);
    }
  }
  // Both files are complete under their .tmp names before either
  // appears; the map follows the delta it belongs to.
  uint64_t map_bytes = 0;
  bool map_written = false;
  if (status == kIoOk && !map_out.empty()) {
    status = write_map_tmp(map_tmp, static_cast<uint32_t>(src->block_size()),
                           granule, fps, &map_bytes, &why);
    map_written = status == kIoOk;
  }
  if (status == kIoOk && rename(tmp.c_str(), path.c_str()) != 0) {
    status = kIoFailed;
    why = errno_text("rename to " + path);
  }
  if (status != kIoOk) {
    unlink(tmp.c_str());
    if (map_written) unlink(map_tmp.c_str());
    return fail(error, status == kIoInvalid ? kIoInvalid : kIoFailed, why);
  }
  if (map_written && rename(map_tmp.c_str(), map_out.c_str()) != 0) {
    why = errno_text("rename to " + map_out);
    unlink(map_tmp.c_str());
    return fail(error, kIoFailed, why + " (" + path + " was written)");
  }
  if (maps != nullptr) maps->map_bytes = map_bytes;
  if (stats != nullptr) {
    stats->version = kDeltaVersion;
    stats->block_size = static_cast<uint32_t>(src->block_size());
    stats->granule = granule;
    stats->full = full;
    stats->volume_bytes = length;
    stats->n_granules = n_granules;
    stats->n_marked = n_marked;
    stats->file_bytes = file_bytes;
  }
  return kIoOk;
}

int delta_file_info(const std::string& path, DeltaInfo* info,
                    std::string* error) {
  Fd in;
  in.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (in.fd < 0) return fail(error, kIoFailed, errno_text("open " + path));
  ParsedFile file;
  const int status = parse_file(in.fd, &file, error);
  if (status == kIoOk && info != nullptr) *info = file.info;
  return status;
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
  const uint64_t length = bdev->size_bytes();
  struct stat st;
  if (!overwrite && lstat(path.c_str(), &st) == 0) {
    return fail(error, kIoFailed, path + " exists (overwrite not set)");
  }
  std::vector<uint8_t> fps;
  int status = fingerprint_pass(bdev, length, granule, nullptr, nullptr, &fps);
  if (status == kIoInvalid) return fail(error, kIoInvalid, kBadGranule);
  if (status != kIoOk) return fail(error, kIoFailed, "fingerprint pass failed");
  const std::string tmp = path + ".tmp";
  uint64_t file_bytes = 0;
  status = write_map_tmp(tmp, static_cast<uint32_t>(bdev->block_size()),
                         granule, fps, &file_bytes, error);
  if (status != kIoOk) return status;
  if (rename(tmp.c_str(), path.c_str()) != 0) {
    const std::string why = errno_text("rename to " + path);
    unlink(tmp.c_str());
    return fail(error, kIoFailed, why);
  }
  if (stats != nullptr) {
    stats->version = kFingerprintMapVersion;
    stats->block_size = static_cast<uint32_t>(bdev->block_size());
    stats->granule = granule;
    stats->algorithm = kFingerprintAlgorithm;
    stats->volume_bytes = length;
    stats->n_granules = length / granule;
    stats->file_bytes = file_bytes;
  }
  return kIoOk;
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
    stats->mismatched = 0;
    stats->first_mismatches.clear();
    for (uint64_t w = 0; w < bitmap.size(); ++w) {
      uint64_t word = bitmap[w];
      stats->mismatched += static_cast<uint64_t>(__builtin_popcountll(word));
      while (word != 0 && stats->first_mismatches.size() < max_report) {
        stats->first_mismatches.push_back(
            w * 64 + static_cast<uint64_t>(__builtin_ctzll(word)));
        word &= word - 1;
      }
    }
  }
  return kIoOk;
}

int bdev_import_delta(Bdev* dst, const std::string& path, bool dry_run,
                      DeltaInfo* stats, std::string* error) {
  if (dst == nullptr || path.empty()) {
    return fail(error, kIoInvalid, "bdev and path required");
  }
  Fd in;
  in.fd = open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (in.fd < 0) return fail(error, kIoFailed, errno_text("open " + path));
  ParsedFile file;
  int status = parse_file(in.fd, &file, error);
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
  RecordReader reader(in.fd, file);
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

}  // namespace hipstore
