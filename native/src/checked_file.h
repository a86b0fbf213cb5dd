// The checked-file core under the on-disk formats of delta.h: a 64-byte
// header with a CRC, a stream of records with a CRC each, a 16-byte
// trailer, and an output file that takes its final name only complete.
// A format supplies its magics, the meaning of header bytes 20-23 and
// 40-59 and its body length; every other check and every cleanup rule
// is here, once.
//
// Plain host code: of the project it needs crc32c_sw and nothing else
// (hipstore/crc32c.h also brings the IoStatus values returned below).

#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "hipstore/crc32c.h"

namespace hipstore {
namespace checked_file {

constexpr uint64_t kHeaderBytes = 64;
constexpr uint64_t kTrailerBytes = 16;
// Same bound as the granule calls: 256 MiB of bitmap.
constexpr uint64_t kMaxGranules = 1ull << 31;

// Little-endian.
inline void put_u32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}
inline void put_u64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = static_cast<uint8_t>(v >> (8 * i));
}
inline uint32_t get_u32(const uint8_t* p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) v |= static_cast<uint32_t>(p[i]) << (8 * i);
  return v;
}
inline uint64_t get_u64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= static_cast<uint64_t>(p[i]) << (8 * i);
  return v;
}

// Sets *error (when given) and returns `status`.
int fail(std::string* error, int status, const std::string& what);

struct Fd {
  int fd = -1;
  Fd() = default;
  Fd(const Fd&) = delete;
  Fd& operator=(const Fd&) = delete;
  ~Fd();
};

struct Format {
  char magic[8];
  char end_magic[8];
  uint32_t version;
  const char* noun;  // "delta file", for messages
};

// Header bytes 12-59, in file order; magic, version and the CRC of bytes
// 0-59 at byte 60 belong to the codec.
struct Header {
  uint32_t block_size = 0;
  uint32_t granule = 0;
  uint32_t word = 0;  // bytes 20-23: the format's flags or algorithm
  uint64_t volume_bytes = 0;
  uint64_t n_granules = 0;
  uint8_t owned[20] = {0};  // bytes 40-59: the format's
};

// Non-zero block size and granule, granule a multiple of the block size
// and of 16, 1 <= n_granules <= kMaxGranules, volume_bytes ==
// n_granules * granule. With it, no length computed from a header wraps.
bool geometry_ok(uint64_t block_size, uint64_t granule, uint64_t volume_bytes,
                 uint64_t n_granules);

// Bytes of a record stream of `total` units: for each next
// min(remaining, per_record) units, u32 count, u32 crc32c(payload),
// count * unit bytes.
uint64_t record_stream_bytes(uint64_t total, uint64_t unit,
                             uint64_t per_record);

class InFile {
 public:
  // Checks, in this order: regular file, room for header and trailer,
  // magic, header CRC, version. kIoFailed when the file cannot be opened.
  int open(const std::string& path, const Format& format, std::string* error);
  // The file is exactly header, `body` bytes and trailer.
  int check_length(uint64_t body, std::string* error) const;
  // End magic and count.
  int check_trailer(uint64_t count, std::string* error) const;
  // Exactly `len` bytes at `offset`; false on error or a short file.
  bool read(void* data, size_t len, uint64_t offset) const;

  Header header;
  uint64_t file_bytes = 0;

 private:
  Fd in_;
  const Format* format_ = nullptr;
};

// Hands out the units of the record stream at `offset` in whatever
// chunks the caller asks for; a record's CRC is checked before any of
// its bytes leave. A wrong count or CRC is kIoInvalid and names the
// record, a failed read kIoFailed.
class RecordReader {
 public:
  RecordReader(const InFile* in, uint64_t offset, uint64_t unit,
               uint64_t per_record, uint64_t total);
  // data == nullptr: verify only.
  int take(uint8_t* data, uint64_t count, std::string* error);
  // Units not yet handed out.
  uint64_t left() const { return left_ + (have_ - pos_); }

 private:
  int next_record(std::string* error);

  const InFile* in_;
  uint64_t offset_, unit_, per_record_;
  uint64_t left_;  // units in records not yet read
  uint64_t have_ = 0, pos_ = 0;  // units in buf_, units of them handed out
  uint64_t index_ = 0;
  std::vector<uint8_t> buf_;
};

// Written as final_path + ".tmp"; the destructor removes a tmp file that
// was not published.
class OutFile {
 public:
  explicit OutFile(const std::string& final_path);
  ~OutFile();
  // Creates the tmp file and writes the header.
  int begin(const Format& format, const Header& header, std::string* error);
  // A failure stays: later writes fail too, and end() reports it.
  bool write(const void* data, size_t len);
  // Writes the trailer and syncs: the tmp file is complete.
  int end(uint64_t count, std::string* error);
  int publish(std::string* error);
  uint64_t bytes() const { return bytes_; }
  const std::string& tmp() const { return tmp_; }

 private:
  const std::string final_, tmp_;
  const Format* format_ = nullptr;
  Fd out_;
  uint64_t bytes_ = 0;
  bool failed_ = false, published_ = false;
};

// Cuts a dense stream of `total` units into records, whatever chunks
// add() receives.
class RecordWriter {
 public:
  RecordWriter(OutFile* out, uint64_t unit, uint64_t per_record,
               uint64_t total);
  // kIoFailed on a failed write or on more units than announced.
  int add(const uint8_t* data, uint64_t count);
  bool complete() const { return left_ == 0 && have_ == 0; }

 private:
  OutFile* out_;
  uint64_t unit_, per_record_;
  uint64_t left_;  // units not yet written
  uint64_t have_ = 0;  // units in buf_
  std::vector<uint8_t> buf_;
};

}  // namespace checked_file
}  // namespace hipstore
