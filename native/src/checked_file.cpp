// The checked-file core (checked_file.h).

#include "checked_file.h"

#include <errno.h>
#include <fcntl.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

namespace hipstore {
namespace checked_file {

namespace {

std::string errno_text(const std::string& what) {
  return what + ": " + strerror(errno);
}

// One record's worth of buffer, or less for a shorter stream.
uint64_t buffer_units(uint64_t per_record, uint64_t total) {
  return std::min(per_record, std::max<uint64_t>(total, 1));
}

}  // namespace

int fail(std::string* error, int status, const std::string& what) {
  if (error != nullptr) *error = what;
  return status;
}

Fd::~Fd() {
  if (fd >= 0) close(fd);
}

bool geometry_ok(uint64_t block_size, uint64_t granule, uint64_t volume_bytes,
                 uint64_t n_granules) {
  return block_size != 0 && granule != 0 && granule % block_size == 0 &&
         granule % 16 == 0 && n_granules != 0 && n_granules <= kMaxGranules &&
         volume_bytes / granule == n_granules && volume_bytes % granule == 0;
}

uint64_t record_stream_bytes(uint64_t total, uint64_t unit,
                             uint64_t per_record) {
  return (total + per_record - 1) / per_record * 8 + total * unit;
}

int InFile::open(const std::string& path, const Format& format,
                 std::string* error) {
  format_ = &format;
  in_.fd = ::open(path.c_str(), O_RDONLY | O_CLOEXEC);
  if (in_.fd < 0) return fail(error, kIoFailed, errno_text("open " + path));
  struct stat st;
  if (fstat(in_.fd, &st) != 0) {
    return fail(error, kIoFailed, errno_text("fstat"));
  }
  if (!S_ISREG(st.st_mode)) {
    return fail(error, kIoInvalid, "not a regular file");
  }
  file_bytes = static_cast<uint64_t>(st.st_size);
  uint8_t h[kHeaderBytes];
  if (file_bytes < kHeaderBytes + kTrailerBytes || !read(h, sizeof(h), 0)) {
    return fail(error, kIoInvalid, "file shorter than header and trailer");
  }
  const std::string noun = format.noun;
  if (memcmp(h, format.magic, 8) != 0) {
    return fail(error, kIoInvalid, "not a hipstore " + noun + " (bad magic)");
  }
  if (get_u32(h + 60) != crc32c_sw(0, h, 60)) {
    return fail(error, kIoInvalid, "header CRC mismatch");
  }
  if (get_u32(h + 8) != format.version) {
    return fail(error, kIoInvalid, "unsupported " + noun + " version");
  }
  header.block_size = get_u32(h + 12);
  header.granule = get_u32(h + 16);
  header.word = get_u32(h + 20);
  header.volume_bytes = get_u64(h + 24);
  header.n_granules = get_u64(h + 32);
  memcpy(header.owned, h + 40, sizeof(header.owned));
  return kIoOk;
}

int InFile::check_length(uint64_t body, std::string* error) const {
  const uint64_t expected = kHeaderBytes + body + kTrailerBytes;
  if (file_bytes == expected) return kIoOk;
  return fail(error, kIoInvalid,
              "file length " + std::to_string(file_bytes) +
                  " does not follow from the header (" +
                  std::to_string(expected) + ")");
}

int InFile::check_trailer(uint64_t count, std::string* error) const {
  uint8_t t[kTrailerBytes];
  if (!read(t, sizeof(t), file_bytes - kTrailerBytes)) {
    return fail(error, kIoFailed, "cannot read trailer");
  }
  if (memcmp(t, format_->end_magic, 8) != 0 || get_u64(t + 8) != count) {
    return fail(error, kIoInvalid, "bad trailer");
  }
  return kIoOk;
}

bool InFile::read(void* data, size_t len, uint64_t offset) const {
  uint8_t* p = static_cast<uint8_t*>(data);
  while (len > 0) {
    const ssize_t n = pread(in_.fd, p, len, static_cast<off_t>(offset));
    if (n < 0 && errno == EINTR) continue;
    if (n <= 0) return false;
    p += n;
    len -= static_cast<size_t>(n);
    offset += static_cast<uint64_t>(n);
  }
  return true;
}

RecordReader::RecordReader(const InFile* in, uint64_t offset, uint64_t unit,
                           uint64_t per_record, uint64_t total)
    : in_(in), offset_(offset), unit_(unit), per_record_(per_record),
      left_(total), buf_(buffer_units(per_record, total) * unit) {}

int RecordReader::take(uint8_t* data, uint64_t count, std::string* error) {
  while (count > 0) {
    if (pos_ == have_) {
      const int status = next_record(error);
      if (status != kIoOk) return status;
    }
    const uint64_t n = std::min(count, have_ - pos_);
    if (data != nullptr) {
      memcpy(data, &buf_[pos_ * unit_], n * unit_);
      data += n * unit_;
    }
    pos_ += n;
    count -= n;
  }
  return kIoOk;
}

int RecordReader::next_record(std::string* error) {
  const uint64_t want = std::min(per_record_, left_);
  if (want == 0) return fail(error, kIoInvalid, "record stream exhausted");
  uint8_t head[8];
  if (!in_->read(head, 8, offset_)) {
    return fail(error, kIoFailed, "cannot read record header");
  }
  if (get_u32(head) != want) {
    return fail(error, kIoInvalid,
                "record " + std::to_string(index_) + " has a wrong count");
  }
  if (!in_->read(buf_.data(), want * unit_, offset_ + 8)) {
    return fail(error, kIoFailed, "cannot read record payload");
  }
  if (crc32c_sw(0, buf_.data(), want * unit_) != get_u32(head + 4)) {
    return fail(error, kIoInvalid,
                "record " + std::to_string(index_) + " CRC mismatch");
  }
  offset_ += 8 + want * unit_;
  left_ -= want;
  have_ = want;
  pos_ = 0;
  ++index_;
  return kIoOk;
}

OutFile::OutFile(const std::string& final_path)
    : final_(final_path), tmp_(final_path + ".tmp") {}

OutFile::~OutFile() {
  if (out_.fd >= 0 && !published_) unlink(tmp_.c_str());
}

int OutFile::begin(const Format& format, const Header& header,
                   std::string* error) {
  format_ = &format;
  out_.fd = ::open(tmp_.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC,
                   0644);
  if (out_.fd < 0) return fail(error, kIoFailed, errno_text("open " + tmp_));
  uint8_t raw[kHeaderBytes];
  memcpy(raw, format.magic, 8);
  put_u32(raw + 8, format.version);
  put_u32(raw + 12, header.block_size);
  put_u32(raw + 16, header.granule);
  put_u32(raw + 20, header.word);
  put_u64(raw + 24, header.volume_bytes);
  put_u64(raw + 32, header.n_granules);
  memcpy(raw + 40, header.owned, sizeof(header.owned));
  put_u32(raw + 60, crc32c_sw(0, raw, 60));
  if (!write(raw, sizeof(raw))) {
    return fail(error, kIoFailed, errno_text("write " + tmp_));
  }
  return kIoOk;
}

bool OutFile::write(const void* data, size_t len) {
  const uint8_t* p = static_cast<const uint8_t*>(data);
  for (size_t done = 0; done < len && !failed_;) {
    const ssize_t n = ::write(out_.fd, p + done, len - done);
    if (n >= 0) {
      done += static_cast<size_t>(n);
    } else if (errno != EINTR) {
      failed_ = true;
    }
  }
  if (!failed_) bytes_ += len;
  return !failed_;
}

int OutFile::end(uint64_t count, std::string* error) {
  uint8_t t[kTrailerBytes];
  memcpy(t, format_->end_magic, 8);
  put_u64(t + 8, count);
  if (!write(t, sizeof(t)) || fsync(out_.fd) != 0) {
    return fail(error, kIoFailed, errno_text("write " + tmp_));
  }
  return kIoOk;
}

int OutFile::publish(std::string* error) {
  if (rename(tmp_.c_str(), final_.c_str()) != 0) {
    return fail(error, kIoFailed, errno_text("rename to " + final_));
  }
  published_ = true;
  return kIoOk;
}

RecordWriter::RecordWriter(OutFile* out, uint64_t unit, uint64_t per_record,
                           uint64_t total)
    : out_(out), unit_(unit), per_record_(per_record), left_(total),
      buf_(8 + buffer_units(per_record, total) * unit) {}

int RecordWriter::add(const uint8_t* data, uint64_t count) {
  while (count > 0) {
    const uint64_t want = std::min(per_record_, left_);
    if (want == 0) return kIoFailed;  // more units than announced
    const uint64_t take = std::min(count, want - have_);
    memcpy(&buf_[8 + have_ * unit_], data, take * unit_);
    have_ += take;
    data += take * unit_;
    count -= take;
    if (have_ == want) {
      put_u32(&buf_[0], static_cast<uint32_t>(have_));
      put_u32(&buf_[4], crc32c_sw(0, &buf_[8], have_ * unit_));
      if (!out_->write(buf_.data(), 8 + have_ * unit_)) return kIoFailed;
      left_ -= have_;
      have_ = 0;
    }
  }
  return kIoOk;
}

}  // namespace checked_file
}  // namespace hipstore
