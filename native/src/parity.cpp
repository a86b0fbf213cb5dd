// P+Q parity across bdevs (hipstore/parity.h): the GF(2^8) tables, the
// validation and path selection of the four calls, and their generic
// path through bdev_read_sync / bdev_write_sync.
//
// The generic path is a different algorithm from the kernels of
// parity_ops.hip on purpose: byte-wise log/exp table arithmetic, Q as
// the plain sum of g^i * D_i (no Horner, no packed doubling), so that
// comparing the two paths checks both.

#include "hipstore/parity.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <utility>

namespace hipstore {

// ---------------------------------------------------------------------------
// GF(2^8), polynomial 0x11D, generator 2
// ---------------------------------------------------------------------------

namespace {

struct GfTables {
  uint8_t exp[510] = {};  // exp[i] = g^i, doubled so log a + log b needs no mod
  uint8_t log[256] = {};  // log[0] is unused
};

constexpr GfTables make_gf_tables() {
  GfTables t;
  uint32_t x = 1;
  for (int i = 0; i < 255; ++i) {
    t.exp[i] = static_cast<uint8_t>(x);
    t.exp[i + 255] = static_cast<uint8_t>(x);
    t.log[x] = static_cast<uint8_t>(i);
    x <<= 1;
    if (x & 0x100) x ^= 0x11D;
  }
  return t;
}

constexpr GfTables kGf = make_gf_tables();
static_assert(kGf.exp[8] == 0x1D && kGf.exp[254] == 0x8E && kGf.log[2] == 1,
              "GF(2^8) tables over 0x11D");

// row[d] = c * d: one table per coefficient, one lookup per byte.
void mul_row(uint8_t c, uint8_t row[256]) {
  for (int d = 0; d < 256; ++d) row[d] = gf256_mul(c, static_cast<uint8_t>(d));
}

}  // namespace

uint8_t gf256_mul(uint8_t a, uint8_t b) {
  if (a == 0 || b == 0) return 0;
  return kGf.exp[kGf.log[a] + kGf.log[b]];
}

uint8_t gf256_inv(uint8_t a) { return kGf.exp[255 - kGf.log[a]]; }

uint8_t gf256_pow2(int exponent) {
  return kGf.exp[((exponent % 255) + 255) % 255];
}

ParityCoeffs parity_coeffs_one_by_q(uint32_t x) {
  return {0, gf256_pow2(-static_cast<int>(x))};
}

ParityCoeffs parity_coeffs_two(uint32_t x, uint32_t y) {
  const uint8_t gyx = gf256_pow2(static_cast<int>(y - x));
  const uint8_t d = gf256_inv(gyx ^ 1);  // y - x in 1..31: g^(y-x) != 1
  return {gf256_mul(gyx, d), gf256_mul(gf256_pow2(-static_cast<int>(x)), d)};
}

// ---------------------------------------------------------------------------
// Validation
// ---------------------------------------------------------------------------

namespace {

constexpr uint64_t kSpan = 1ull << 20;           // generic-path span cap
constexpr uint64_t kMaxGranules = 1ull << 31;    // bdev_diff_sync's limit

int fail(ParityReport* report, int status, const char* why) {
  if (report != nullptr) report->error = why;
  return status;
}

bool same_store(Bdev* a, Bdev* b) {
  if (a == b) return true;
  void* base = a->device_base();
  return base != nullptr && base == b->device_base() &&
         a->gpu_device() == b->gpu_device();
}

// The rules common to the three calls; on success `all` holds every
// member given, data first, then P, then Q.
int validate_set(const std::vector<ParityMember>& data, ParityMember p,
                 ParityMember q, uint64_t length,
                 std::vector<ParityMember>* all, ParityReport* report) {
  if (report != nullptr) *report = ParityReport{};
  if (data.empty() || data.size() > kParityMaxData) {
    return fail(report, kIoInvalid, "between 1 and 32 data members are needed");
  }
  if (p.bdev == nullptr && q.bdev == nullptr) {
    return fail(report, kIoInvalid, "neither p nor q given");
  }
  *all = data;
  if (p.bdev != nullptr) all->push_back(p);
  if (q.bdev != nullptr) all->push_back(q);
  for (const ParityMember& m : *all) {
    if (m.bdev == nullptr) {
      return fail(report, kIoInvalid, "a data member is missing");
    }
  }
  const uint64_t bs = (*all)[0].bdev->block_size();
  if (bs == 0 || bs > kSpan) {
    return fail(report, kIoInvalid, "unsupported block size");
  }
  for (const ParityMember& m : *all) {
    if (m.bdev->block_size() != bs) {
      return fail(report, kIoInvalid, "members do not share a block size");
    }
  }
  if (length == 0 || length % bs != 0 || length % 16 != 0) {
    return fail(report, kIoInvalid,
                "length must be a non-zero multiple of the block size and "
                "of 16");
  }
  for (const ParityMember& m : *all) {
    if (m.offset % bs != 0) {
      return fail(report, kIoInvalid,
                  "offsets must be multiples of the block size");
    }
    // By subtraction: no 64-bit sum that could wrap.
    const uint64_t size = m.bdev->size_bytes();
    if (length > size || m.offset > size - length) {
      return fail(report, kIoInvalid, "range out of bounds");
    }
  }
  for (size_t i = 0; i < all->size(); ++i) {
    for (size_t j = i + 1; j < all->size(); ++j) {
      if (same_store((*all)[i].bdev, (*all)[j].bdev)) {
        return fail(report, kIoInvalid,
                    "a bdev or backing store appears twice in the set");
      }
    }
  }
  return kIoOk;
}

// The granule rules of the check and update calls.
int validate_granule(uint64_t bs, uint64_t length, uint32_t granule,
                     ParityReport* report) {
  if (granule == 0 || granule % bs != 0 || granule % 16 != 0) {
    return fail(report, kIoInvalid,
                "granule must be a multiple of the block size and of 16");
  }
  if (length % granule != 0) {
    return fail(report, kIoInvalid,
                "length must be a multiple of the granule");
  }
  if (length / granule > kMaxGranules) {
    return fail(report, kIoInvalid, "too many granules");
  }
  return kIoOk;
}

// GPU path or not: one device reaches every member (`first` decides
// which) and every offset keeps the 16-byte alignment of the bases.
int select_device(const std::vector<ParityMember>& all, Bdev* first) {
  std::vector<Bdev*> members{first};
  for (const ParityMember& m : all) {
    if (m.offset % 16 != 0) return -1;
    if (m.bdev != first) members.push_back(m.bdev);
  }
  return parity_kernel_device(members);
}

uint8_t* device_ptr(const ParityMember& m) {
  if (m.bdev == nullptr) return nullptr;
  return static_cast<uint8_t*>(m.bdev->device_base()) + m.offset;
}

ParitySet device_set(const std::vector<ParityMember>& data) {
  ParitySet set{};
  set.k = static_cast<uint32_t>(data.size());
  for (uint32_t i = 0; i < set.k; ++i) set.data[i] = device_ptr(data[i]);
  return set;
}

// ---------------------------------------------------------------------------
// Generic path
// ---------------------------------------------------------------------------

// Per-thread pinned spans, kept like the buffers of the other bulk
// calls (a pinned free waits for the device to go idle).
struct SpanBufs {
  uint8_t* base = nullptr;
  ~SpanBufs() { free_pinned(base); }
  uint8_t* get(int which) {
    if (base == nullptr) base = static_cast<uint8_t*>(alloc_pinned(4 * kSpan));
    return base == nullptr ? nullptr : base + which * kSpan;
  }
};

SpanBufs& span_bufs() {
  thread_local SpanBufs bufs;
  return bufs;
}

// P and Q sums of the members of `data` that are present, over
// [pos, pos + n) of the range, into sum_p / sum_q (either may be null).
int span_sums(const std::vector<ParityMember>& data, uint64_t pos, uint64_t n,
              uint8_t* in, uint8_t* sum_p, uint8_t* sum_q) {
  if (sum_p != nullptr) memset(sum_p, 0, n);
  if (sum_q != nullptr) memset(sum_q, 0, n);
  uint8_t row[256];
  for (size_t i = 0; i < data.size(); ++i) {
    if (data[i].bdev == nullptr) continue;  // lost: contributes nothing
    const int status = bdev_read_sync(data[i].bdev, data[i].offset + pos, in, n);
    if (status != kIoOk) return status;
    if (sum_p != nullptr) {
      for (uint64_t b = 0; b < n; ++b) sum_p[b] ^= in[b];
    }
    if (sum_q != nullptr) {
      mul_row(gf256_pow2(static_cast<int>(i)), row);
      for (uint64_t b = 0; b < n; ++b) sum_q[b] ^= row[in[b]];
    }
  }
  return kIoOk;
}

// Largest multiple of the block size (<= kSpan, validated) in the cap.
uint64_t span_bytes(uint64_t block_size) {
  return kSpan / block_size * block_size;
}

int encode_generic(const std::vector<ParityMember>& data, ParityMember p,
                   ParityMember q, uint64_t length) {
  uint8_t* in = span_bufs().get(0);
  if (in == nullptr) return kIoFailed;
  uint8_t* sum_p = p.bdev != nullptr ? span_bufs().get(1) : nullptr;
  uint8_t* sum_q = q.bdev != nullptr ? span_bufs().get(2) : nullptr;
  const uint64_t span = span_bytes(data[0].bdev->block_size());
  for (uint64_t pos = 0; pos < length; pos += span) {
    const uint64_t n = std::min(span, length - pos);
    int status = span_sums(data, pos, n, in, sum_p, sum_q);
    if (status == kIoOk && sum_p != nullptr) {
      status = bdev_write_sync(p.bdev, p.offset + pos, sum_p, n);
    }
    if (status == kIoOk && sum_q != nullptr) {
      status = bdev_write_sync(q.bdev, q.offset + pos, sum_q, n);
    }
    if (status != kIoOk) return status;
  }
  return kIoOk;
}

// Marks the granules of [pos, pos + n) in which `sum` and `stored`
// differ; a span need not start or end on a granule boundary.
void mark_span(const uint8_t* sum, const uint8_t* stored, uint64_t pos,
               uint64_t n, uint32_t granule, std::vector<uint64_t>* words) {
  for (uint64_t off = 0; off < n;) {
    const uint64_t g = (pos + off) / granule;
    const uint64_t piece =
        std::min<uint64_t>(granule - (pos + off) % granule, n - off);
    if (memcmp(sum + off, stored + off, piece) != 0) {
      (*words)[g / 64] |= 1ull << (g % 64);
    }
    off += piece;
  }
}

int check_generic(const std::vector<ParityMember>& data, ParityMember p,
                  ParityMember q, uint64_t length, uint32_t granule,
                  std::vector<uint64_t>* p_words,
                  std::vector<uint64_t>* q_words) {
  uint8_t* in = span_bufs().get(0);
  if (in == nullptr) return kIoFailed;
  uint8_t* sum_p = p.bdev != nullptr ? span_bufs().get(1) : nullptr;
  uint8_t* sum_q = q.bdev != nullptr ? span_bufs().get(2) : nullptr;
  const uint64_t n_words = (length / granule + 63) / 64;
  if (sum_p != nullptr) p_words->assign(n_words, 0);
  if (sum_q != nullptr) q_words->assign(n_words, 0);
  const uint64_t span = span_bytes(data[0].bdev->block_size());
  for (uint64_t pos = 0; pos < length; pos += span) {
    const uint64_t n = std::min(span, length - pos);
    int status = span_sums(data, pos, n, in, sum_p, sum_q);
    if (status == kIoOk && sum_p != nullptr) {
      status = bdev_read_sync(p.bdev, p.offset + pos, in, n);
      if (status == kIoOk) mark_span(sum_p, in, pos, n, granule, p_words);
    }
    if (status == kIoOk && sum_q != nullptr) {
      status = bdev_read_sync(q.bdev, q.offset + pos, in, n);
      if (status == kIoOk) mark_span(sum_q, in, pos, n, granule, q_words);
    }
    if (status != kIoOk) return status;
  }
  return kIoOk;
}

// `survivors` has null bdevs in the lost slots; p / q are null when the
// coefficients do not need them.
int rebuild_generic(const std::vector<ParityMember>& survivors, ParityMember p,
                    ParityMember q, ParityCoeffs coeffs, ParityMember out_a,
                    ParityMember out_b, uint64_t length) {
  uint8_t* in = span_bufs().get(0);
  if (in == nullptr) return kIoFailed;
  uint8_t* syn_p = coeffs.a != 0 ? span_bufs().get(1) : nullptr;
  uint8_t* syn_q = coeffs.b != 0 ? span_bufs().get(2) : nullptr;
  uint8_t* out = span_bufs().get(3);
  uint8_t row_a[256];
  uint8_t row_b[256];
  mul_row(coeffs.a, row_a);
  mul_row(coeffs.b, row_b);
  const uint64_t span = span_bytes(out_a.bdev->block_size());
  for (uint64_t pos = 0; pos < length; pos += span) {
    const uint64_t n = std::min(span, length - pos);
    int status = span_sums(survivors, pos, n, in, syn_p, syn_q);
    if (status != kIoOk) return status;
    memset(out, 0, n);
    if (syn_p != nullptr) {
      status = bdev_read_sync(p.bdev, p.offset + pos, in, n);
      if (status != kIoOk) return status;
      for (uint64_t b = 0; b < n; ++b) {
        syn_p[b] ^= in[b];
        out[b] = row_a[syn_p[b]];
      }
    }
    if (syn_q != nullptr) {
      status = bdev_read_sync(q.bdev, q.offset + pos, in, n);
      if (status != kIoOk) return status;
      for (uint64_t b = 0; b < n; ++b) out[b] ^= row_b[syn_q[b] ^ in[b]];
    }
    status = bdev_write_sync(out_a.bdev, out_a.offset + pos, out, n);
    if (status == kIoOk && out_b.bdev != nullptr) {
      for (uint64_t b = 0; b < n; ++b) out[b] ^= syn_p[b];
      status = bdev_write_sync(out_b.bdev, out_b.offset + pos, out, n);
    }
    if (status != kIoOk) return status;
  }
  return kIoOk;
}

// Update from the bases (null bdev = untracked), span by span: the
// deltas of the tracked members are summed with the tables, then XORed
// into the stored parity wherever a member differed. `flags` has one
// entry per piece of the span (a piece is the part of one granule inside
// the span), so that parity is read and written in runs of dirty pieces
// and never inside a granule whose bit stays clear.
int update_generic(const std::vector<ParityMember>& data, ParityMember p,
                   ParityMember q, const std::vector<ParityMember>& bases,
                   uint64_t length, uint32_t granule, bool refresh,
                   std::vector<uint64_t>* words) {
  uint8_t* nw = span_bufs().get(0);
  if (nw == nullptr) return kIoFailed;
  uint8_t* old = span_bufs().get(1);
  uint8_t* sum_p = p.bdev != nullptr ? span_bufs().get(2) : nullptr;
  uint8_t* sum_q = q.bdev != nullptr ? span_bufs().get(3) : nullptr;
  words->assign((length / granule + 63) / 64, 0);
  const uint64_t span = span_bytes(data[0].bdev->block_size());
  std::vector<uint8_t> flags;
  uint8_t row[256];
  for (uint64_t pos = 0; pos < length; pos += span) {
    const uint64_t n = std::min(span, length - pos);
    if (sum_p != nullptr) memset(sum_p, 0, n);
    if (sum_q != nullptr) memset(sum_q, 0, n);
    flags.clear();
    for (size_t i = 0; i < data.size(); ++i) {
      if (bases[i].bdev == nullptr) continue;
      int status = bdev_read_sync(data[i].bdev, data[i].offset + pos, nw, n);
      if (status == kIoOk) {
        status = bdev_read_sync(bases[i].bdev, bases[i].offset + pos, old, n);
      }
      if (status != kIoOk) return status;
      bool differs = false;
      size_t piece_index = 0;
      for (uint64_t off = 0; off < n; ++piece_index) {
        const uint64_t g = (pos + off) / granule;
        const uint64_t piece =
            std::min<uint64_t>(granule - (pos + off) % granule, n - off);
        if (piece_index == flags.size()) flags.push_back(0);
        if (memcmp(nw + off, old + off, piece) != 0) {
          flags[piece_index] = 1;
          (*words)[g / 64] |= 1ull << (g % 64);
          differs = true;
        }
        off += piece;
      }
      if (!differs) continue;
      for (uint64_t b = 0; b < n; ++b) old[b] ^= nw[b];  // d_i
      if (sum_p != nullptr) {
        for (uint64_t b = 0; b < n; ++b) sum_p[b] ^= old[b];
      }
      if (sum_q != nullptr) {
        mul_row(gf256_pow2(static_cast<int>(i)), row);
        for (uint64_t b = 0; b < n; ++b) sum_q[b] ^= row[old[b]];
      }
      if (refresh) {
        status = bdev_write_sync(bases[i].bdev, bases[i].offset + pos, nw, n);
        if (status != kIoOk) return status;
      }
    }
    // Runs of dirty pieces: stored ^= delta.
    size_t piece_index = 0;
    uint64_t run_start = 0;
    bool in_run = false;
    for (uint64_t off = 0; off <= n; ++piece_index) {
      const bool dirty = off < n && flags[piece_index] != 0;
      if (dirty && !in_run) run_start = off;
      if (!dirty && in_run) {
        const uint64_t run = off - run_start;
        for (const auto& [parity, sum] : {std::pair{p, sum_p}, std::pair{q, sum_q}}) {
          if (sum == nullptr) continue;
          const uint64_t at = parity.offset + pos + run_start;
          int status = bdev_read_sync(parity.bdev, at, nw, run);
          if (status != kIoOk) return status;
          for (uint64_t b = 0; b < run; ++b) nw[b] ^= sum[run_start + b];
          status = bdev_write_sync(parity.bdev, at, nw, run);
          if (status != kIoOk) return status;
        }
      }
      in_run = dirty;
      if (off == n) break;
      off += std::min<uint64_t>(granule - (pos + off) % granule, n - off);
    }
  }
  return kIoOk;
}

void fill_stats(const std::vector<uint64_t>& words, uint64_t n_granules,
                uint32_t max_report, DiffStats* stats) {
  stats->granules = n_granules;
  stats->mismatched = 0;
  stats->first_mismatches.clear();
  for (uint64_t w = 0; w < words.size(); ++w) {
    uint64_t word = words[w];
    stats->mismatched += static_cast<uint64_t>(__builtin_popcountll(word));
    while (word != 0 && stats->first_mismatches.size() < max_report) {
      stats->first_mismatches.push_back(
          w * 64 + static_cast<uint64_t>(__builtin_ctzll(word)));
      word &= word - 1;
    }
  }
}

// Encode after validation; also the last step of a rebuild that lost
// parity.
int encode_validated(const std::vector<ParityMember>& data,
                     const std::vector<ParityMember>& all, ParityMember p,
                     ParityMember q, uint64_t length, ParityReport* report) {
  Bdev* first_out = p.bdev != nullptr ? p.bdev : q.bdev;
  const int device = select_device(all, first_out);
  if (report != nullptr) report->on_gpu = device >= 0;
  const int status =
      device >= 0 ? parity_encode_gpu(device, device_set(data), device_ptr(p),
                                      device_ptr(q), length)
                  : encode_generic(data, p, q, length);
  return status == kIoOk ? kIoOk : fail(report, status, "I/O failed");
}

}  // namespace

// ---------------------------------------------------------------------------
// Public calls
// ---------------------------------------------------------------------------

uint64_t parity_common_length(const std::vector<ParityMember>& data,
                              ParityMember p, ParityMember q, uint64_t unit) {
  std::vector<ParityMember> all = data;
  all.push_back(p);
  all.push_back(q);
  uint64_t room = UINT64_MAX;
  for (const ParityMember& m : all) {
    if (m.bdev == nullptr) continue;
    if (m.offset > m.bdev->size_bytes()) return 0;
    room = std::min(room, m.bdev->size_bytes() - m.offset);
  }
  if (room == UINT64_MAX || unit == 0) return 0;
  return room / unit * unit;
}

int bdev_parity_encode_sync(const std::vector<ParityMember>& data,
                            ParityMember p, ParityMember q, uint64_t length,
                            ParityReport* report) {
  try {
    std::vector<ParityMember> all;
    const int status = validate_set(data, p, q, length, &all, report);
    if (status != kIoOk) return status;
    if ((p.bdev != nullptr && p.bdev->claimed()) ||
        (q.bdev != nullptr && q.bdev->claimed())) {
      return fail(report, kIoFailed,
                  "a parity bdev is claimed; encode runs offline only");
    }
    return encode_validated(data, all, p, q, length, report);
  } catch (const std::exception&) {
    return fail(report, kIoFailed, "I/O failed");
  }
}

int bdev_parity_check_sync(const std::vector<ParityMember>& data,
                           ParityMember p, ParityMember q, uint64_t length,
                           uint32_t granule, uint32_t max_report,
                           ParityCheck* out, ParityReport* report) {
  try {
    std::vector<ParityMember> all;
    int status = validate_set(data, p, q, length, &all, report);
    if (status != kIoOk) return status;
    if (out == nullptr) return fail(report, kIoInvalid, "no result to fill");
    status = validate_granule(all[0].bdev->block_size(), length, granule,
                              report);
    if (status != kIoOk) return status;
    const uint64_t n_granules = length / granule;
    *out = ParityCheck{};
    Bdev* first = p.bdev != nullptr ? p.bdev : q.bdev;
    const int device = select_device(all, first);
    if (report != nullptr) report->on_gpu = device >= 0;
    status = device >= 0
                 ? parity_check_gpu(device, device_set(data), device_ptr(p),
                                    device_ptr(q), n_granules, granule,
                                    &out->p_bitmap, &out->q_bitmap)
                 : check_generic(data, p, q, length, granule, &out->p_bitmap,
                                 &out->q_bitmap);
    if (status != kIoOk) return fail(report, status, "I/O failed");
    if (p.bdev != nullptr) {
      fill_stats(out->p_bitmap, n_granules, max_report, &out->p);
    }
    if (q.bdev != nullptr) {
      fill_stats(out->q_bitmap, n_granules, max_report, &out->q);
    }
    return kIoOk;
  } catch (const std::exception&) {
    return fail(report, kIoFailed, "I/O failed");
  }
}

int bdev_parity_rebuild_sync(const std::vector<ParityMember>& data,
                             ParityMember p, ParityMember q, uint64_t length,
                             const std::vector<int>& lost,
                             ParityReport* report) {
  try {
    std::vector<ParityMember> all;
    int status = validate_set(data, p, q, length, &all, report);
    if (status != kIoOk) return status;
    if (lost.empty() || lost.size() > 2) {
      return fail(report, kIoInvalid, "one or two lost members are needed");
    }
    if (lost.size() == 2 && lost[0] == lost[1]) {
      return fail(report, kIoInvalid, "duplicate entry in lost");
    }
    bool lost_p = false;
    bool lost_q = false;
    std::vector<uint32_t> lost_data;
    for (int entry : lost) {
      if (entry == kParityLostP) {
        lost_p = true;
      } else if (entry == kParityLostQ) {
        lost_q = true;
      } else if (entry >= 0 && static_cast<size_t>(entry) < data.size()) {
        lost_data.push_back(static_cast<uint32_t>(entry));
      } else {
        return fail(report, kIoInvalid, "lost index is not below k");
      }
    }
    if ((lost_p && p.bdev == nullptr) || (lost_q && q.bdev == nullptr)) {
      return fail(report, kIoInvalid, "a lost parity must be given");
    }
    std::sort(lost_data.begin(), lost_data.end());
    const bool use_p = p.bdev != nullptr && !lost_p;
    const bool use_q = q.bdev != nullptr && !lost_q;
    if (lost_data.size() > static_cast<size_t>(use_p) + use_q) {
      return fail(report, kIoInvalid,
                  "the remaining parity cannot cover this loss (a lost data "
                  "member needs p or q, two need both)");
    }
    std::vector<Bdev*> targets;
    for (uint32_t x : lost_data) targets.push_back(data[x].bdev);
    if (lost_p) targets.push_back(p.bdev);
    if (lost_q) targets.push_back(q.bdev);
    for (Bdev* t : targets) {
      if (t->claimed()) {
        return fail(report, kIoFailed,
                    "a target bdev is claimed; rebuild runs offline only");
      }
    }

    if (!lost_data.empty()) {
      ParityCoeffs coeffs;
      ParityMember out_a = data[lost_data[0]];
      ParityMember out_b;
      if (lost_data.size() == 2) {
        coeffs = parity_coeffs_two(lost_data[0], lost_data[1]);
        out_b = data[lost_data[1]];
      } else if (use_p) {
        coeffs = ParityCoeffs{1, 0};
      } else {
        coeffs = parity_coeffs_one_by_q(lost_data[0]);
      }
      std::vector<ParityMember> survivors = data;
      for (uint32_t x : lost_data) survivors[x] = ParityMember{};
      const ParityMember rp = coeffs.a != 0 ? p : ParityMember{};
      const ParityMember rq = coeffs.b != 0 ? q : ParityMember{};
      // Parity that is lost too, or not needed, is not read and does not
      // decide the path.
      std::vector<ParityMember> touched;
      for (const ParityMember& m : data) touched.push_back(m);
      if (rp.bdev != nullptr) touched.push_back(rp);
      if (rq.bdev != nullptr) touched.push_back(rq);
      const int device = select_device(touched, out_a.bdev);
      if (report != nullptr) report->on_gpu = device >= 0;
      status = device >= 0
                   ? parity_rebuild_gpu(device, device_set(survivors),
                                        device_ptr(rp), device_ptr(rq), coeffs,
                                        device_ptr(out_a), device_ptr(out_b),
                                        length)
                   : rebuild_generic(survivors, rp, rq, coeffs, out_a, out_b,
                                     length);
      if (status != kIoOk) return fail(report, status, "I/O failed");
    }
    if (lost_p || lost_q) {
      const ParityMember wp = lost_p ? p : ParityMember{};
      const ParityMember wq = lost_q ? q : ParityMember{};
      std::vector<ParityMember> touched = data;
      if (wp.bdev != nullptr) touched.push_back(wp);
      if (wq.bdev != nullptr) touched.push_back(wq);
      return encode_validated(data, touched, wp, wq, length, report);
    }
    return kIoOk;
  } catch (const std::exception&) {
    return fail(report, kIoFailed, "I/O failed");
  }
}

int bdev_parity_update_sync(const std::vector<ParityMember>& data,
                            ParityMember p, ParityMember q,
                            const std::vector<ParityMember>& bases,
                            uint64_t length, uint32_t granule,
                            uint32_t max_report, bool refresh,
                            DiffStats* changed, std::vector<uint64_t>* bitmap,
                            ParityReport* report) {
  try {
    std::vector<ParityMember> all;
    int status = validate_set(data, p, q, length, &all, report);
    if (status != kIoOk) return status;
    if (changed == nullptr || bitmap == nullptr) {
      return fail(report, kIoInvalid, "no result to fill");
    }
    if (bases.size() != data.size()) {
      return fail(report, kIoInvalid, "one base slot per data member is needed");
    }
    const uint64_t bs = all[0].bdev->block_size();
    std::vector<ParityMember> tracked;
    for (const ParityMember& b : bases) {
      if (b.bdev == nullptr) continue;
      if (b.bdev->block_size() != bs) {
        return fail(report, kIoInvalid,
                    "a base does not have the set's block size");
      }
      if (b.offset % bs != 0) {
        return fail(report, kIoInvalid,
                    "offsets must be multiples of the block size");
      }
      const uint64_t size = b.bdev->size_bytes();
      if (length > size || b.offset > size - length) {
        return fail(report, kIoInvalid, "base range out of bounds");
      }
      for (const ParityMember& m : all) {
        if (same_store(b.bdev, m.bdev)) {
          return fail(report, kIoInvalid,
                      "a base shares a bdev or backing store with a member");
        }
      }
      for (const ParityMember& other : tracked) {
        if (same_store(b.bdev, other.bdev)) {
          return fail(report, kIoInvalid,
                      "two bases share a bdev or backing store");
        }
      }
      tracked.push_back(b);
    }
    if (tracked.empty()) {
      return fail(report, kIoInvalid, "no base given: nothing is tracked");
    }
    status = validate_granule(bs, length, granule, report);
    if (status != kIoOk) return status;
    if ((p.bdev != nullptr && p.bdev->claimed()) ||
        (q.bdev != nullptr && q.bdev->claimed())) {
      return fail(report, kIoFailed,
                  "a parity bdev is claimed; update runs offline only");
    }
    if (refresh) {
      for (const ParityMember& b : tracked) {
        if (b.bdev->claimed()) {
          return fail(report, kIoFailed,
                      "a base bdev is claimed; refresh runs offline only");
        }
      }
    }
    const uint64_t n_granules = length / granule;
    *changed = DiffStats{};
    bitmap->clear();
    std::vector<ParityMember> touched = all;
    touched.insert(touched.end(), tracked.begin(), tracked.end());
    Bdev* first = p.bdev != nullptr ? p.bdev : q.bdev;
    const int device = select_device(touched, first);
    if (report != nullptr) report->on_gpu = device >= 0;
    status = device >= 0
                 ? parity_update_gpu(device, device_set(data), device_set(bases),
                                     device_ptr(p), device_ptr(q), n_granules,
                                     granule, refresh, bitmap)
                 : update_generic(data, p, q, bases, length, granule, refresh,
                                  bitmap);
    if (status != kIoOk) return fail(report, status, "I/O failed");
    fill_stats(*bitmap, n_granules, max_report, changed);
    return kIoOk;
  } catch (const std::exception&) {
    return fail(report, kIoFailed, "I/O failed");
  }
}

}  // namespace hipstore
