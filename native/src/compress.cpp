// The HSLZ1 and HSLZD1 granule codecs on the host (hipstore/compress.h):
// the normative parse, byte for byte what k_lz_compress_marked<false> and
// k_lz_compress_marked<true> emit, the validator and the decoder. Plain host
// code; the marked calls and the kernels are in compress_ops.hip.

#include "hipstore/compress.h"

#include <string.h>

#include <vector>

namespace hipstore {

namespace {

uint32_t load_u32(const uint8_t* p) {
  return static_cast<uint32_t>(p[0]) | static_cast<uint32_t>(p[1]) << 8 |
         static_cast<uint32_t>(p[2]) << 16 | static_cast<uint32_t>(p[3]) << 24;
}

uint32_t lz_hash(uint32_t v) { return (v * kLzHashMul) >> (32 - kLzHashBits); }

// Extension bytes of a length whose nibble is 15.
uint32_t ext_bytes(uint32_t len) { return len >= 15 ? 1 + (len - 15) / 255 : 0; }

uint8_t* put_ext(uint8_t* o, uint32_t len) {
  if (len < 15) return o;
  len -= 15;
  for (; len >= 255; len -= 255) *o++ = 255;
  *o++ = static_cast<uint8_t>(len);
  return o;
}

bool refuse(std::string* why, const char* what) {
  if (why != nullptr) *why = what;
  return false;
}

// One token walk for the validator (out == nullptr) and the decoder.
// `history` is what lies before the granule: 0 for HSLZ1, the granule
// size for HSLZD1, whose decoder reads those bytes from `dict`.
bool lz_walk(const uint8_t* piece, uint64_t size, uint32_t granule,
             uint64_t history, const uint8_t* dict, uint8_t* out,
             std::string* why) {
  if (!lz_granule_ok(granule)) return refuse(why, "unsupported granule");
  if (size == 0 || size > granule) return refuse(why, "stored size out of range");
  if (size == granule) {
    if (out != nullptr) memcpy(out, piece, granule);
    return true;
  }
  uint64_t ip = 0;
  uint64_t op = 0;
  // A length: the nibble, then bytes up to and including the first that
  // is not 255. false when the piece ends inside it.
  auto length = [&](uint64_t nibble, uint64_t* len) {
    *len = nibble;
    if (nibble != 15) return true;
    for (;;) {
      if (ip >= size) return false;
      const uint8_t b = piece[ip++];
      *len += b;
      if (b != 255) return true;
    }
  };
  for (;;) {
    if (ip >= size) return refuse(why, "piece ends before its last literals");
    const uint8_t token = piece[ip++];
    uint64_t lit = 0;
    if (!length(token >> 4, &lit)) return refuse(why, "truncated literal length");
    if (lit > size - ip) return refuse(why, "literal run overruns the piece");
    if (lit > granule - op) return refuse(why, "literal run overruns the granule");
    if (out != nullptr) memcpy(out + op, piece + ip, lit);
    ip += lit;
    op += lit;
    if (ip == size) {
      if (op != granule) return refuse(why, "output shorter than the granule");
      if (lit < 5) return refuse(why, "fewer than 5 final literals");
      return true;
    }
    if (size - ip < 2) return refuse(why, "truncated offset");
    const uint64_t offset = piece[ip] | static_cast<uint64_t>(piece[ip + 1]) << 8;
    ip += 2;
    if (offset == 0) return refuse(why, "offset 0");
    if (offset > history + op) {
      return refuse(why, history != 0 ? "offset past the start of the dictionary"
                                      : "offset past the start of the granule");
    }
    uint64_t len = 0;
    if (!length(token & 15, &len)) return refuse(why, "truncated match length");
    len += 4;
    if (op > granule - 12) return refuse(why, "match starts after granule - 12");
    if (len > granule - 5 - op) return refuse(why, "match overruns granule - 5");
    if (out != nullptr) {
      for (uint64_t i = 0; i < len; ++i) {
        const uint64_t at = history + op + i - offset;  // in dict || out
        out[op + i] = at >= history ? out[at - history] : dict[at];
      }
    }
    op += len;
  }
}

// The parse of compress.h over image[0, start + granule): the granule is
// image[start, start + granule), what lies before it is history that
// `table` (position + 1, 0 = empty) already holds. `aligned` adds
// HSLZD1's candidate q - granule.
uint32_t lz_parse(const uint8_t* image, uint32_t start, uint32_t granule,
                  bool aligned, uint32_t* table, uint8_t* out) {
  const uint32_t end = start + granule;
  const uint32_t last = end - 12;  // last position a match may start at
  uint32_t anchor = start;
  uint32_t op = 0;
  // Literals [anchor, anchor + lit), then a match unless len == 0.
  // false: the block would not be smaller than the granule.
  auto emit = [&](uint32_t lit, uint32_t offset, uint32_t len) {
    const uint32_t ml = len != 0 ? len - 4 : 0;
    const uint32_t need = 1 + ext_bytes(lit) + lit +
                          (len != 0 ? 2 + ext_bytes(ml) : 0);
    if (op + need >= granule) return false;
    uint8_t* o = out + op;
    *o++ = static_cast<uint8_t>((lit < 15 ? lit : 15) << 4 | (ml < 15 ? ml : 15));
    o = put_ext(o, lit);
    memcpy(o, image + anchor, lit);
    o += lit;
    if (len != 0) {
      *o++ = static_cast<uint8_t>(offset);
      *o++ = static_cast<uint8_t>(offset >> 8);
      o = put_ext(o, ml);
    }
    op += need;
    return true;
  };
  bool fits = true;
  for (uint32_t p = start; fits && p <= last;) {
    const uint32_t lanes = last - p + 1 < kLzWindow ? last - p + 1 : kLzWindow;
    uint32_t winner = lanes;
    uint32_t cand = 0;
    for (uint32_t l = 0; l < lanes && winner == lanes; ++l) {
      const uint32_t q = p + l;
      const uint32_t v = load_u32(image + q);
      const uint32_t slot = table[lz_hash(v)];
      if (aligned && load_u32(image + q - granule) == v) {
        winner = l;
        cand = q - granule;
      } else if (slot != 0 && load_u32(image + slot - 1) == v) {
        winner = l;
        cand = slot - 1;
      }
    }
    // Ascending, so a slot ends up with the greatest position.
    for (uint32_t l = 0; l < lanes && l <= winner; ++l) {
      table[lz_hash(load_u32(image + p + l))] = p + l + 1;
    }
    if (winner == lanes) {
      p += kLzWindow;
      continue;
    }
    const uint32_t q = p + winner;
    uint32_t len = 4;
    while (q + len < end - 5 && image[cand + len] == image[q + len]) ++len;
    fits = emit(q - anchor, q - cand, len);
    anchor = p = q + len;
  }
  if (fits) fits = emit(end - anchor, 0, 0);
  if (!fits) {
    memcpy(out, image + start, granule);
    return granule;
  }
  return op;
}

}  // namespace

uint32_t lz_compress_granule(const uint8_t* in, uint32_t granule,
                             uint8_t* out) {
  uint32_t table[1u << kLzHashBits] = {0};
  return lz_parse(in, 0, granule, false, table, out);
}

uint32_t lz_dict_compress_granule(const uint8_t* in, const uint8_t* dict,
                                  uint32_t granule, uint8_t* out) {
  std::vector<uint8_t> image(2 * static_cast<size_t>(granule));
  memcpy(image.data(), dict, granule);
  memcpy(image.data() + granule, in, granule);
  uint32_t table[1u << kLzHashBits] = {0};
  // Ascending, so a slot ends up with the greatest position.
  for (uint32_t q = 0; q < granule; ++q) {
    table[lz_hash(load_u32(image.data() + q))] = q + 1;
  }
  return lz_parse(image.data(), granule, granule, true, table, out);
}

bool lz_validate_granule(const uint8_t* piece, uint64_t size, uint32_t granule,
                         std::string* why) {
  return lz_walk(piece, size, granule, 0, nullptr, nullptr, why);
}

bool lz_decompress_granule(const uint8_t* piece, uint64_t size,
                           uint32_t granule, uint8_t* out, std::string* why) {
  return lz_walk(piece, size, granule, 0, nullptr, out, why);
}

bool lz_dict_validate_granule(const uint8_t* piece, uint64_t size,
                              uint32_t granule, std::string* why) {
  return lz_walk(piece, size, granule, granule, nullptr, nullptr, why);
}

bool lz_dict_decompress_granule(const uint8_t* piece, uint64_t size,
                                uint32_t granule, const uint8_t* dict,
                                uint8_t* out, std::string* why) {
  return lz_walk(piece, size, granule, granule, dict, out, why);
}

}  // namespace hipstore
