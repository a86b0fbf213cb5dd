// MI355X (gfx950) HSLZ1 compression of marked granules (definitions and
// the normative parse in hipstore/compress.h): k_lz_compress_marked,
// k_gather_var and k_lz_decompress_marked, their window loops and the
// generic path. Like bulk_ops.hip, each call owns its stream, runs to
// completion and returns.
//
// Work split: a wave takes one whole granule at a time and waves
// grid-stride over the granules of the window's bitmap words (at most
// 2048 workgroups), so the bit test and the whole parse are wave-uniform
// and waves never wait for each other: there is no workgroup barrier in
// this file. The slot of a granule comes from the bitmap and
// rank_before_word exactly as in k_pack_marked.
//
// Data movement, compress: HBM -> LDS (16 B per lane) -> parse in LDS ->
// block built in LDS -> HBM scratch slot `rank` (16 B per lane), stored
// size -> pinned sizes[rank]. The host turns a window's sizes into
// 16-byte-aligned offsets and k_gather_var moves only the stored bytes
// over PCIe into the pinned dense buffer. Decompress is the way back:
// pinned dense -> LDS piece -> LDS granule image -> HBM.
//
// LDS per wave: compress 2 * G + 8 KiB (granule, block, 2048 u32 table
// slots), decompress 2 * G (piece, image). A workgroup has the 4, 2 or 1
// waves that fit 64 KiB: compress 4 waves up to G = 4096 (64 KiB at
// 4096), 2 up to 12288, 1 above; decompress 4 up to 8192, 2 above.
//
// HSLZD1 (the kDict instantiations of the two kernels): the same split
// and movement with the base granule as dictionary. Compress holds the
// image D || X, the block and the table, 3 * G + 8 KiB per wave: D comes
// from the base volume, the table is seeded from it, and the scan runs
// over X with an aligned candidate that needs no table. Decompress holds
// the piece and the image, 3 * G: it reads its target granule as D,
// decodes behind it and only then overwrites the granule. A workgroup has
// as many waves, 1 .. 4, as fit 64 KiB: compress 4 up to G = 2720, 3 up
// to 4544, 2 up to 8192, 1 above; decompress 4 up to 5456, 3 up to 7280,
// 2 up to 10912, 1 above.
//
// Keyed calls (compress.h): k_xts_var (crypt_ops.hip) replaces
// k_gather_var, scratch slot -> registers -> ciphertext in pinned dense,
// and on the way back turns pinned ciphertext into plaintext pieces in
// device scratch, which the decode kernels then read in place of the
// dense buffer, in strict mode (lz_decode): the host never sees a
// plaintext piece, so the kernel's checks are the validation.

#include <hip/hip_runtime.h>

#include <string.h>

#include <algorithm>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "crypt_internal.h"
#include "gpu_internal.h"
#include "hipstore/compress.h"
#include "hipstore/crypt.h"
#include "hipstore/engine.h"
#include "marked_internal.h"

namespace hipstore {

namespace {

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

constexpr uint32_t kLzTableBytes = (1u << kLzHashBits) * 4;
constexpr uint32_t kLzMaxLds = 64u << 10;  // per workgroup

// Orders this wave's LDS accesses: what one lane wrote before it, any
// lane reads after it. LDS serves a wave's accesses in issue order, so
// this only has to keep the compiler from moving them.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Little-endian u32 at byte `q` of an LDS image, q + 8 <= its size:
// two aligned words and a funnel shift.
__device__ __forceinline__ uint32_t lds_u32(const uint32_t* img, uint32_t q) {
  const uint64_t pair =
      static_cast<uint64_t>(img[(q >> 2) + 1]) << 32 | img[q >> 2];
  return static_cast<uint32_t>(pair >> ((q & 3) * 8));
}

__device__ __forceinline__ uint32_t lz_ext_bytes(uint32_t len) {
  return len >= 15 ? 1 + (len - 15) / 255 : 0;
}

// The extension bytes of `len` at out[o]: the 255s by all lanes, the
// last byte by lane 0. Returns the position after them.
__device__ __forceinline__ uint32_t lz_put_ext(uint8_t* out, uint32_t o,
                                               uint32_t len, uint32_t lane) {
  if (len < 15) return o;
  const uint32_t n = (len - 15) / 255;
  for (uint32_t i = lane; i < n; i += 64) out[o + i] = 255;
  if (lane == 0) out[o + n] = static_cast<uint8_t>(len - 15 - n * 255);
  return o + n + 1;
}

// One sequence at out[op]: token and lengths by lane 0, literals
// in[anchor, anchor + lit) by all lanes, then the match unless len == 0.
// false, with nothing written, when the block would not stay below G.
__device__ __forceinline__ bool lz_emit(const uint8_t* in, uint8_t* out,
                                        uint32_t& op, uint32_t anchor,
                                        uint32_t lit, uint32_t offset,
                                        uint32_t len, uint32_t granule,
                                        uint32_t lane) {
  const uint32_t ml = len != 0 ? len - 4 : 0;
  const uint32_t need =
      1 + lz_ext_bytes(lit) + lit + (len != 0 ? 2 + lz_ext_bytes(ml) : 0);
  if (op + need >= granule) return false;
  uint32_t o = op;
  if (lane == 0) {
    out[o] = static_cast<uint8_t>(min(lit, 15u) << 4 | min(ml, 15u));
  }
  o = lz_put_ext(out, o + 1, lit, lane);
  for (uint32_t i = lane; i < lit; i += 64) out[o + i] = in[anchor + i];
  o += lit;
  if (len != 0) {
    if (lane == 0) {
      out[o] = static_cast<uint8_t>(offset);
      out[o + 1] = static_cast<uint8_t>(offset >> 8);
    }
    o = lz_put_ext(out, o + 2, ml, lane);
  }
  op = o;
  return true;
}

// The parse of compress.h over the LDS image `in`; the block goes to
// `out`. Returns the stored size, `granule` for raw. Everything but the
// per-lane candidate test is wave-uniform. kDict is HSLZD1: `in` is
// D || X, `table` holds the positions of D, the scan starts at G and a
// lane first tries its aligned position q - G, which needs no table.
template <bool kDict>
__device__ __forceinline__ uint32_t lz_parse(const uint8_t* in, uint8_t* out,
                                             uint32_t* table, uint32_t granule,
                                             uint32_t lane) {
  const uint32_t* in32 = reinterpret_cast<const uint32_t*>(in);
  const uint32_t start = kDict ? granule : 0;
  const uint32_t end = start + granule;
  const uint32_t last = end - 12;
  uint32_t anchor = start;
  uint32_t op = 0;
  uint32_t p = start;
  while (p <= last) {
    const uint32_t q = p + lane;
    const bool live = q <= last;
    uint32_t hash = 0;
    uint32_t cand = 0;
    bool hit = false;
    if (live) {
      const uint32_t v = lds_u32(in32, q);
      hash = (v * kLzHashMul) >> (32 - kLzHashBits);
      const uint32_t slot = table[hash];  // position + 1, 0 = empty
      if (kDict && lds_u32(in32, q - granule) == v) {
        cand = q - granule;
        hit = true;
      } else if (slot != 0) {
        cand = slot - 1;
        hit = lds_u32(in32, cand) == v;
      }
    }
    const unsigned long long hits = __ballot(hit);
    const uint32_t winner =
        hits != 0 ? static_cast<uint32_t>(__builtin_ctzll(hits)) : 64;
    wave_sync();  // every candidate was read before any insert
    if (live && lane <= winner) atomicMax(&table[hash], q + 1);
    wave_sync();
    if (hits == 0) {
      p += kLzWindow;
      continue;
    }
    const uint32_t wq = p + winner;
    const uint32_t wc = static_cast<uint32_t>(
        __shfl(static_cast<int>(cand), static_cast<int>(winner)));
    // 64 bytes per step; the first lane that must stop ends the match.
    const uint32_t cap = end - 5 - wq;  // >= 7: wq <= end - 12
    uint32_t len = 4;
    for (;;) {
      const uint32_t i = len + lane;
      const bool stop = i >= cap || in[wc + i] != in[wq + i];
      const unsigned long long stops = __ballot(stop);
      if (stops != 0) {
        len += static_cast<uint32_t>(__builtin_ctzll(stops));
        break;
      }
      len += 64;
    }
    if (!lz_emit(in, out, op, anchor, wq - anchor, wq - wc, len, granule,
                 lane)) {
      return granule;
    }
    anchor = p = wq + len;
  }
  if (!lz_emit(in, out, op, anchor, end - anchor, 0, 0, granule, lane)) {
    return granule;
  }
  return op;
}

// Scratch slot `slot` (stride G) receives the piece, its pad up to the
// next multiple of 16 zeroed, and sizes[slot] its stored size: plain
// loads and stores, no global atomics, nothing read that an earlier
// launch left in scratch or sizes. Per-wave LDS: the granule X (G), the
// block (G) and the table.
//
// kDict is HSLZD1: granule g of `base` is the dictionary D of granule g
// of `src` (`base` is not read without it). The per-wave LDS then begins
// with D, the image D || X (2G, D immediately before X, so a u32 that
// straddles the boundary and a match that runs from D into X are plain
// addressing), and the cleared table is seeded with the positions of D in
// rows of 64: atomicMax of position + 1 leaves the greatest position in a
// slot whatever the order.
template <bool kDict>
__global__ __launch_bounds__(kWavesPerWg * 64) void k_lz_compress_marked(
    const uint8_t* __restrict__ src, const uint8_t* __restrict__ base,
    uint8_t* __restrict__ scratch, uint32_t* __restrict__ sizes,
    const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule) {
  extern __shared__ uint4 lz_lds[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule >> 4;
  uint8_t* image = reinterpret_cast<uint8_t*>(lz_lds) +
                   (threadIdx.x >> 6) *
                       ((kDict ? 3 : 2) * granule + kLzTableBytes);
  uint8_t* out = image + (kDict ? 2 : 1) * granule;
  uint32_t* table = reinterpret_cast<uint32_t*>(out + granule);
  wave_window_walk(bitmap, rank_before_word, win, [&](uint64_t g,
                                                      uint32_t slot) {
    const uint4* __restrict__ pd =
        kDict ? reinterpret_cast<const uint4*>(base + g * granule) : nullptr;
    const uint4* __restrict__ px =
        reinterpret_cast<const uint4*>(src + g * granule);
    uint4* image16 = reinterpret_cast<uint4*>(image);
    uint4* x16 = image16 + (kDict ? n16 : 0);
    uint4* table16 = reinterpret_cast<uint4*>(table);
#pragma unroll 4
    for (uint32_t i = lane; i < n16; i += 64) {
      if (kDict) image16[i] = pd[i];
      x16[i] = px[i];
    }
    for (uint32_t i = lane; i < kLzTableBytes / 16; i += 64) {
      table16[i] = make_uint4(0, 0, 0, 0);
    }
    wave_sync();
    if (kDict) {
      const uint32_t* image32 = reinterpret_cast<const uint32_t*>(image);
      for (uint32_t q = lane; q < granule; q += 64) {  // q + 8 <= 2G
        const uint32_t v = lds_u32(image32, q);
        atomicMax(&table[(v * kLzHashMul) >> (32 - kLzHashBits)], q + 1);
      }
      wave_sync();
    }
    const uint32_t size = lz_parse<kDict>(image, out, table, granule, lane);
    // size < granule and granule % 16 == 0: the pad stays inside `out`.
    if (size != granule && lane < ((16 - (size & 15)) & 15)) {
      out[size + lane] = 0;
    }
    wave_sync();
    const uint4* from =
        size == granule ? x16 : reinterpret_cast<const uint4*>(out);
    uint4* __restrict__ ps = reinterpret_cast<uint4*>(
        scratch + static_cast<uint64_t>(slot) * granule);
    for (uint32_t i = lane; i < (size + 15) >> 4; i += 64) ps[i] = from[i];
    if (lane == 0) sizes[slot] = size;
    wave_sync();  // the next granule overwrites this LDS
  });
}

// Piece r of a window, padded to 16 bytes, from scratch slot r to
// dense + offsets[r]: wave per piece, 16 bytes per lane. The pad bytes
// are the zeros k_lz_compress_marked left behind the piece. A size above
// G cannot come from that kernel and is cut to G, so no access leaves
// the slot.
__global__ __launch_bounds__(kWavesPerWg * 64) void k_gather_var(
    const uint8_t* __restrict__ scratch, uint8_t* __restrict__ dense,
    const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
    uint32_t count, uint32_t granule) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * kWavesPerWg + (threadIdx.x >> 6); r < count;
       r += gridDim.x * kWavesPerWg) {
    const uint32_t size = min(uniform(sizes[r]), granule);
    const uint4* __restrict__ ps = reinterpret_cast<const uint4*>(
        scratch + static_cast<uint64_t>(r) * granule);
    uint4* __restrict__ pd = reinterpret_cast<uint4*>(dense + offsets[r]);
    for (uint32_t i = lane; i < (size + 15) >> 4; i += 64) pd[i] = ps[i];
  }
}

// One byte of the piece, the same for every lane.
__device__ __forceinline__ uint32_t lz_byte(const uint8_t* piece, uint32_t ip) {
  return uniform(piece[ip]);
}

// The rest of a length whose nibble was 15. false when the piece ends
// inside it.
__device__ __forceinline__ bool lz_take_ext(const uint8_t* piece,
                                            uint32_t size, uint32_t& ip,
                                            uint32_t& len) {
  for (;;) {
    if (ip >= size) return false;
    const uint32_t b = lz_byte(piece, ip++);
    len += b;  // at most 255 * size
    if (b != 255) return true;
  }
}

// Decodes piece[0, size), size < G, into image[start, end), end = start
// + G; image[0, start) is history that matches may reach into (HSLZD1's
// dictionary; start = 0 for HSLZ1). Every read of the piece is checked
// against `size`, every write of the image against `end` and every
// offset against op before it happens; a sequence that would leave any
// of them ends the decode with false. A match reads image[op - offset +
// (i mod offset)], which lies below op for every i: correct down to
// offset 1 without any order among the lanes.
//
// kStrict adds the end-of-block rules of lz_validate_granule (at least 5
// final literals; no match starts after G - 12 or runs past G - 5), so
// that the decode accepts exactly the pieces the host validators accept:
// for the keyed calls, whose pieces the host sees only as ciphertext.
template <bool kStrict = false>
__device__ __forceinline__ bool lz_decode(const uint8_t* piece, uint32_t size,
                                          uint8_t* image, uint32_t start,
                                          uint32_t end, uint32_t lane) {
  uint32_t ip = 0;
  uint32_t op = start;
  for (;;) {
    if (ip >= size) return false;
    const uint32_t token = lz_byte(piece, ip++);
    uint32_t lit = token >> 4;
    if (lit == 15 && !lz_take_ext(piece, size, ip, lit)) return false;
    if (lit > size - ip || lit > end - op) return false;
    for (uint32_t i = lane; i < lit; i += 64) image[op + i] = piece[ip + i];
    ip += lit;
    op += lit;
    if (ip == size) return op == end && (!kStrict || lit >= 5);
    if (size - ip < 2) return false;
    const uint32_t offset = lz_byte(piece, ip) | lz_byte(piece, ip + 1) << 8;
    ip += 2;
    if (offset == 0 || offset > op) return false;
    uint32_t len = token & 15;
    if (len == 15 && !lz_take_ext(piece, size, ip, len)) return false;
    len += 4;
    if (len > end - op) return false;
    if (kStrict && (end - op < 12 || len > end - 5 - op)) return false;
    wave_sync();  // the literals above may be the match's source
    const uint32_t from = op - offset;
    const uint32_t step = 64 % offset;
    uint32_t r = lane % offset;
    for (uint32_t i = lane; i < len; i += 64) {
      image[op + i] = image[from + r];
      r += step;
      if (r >= offset) r -= offset;
    }
    wave_sync();
    op += len;
  }
}

// Window slot `slot` of the dense buffer (sizes[slot] bytes at
// offsets[slot]) becomes the marked granule of that rank; unmarked
// granules are never written. bad[slot] is written for every piece of
// the window: 0, or 1 when the piece could not be decoded, in which case
// its granule is left alone. Per-wave LDS: the piece (G) and the image
// (G). kStrict: lz_decode's; `dense` is then the device buffer k_xts_var
// decrypted the window into.
//
// kDict is HSLZD1: the dictionary of a piece is what its granule of `dst`
// holds now, and the image is 2G. The wave reads the granule into
// image[0, G), decodes into image[G, 2G) and only then writes the
// granule, so it reads its target before it overwrites it; it touches no
// other granule, so waves need no order. A raw piece is copied straight
// and reads nothing of `dst`.
template <bool kDict, bool kStrict>
__global__ __launch_bounds__(kWavesPerWg * 64) void k_lz_decompress_marked(
    uint8_t* dst, const uint8_t* __restrict__ dense,
    const uint32_t* __restrict__ sizes, const uint64_t* __restrict__ offsets,
    uint8_t* __restrict__ bad, const unsigned long long* __restrict__ bitmap,
    const uint32_t* __restrict__ rank_before_word, MarkedWindow win,
    uint32_t granule) {
  extern __shared__ uint4 lz_lds[];
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule >> 4;
  uint4* piece16 = lz_lds + (threadIdx.x >> 6) * ((kDict ? 3 : 2) * n16);
  uint4* image16 = piece16 + n16;
  uint4* x16 = image16 + (kDict ? n16 : 0);  // where the granule is decoded
  wave_window_walk(bitmap, rank_before_word, win, [&](uint64_t g,
                                                      uint32_t slot) {
    const uint32_t size = uniform(sizes[slot]);
    const uint4* __restrict__ pp =
        reinterpret_cast<const uint4*>(dense + offsets[slot]);
    uint4* pd = reinterpret_cast<uint4*>(dst + g * granule);
    bool ok = size != 0 && size <= granule;
    if (size == granule) {  // raw
#pragma unroll 4
      for (uint32_t i = lane; i < n16; i += 64) pd[i] = pp[i];
    } else if (ok) {
      for (uint32_t i = lane; i < (size + 15) >> 4; i += 64) piece16[i] = pp[i];
      if (kDict) {
#pragma unroll 4
        for (uint32_t i = lane; i < n16; i += 64) image16[i] = pd[i];
      }
      wave_sync();
      const uint32_t start = kDict ? granule : 0;
      ok = lz_decode<kStrict>(reinterpret_cast<const uint8_t*>(piece16), size,
                              reinterpret_cast<uint8_t*>(image16), start,
                              start + granule, lane);
      wave_sync();
      if (ok) {
#pragma unroll 4
        for (uint32_t i = lane; i < n16; i += 64) pd[i] = x16[i];
      }
      wave_sync();  // the next piece overwrites this LDS
    }
    if (lane == 0) bad[slot] = ok ? 0 : 1;
  });
}

// ---------------------------------------------------------------------------
// Window loops
// ---------------------------------------------------------------------------

// Waves per workgroup for `per_wave` bytes of LDS each.
uint32_t lz_waves(uint32_t per_wave) {
  return 4 * per_wave <= kLzMaxLds ? 4 : 2 * per_wave <= kLzMaxLds ? 2 : 1;
}

// The HSLZD1 kernels take as many waves, 1 .. 4, as fit.
uint32_t lzd_waves(uint32_t per_wave) {
  return std::min<uint32_t>(4, kLzMaxLds / per_wave);
}

// Device memory that grows on demand and keeps what it has, like
// PinnedBuf; one device at a time.
struct DeviceBuf {
  uint8_t* ptr = nullptr;
  uint64_t capacity = 0;
  int device = -1;

  DeviceBuf() = default;
  ~DeviceBuf() { release(); }
  DeviceBuf(const DeviceBuf&) = delete;
  DeviceBuf& operator=(const DeviceBuf&) = delete;

  void release() {
    if (ptr != nullptr) (void)hipFree(ptr);
    ptr = nullptr;
    capacity = 0;
  }
  // The current device is `dev`.
  uint8_t* reserve(int dev, uint64_t bytes) {
    if (dev != device || bytes > capacity) {
      release();
      HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ptr), bytes));
      capacity = bytes;
      device = dev;
    }
    return ptr;
  }
};

// Per-thread buffers of the two calls, two halves each on the GPU path.
struct CompressCtx {
  DeviceBuf scratch;            // slots of stride G
  PinnedBuf<uint8_t> dense;     // padded pieces
  PinnedBuf<uint32_t> sizes;
  PinnedBuf<uint64_t> offsets;  // of the pieces in `dense`
  PinnedBuf<uint8_t> bad;       // k_lz_decompress_marked's flags
};

CompressCtx& compress_ctx() {
  thread_local CompressCtx ctx;
  return ctx;
}

// Granule index of marked granule number `rank` (error messages).
uint64_t granule_of_rank(const std::vector<uint64_t>& bitmap, uint64_t rank) {
  for (uint64_t w = 0; w < bitmap.size(); ++w) {
    uint64_t word = bitmap[w];
    const uint64_t have = static_cast<uint64_t>(__builtin_popcountll(word));
    if (rank >= have) {
      rank -= have;
      continue;
    }
    for (; rank > 0; --rank) word &= word - 1;
    return w * 64 + static_cast<uint64_t>(__builtin_ctzll(word));
  }
  return bitmap.size() * 64;
}

// What a piece of `size` bytes takes of a window's dense stream. A keyed
// call stores at least one cipher block per piece (min_piece = 16).
uint64_t piece_room(uint32_t size, uint32_t min_piece) {
  return lz_padded(std::max(size, min_piece));
}

// Exclusive offsets of a window's padded pieces.
void piece_offsets(const uint32_t* sizes, uint64_t count, uint32_t min_piece,
                   uint64_t* offsets) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < count; ++i) {
    offsets[i] = at;
    at += piece_room(sizes[i], min_piece);
  }
}

// The key of a keyed call: both directions' schedules for the host codec.
// Null when the call has no key.
struct LzKey {
  const XtsSchedules* schedules = nullptr;
  uint64_t first_unit = 0;
  explicit operator bool() const { return schedules != nullptr; }
  uint32_t min_piece() const { return schedules != nullptr ? 16 : 1; }
};

bool size_ok(uint32_t size, uint32_t granule) {
  return size != 0 && size <= granule;
}

void name_bad_piece(const std::vector<uint64_t>& bitmap, uint64_t rank,
                    const std::string& why, std::string* error) {
  if (error != nullptr) {
    *error = "granule " + std::to_string(granule_of_rank(bitmap, rank)) +
             ": bad compressed piece (" + why + ")";
  }
}

// Sizes, then every piece, of one window as a source delivered it;
// fills `offsets`. kIoInvalid names the granule.
int check_window(const std::vector<uint64_t>& bitmap, const uint8_t* data,
                 const uint32_t* sizes, uint64_t first_rank, uint64_t count,
                 uint32_t granule, bool dictionary, uint32_t min_piece,
                 uint64_t* offsets, std::string* error) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < count; ++i) {
    std::string why = "stored size out of range";
    if (!size_ok(sizes[i], granule) ||
        !(dictionary
              ? lz_dict_validate_granule(data + at, sizes[i], granule, &why)
              : lz_validate_granule(data + at, sizes[i], granule, &why))) {
      name_bad_piece(bitmap, first_rank + i, why, error);
      return kIoInvalid;
    }
    offsets[i] = at;
    at += piece_room(sizes[i], min_piece);
  }
  return kIoOk;
}

// What the host can check of a keyed window, whose pieces are ciphertext:
// the sizes. Fills `offsets`.
int check_window_sizes(const std::vector<uint64_t>& bitmap,
                       const uint32_t* sizes, uint64_t first_rank,
                       uint64_t count, uint32_t granule, uint64_t* offsets,
                       std::string* error) {
  for (uint64_t i = 0; i < count; ++i) {
    if (!size_ok(sizes[i], granule)) {
      name_bad_piece(bitmap, first_rank + i, "stored size out of range", error);
      return kIoInvalid;
    }
  }
  piece_offsets(sizes, count, 16, offsets);
  return kIoOk;
}

// What both GPU window loops run on: the window stream, its staging the
// dense pieces, with the per-piece arrays. `done` events end a half's last
// kernel, `packed` ends k_lz_compress_marked alone. With `dictionary` the
// HSLZD1 kernels run: compress reads the dictionaries at `dict`,
// decompress takes them from the target itself.
struct LzStream : WindowStream {
  hipEvent_t packed[2] = {nullptr, nullptr};
  uint64_t chunk;  // granules per half
  uint8_t* scratch = nullptr;
  uint32_t* sizes;
  uint64_t* offsets;
  uint8_t* bad;
  bool dictionary;
  const uint8_t* dict;  // the base volume's range in device memory
  // A keyed call: k_xts_var encrypts the pieces on their way from scratch
  // to the dense halves and decrypts them on their way back into scratch,
  // where the strict decode kernels read them. The copy of the schedules
  // here is cleared with the object.
  bool keyed;
  uint64_t first_unit;
  XtsKernelKeys keys;

  LzStream(int device, Bdev* bdev, uint64_t offset, uint32_t granule_bytes,
           const MarkedPlan& plan, bool compress, const LzKey& key,
           bool with_dictionary, const uint8_t* dict_range)
      : WindowStream(device, bdev, offset, granule_bytes, plan,
                     compress_ctx().dense),
        chunk(plan.chunk_granules),
        sizes(compress_ctx().sizes.reserve(2 * chunk)),
        offsets(compress_ctx().offsets.reserve(2 * chunk)),
        bad(compress_ctx().bad.reserve(2 * chunk)),
        dictionary(with_dictionary), dict(dict_range),
        keyed(static_cast<bool>(key)), first_unit(key.first_unit) {
    if (keyed) xts_load_kernel_keys(*key.schedules, compress, &keys);
    if (compress || keyed) {
      scratch = compress_ctx().scratch.reserve(device, 2 * half_bytes);
    }
    if (compress) {
      for (hipEvent_t& e : packed) {
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      }
    }
  }
  ~LzStream() {
    (void)hipStreamSynchronize(stream);
    for (hipEvent_t e : packed) {
      if (e != nullptr) (void)hipEventDestroy(e);
    }
    explicit_bzero(&keys, sizeof(keys));
  }

  // Launch geometry: the waves that fit the LDS, each with `per_wave`
  // bytes of it. HSLZ1 takes 4, 2 or 1, HSLZD1 any of 1 .. 4.
  uint32_t waves(uint32_t per_wave) const {
    return dictionary ? lzd_waves(per_wave) : lz_waves(per_wave);
  }

  void compress(const MarkedWindow& win, int half) {
    const uint32_t per_wave = (dictionary ? 3 : 2) * granule + kLzTableBytes;
    const uint32_t n = waves(per_wave);
    hipLaunchKernelGGL(dictionary ? k_lz_compress_marked<true>
                                  : k_lz_compress_marked<false>,
                       dim3(wave_window_grid(win, n)), dim3(n * 64),
                       n * per_wave, stream, base, dict,
                       scratch + half * half_bytes,
                       device_view(sizes + half * chunk), dev_words, dev_ranks,
                       win, granule);
    record(packed[half]);
  }

  // After packed[half]: the sizes are in, the pieces follow.
  void gather(const MarkedWindow& win, int half) {
    piece_offsets(sizes + half * chunk, win.count, keyed ? 16 : 1,
                  offsets + half * chunk);
    if (keyed) {
      xts_var_launch(true, stream, scratch + half * half_bytes,
                     dev_staging + half * half_bytes,
                     device_view(sizes + half * chunk),
                     device_view(offsets + half * chunk), dev_words, dev_ranks,
                     win, granule, first_unit, keys);
    } else {
      const uint32_t grid = std::min<uint32_t>(
          (win.count + kWavesPerWg - 1) / kWavesPerWg, 2048);
      hipLaunchKernelGGL(k_gather_var, dim3(grid), dim3(kWavesPerWg * 64), 0,
                         stream, scratch + half * half_bytes,
                         dev_staging + half * half_bytes,
                         device_view(sizes + half * chunk),
                         device_view(offsets + half * chunk), win.count,
                         granule);
    }
    record(done[half]);
  }

  // Keyed: the window's sizes were checked (check_window_sizes), so the
  // pieces at their offsets stay inside a half of scratch.
  void decompress(const MarkedWindow& win, int half) {
    const uint32_t per_wave = (dictionary ? 3 : 2) * granule;
    const uint32_t n = waves(per_wave);
    const uint8_t* pieces = dev_staging + half * half_bytes;
    if (keyed) {
      uint8_t* plain = scratch + half * half_bytes;
      xts_var_launch(false, stream, pieces, plain,
                     device_view(sizes + half * chunk),
                     device_view(offsets + half * chunk), dev_words, dev_ranks,
                     win, granule, first_unit, keys);
      pieces = plain;
    }
    hipLaunchKernelGGL(dictionary
                           ? (keyed ? k_lz_decompress_marked<true, true>
                                    : k_lz_decompress_marked<true, false>)
                           : (keyed ? k_lz_decompress_marked<false, true>
                                    : k_lz_decompress_marked<false, false>),
                       dim3(wave_window_grid(win, n)), dim3(n * 64),
                       n * per_wave, stream, base, pieces,
                       device_view(sizes + half * chunk),
                       device_view(offsets + half * chunk),
                       device_view(bad + half * chunk), dev_words, dev_ranks,
                       win, granule);
    record(done[half]);
  }
};

// The shared pack loop with a window in two steps: once its sizes are in
// (packed), its pieces are gathered behind it. Window k+1 is compressed
// while the sink has window k: one stream, so the order on the device is
// compress k, gather k, compress k+1, ...
int compress_gpu(LzStream& ls, const MarkedPlan& plan, const CompressSink& sink,
                 uint64_t* packed) {
  return pack_windows(
      ls, plan,
      [&](const MarkedWindow& win, int half) { ls.compress(win, half); },
      [&](const MarkedWindow& win, int half) {
        wait_marked_event(ls.packed[half]);
        ls.gather(win, half);
      },
      [&](const MarkedWindow& win, int half) {
        return sink(ls.half_of(half), ls.sizes + half * ls.chunk,
                    win.first_rank, win.count);
      },
      packed);
}

// The shared unpack loop; a window is checked on the host before its
// launch, and the flags of a half's last kernel are read before the half
// is used again and, for the kernels still out at the end, after the loop.
int decompress_gpu(LzStream& ls, const MarkedPlan& plan,
                   const std::vector<uint64_t>& bitmap,
                   const DecompressSource& source, uint64_t* unpacked,
                   std::string* error) {
  uint32_t in_half[2] = {0, 0};  // pieces of the kernel that last used it
  uint64_t rank_of[2] = {0, 0};  // rank of the first of them
  // After that kernel: did it give up on a piece? On a keyed call the
  // strict decode is the validation, so that piece is a bad file and is
  // named as host validation names it; otherwise the host had accepted it.
  auto gave_up = [&](int half) {
    const uint8_t* bad = ls.bad + half * ls.chunk;
    const uint8_t* first = std::find_if(bad, bad + in_half[half],
                                        [](uint8_t b) { return b != 0; });
    if (first == bad + in_half[half]) return false;
    if (ls.keyed && (error == nullptr || error->empty())) {
      name_bad_piece(bitmap, rank_of[half] + static_cast<uint64_t>(first - bad),
                     "refused by the strict decoder", error);
    }
    return true;
  };
  const int gave_up_status = ls.keyed ? kIoInvalid : kIoFailed;
  int status = unpack_windows(
      ls, plan,
      [&](int half) -> int {
        const bool bad = gave_up(half);
        in_half[half] = 0;
        return bad ? gave_up_status : kIoOk;
      },
      [&](const MarkedWindow& win, int half) -> int {
        uint8_t* data = ls.half_of(half);
        uint32_t* sizes = ls.sizes + half * ls.chunk;
        const int got = source(data, sizes, win.first_rank, win.count);
        if (got != 0) return got;
        return ls.keyed
                   ? check_window_sizes(bitmap, sizes, win.first_rank,
                                        win.count, ls.granule,
                                        ls.offsets + half * ls.chunk, error)
                   : check_window(bitmap, data, sizes, win.first_rank,
                                  win.count, ls.granule, ls.dictionary, 1,
                                  ls.offsets + half * ls.chunk, error);
      },
      [&](const MarkedWindow& win, int half) {
        ls.decompress(win, half);
        in_half[half] = win.count;
        rank_of[half] = win.first_rank;
      },
      unpacked);
  // The older window first, so that the lowest bad granule is named.
  const int older = rank_of[0] <= rank_of[1] ? 0 : 1;
  if (gave_up(older) || gave_up(older ^ 1)) {
    if (status == kIoOk) status = gave_up_status;
    if (error != nullptr && error->empty()) {
      *error = ls.dictionary ? "k_lzd_decompress_marked gave up on a piece"
                             : "k_lz_decompress_marked gave up on a piece";
    }
  }
  return status;
}

// Generic paths: bdev_pack_marked_sync / bdev_unpack_marked_sync cut the
// chunks, the host codec does the rest. With `base` (HSLZD1) the
// dictionary of every granule is read from it, one granule (at most 16
// KiB) per read. With `key` every piece is one HSXTS2 unit
// (xts_encrypt_var / xts_decrypt_var) in the keyed layout.
int compress_generic(Bdev* src, uint64_t offset, Bdev* base,
                     uint64_t base_offset, uint64_t length, uint32_t granule,
                     const std::vector<uint64_t>& bitmap,
                     uint64_t staging_bytes, const CompressSink& sink,
                     const LzKey& key, uint64_t* packed) {
  std::vector<uint8_t> pieces;
  std::vector<uint32_t> sizes;
  std::vector<uint8_t> dict(base != nullptr ? granule : 0);
  MarkCursor marks{bitmap, length / granule};
  return bdev_pack_marked_sync(
      src, offset, length, granule, bitmap, staging_bytes,
      [&](const uint8_t* data, uint64_t first_rank, uint64_t count) {
        pieces.assign(count * granule, 0);  // pads are 0
        sizes.resize(count);
        uint64_t at = 0;
        for (uint64_t i = 0; i < count; ++i) {
          const uint64_t g = marks.next();
          uint8_t* piece = pieces.data() + at;
          if (base != nullptr) {
            const int status = bdev_read_sync(base, base_offset + g * granule,
                                              dict.data(), granule);
            if (status != kIoOk) return status;
            sizes[i] = lz_dict_compress_granule(data + i * granule, dict.data(),
                                                granule, piece);
          } else {
            sizes[i] = lz_compress_granule(data + i * granule, granule, piece);
          }
          if (key) {
            xts_encrypt_var(*key.schedules, key.first_unit + g, piece, piece,
                            std::max(sizes[i], 16u));
          }
          at += piece_room(sizes[i], key.min_piece());
        }
        return sink(pieces.data(), sizes.data(), first_rank, count);
      },
      packed);
}

int decompress_generic(Bdev* dst, uint64_t offset, uint64_t length,
                       uint32_t granule, const std::vector<uint64_t>& bitmap,
                       uint64_t staging_bytes,
                       const DecompressSource& source, bool dictionary,
                       const LzKey& key, uint64_t* unpacked,
                       std::string* error) {
  std::vector<uint8_t> pieces;
  std::vector<uint32_t> sizes;
  std::vector<uint64_t> offsets;
  std::vector<uint64_t> index;  // of each granule of the chunk
  std::vector<uint8_t> dict(dictionary ? granule : 0);
  MarkCursor marks{bitmap, length / granule};
  // A chunk is written after this returns, and no earlier chunk holds
  // its granules: what is read here is the target's state before the call.
  return bdev_unpack_marked_sync(
      dst, offset, length, granule, bitmap, staging_bytes,
      [&](uint8_t* data, uint64_t first_rank, uint64_t count) {
        pieces.resize(count * granule);
        sizes.resize(count);
        offsets.resize(count);
        index.resize(count);
        for (uint64_t& g : index) g = marks.next();
        int status = source(pieces.data(), sizes.data(), first_rank, count);
        if (status == 0 && key) {
          // Decrypted in place up to the first size that is out of range,
          // which check_window refuses before it looks at a piece.
          uint64_t at = 0;
          for (uint64_t i = 0; i < count && size_ok(sizes[i], granule); ++i) {
            xts_decrypt_var(*key.schedules, key.first_unit + index[i],
                            pieces.data() + at, pieces.data() + at,
                            std::max(sizes[i], 16u));
            at += piece_room(sizes[i], 16);
          }
        }
        if (status == 0) {
          status = check_window(bitmap, pieces.data(), sizes.data(), first_rank,
                                count, granule, dictionary, key.min_piece(),
                                offsets.data(), error);
        }
        for (uint64_t i = 0; status == kIoOk && i < count; ++i) {
          if (!dictionary) {
            lz_decompress_granule(pieces.data() + offsets[i], sizes[i], granule,
                                  data + i * granule);
            continue;
          }
          status = bdev_read_sync(dst, offset + index[i] * granule,
                                  dict.data(), granule);
          if (status == kIoOk) {
            lz_dict_decompress_granule(pieces.data() + offsets[i], sizes[i],
                                       granule, dict.data(),
                                       data + i * granule);
          }
        }
        return status;
      },
      unpacked);
}

// What is the codec's to check before the shared plan
// (plan_marked_windows): the granule, and a key (any of the two fields
// set), which must pass xts_key_ok and leave every unit number below
// 2^64-1.
int lz_plan(Bdev* bdev, uint64_t offset, uint64_t length, uint32_t granule,
            const std::vector<uint64_t>& bitmap, const LzOptions& options,
            bool have_callback, MarkedPlan* plan, std::string* error) {
  const XtsKey& key = options.key;
  if (!lz_granule_ok(granule)) {
    if (error != nullptr) {
      *error = "compression needs 512 <= granule <= 16384, a multiple of 16";
    }
    return kIoInvalid;
  }
  if ((key.key != nullptr || key.len != 0) && !xts_key_ok(key.key, key.len)) {
    if (error != nullptr) {
      *error = "the key must be 64 bytes whose halves differ";
    }
    return kIoInvalid;
  }
  if (key.key != nullptr && length / granule > kXtsKcvUnit - key.first_unit) {
    return kIoInvalid;
  }
  return plan_marked_windows(bdev, offset, length, granule, bitmap,
                             options.staging_bytes, have_callback, plan);
}

// The schedules of a call's key, if it has one, for as long as the call
// runs.
struct CallKey {
  std::unique_ptr<XtsSchedules> schedules;
  LzKey key;
  explicit CallKey(const XtsKey& raw) {
    if (raw.key == nullptr) return;
    schedules.reset(new XtsSchedules(raw.key));
    key = {schedules.get(), raw.first_unit};
  }
};

}  // namespace

int bdev_compress_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                              uint32_t granule,
                              const std::vector<uint64_t>& bitmap,
                              const LzOptions& options,
                              const CompressSink& sink, uint64_t* packed_out,
                              std::string* error) {
  Bdev* base = options.base;
  return marked_call(packed_out, [&](uint64_t* packed) -> int {
    if (base != nullptr) {
      if (!granule_ranges_ok(src, src_offset, base, options.base_offset,
                             length, granule, &bitmap)) {
        return kIoInvalid;
      }
      // Overlap is only possible within one backing store (validated
      // ranges: the difference below cannot wrap).
      const void* s_base = src->device_base();
      const bool same_store =
          src == base || (s_base != nullptr && s_base == base->device_base() &&
                          src->gpu_device() == base->gpu_device());
      if (same_store && std::max(src_offset, options.base_offset) -
                                std::min(src_offset, options.base_offset) <
                            length) {
        if (error != nullptr) *error = "the volume and its base overlap";
        return kIoInvalid;
      }
    }
    MarkedPlan plan;
    const int status = lz_plan(src, src_offset, length, granule, bitmap,
                               options, static_cast<bool>(sink), &plan, error);
    if (status != kIoOk || plan.marked == 0) return status;
    const CallKey call(options.key);
    const int device = granule_kernel_device(src, base != nullptr ? base : src);
    if (device < 0) {
      return compress_generic(src, src_offset, base, options.base_offset,
                              length, granule, bitmap, options.staging_bytes,
                              sink, call.key, packed);
    }
    LzStream ls(device, src, src_offset, granule, plan, true, call.key,
                base != nullptr,
                base != nullptr
                    ? static_cast<const uint8_t*>(base->device_base()) +
                          options.base_offset
                    : nullptr);
    return compress_gpu(ls, plan, sink, packed);
  });
}

int bdev_decompress_marked_sync(Bdev* dst, uint64_t dst_offset,
                                uint64_t length, uint32_t granule,
                                const std::vector<uint64_t>& bitmap,
                                const LzOptions& options,
                                const DecompressSource& source,
                                uint64_t* unpacked_out, std::string* error) {
  return marked_call(unpacked_out, [&](uint64_t* unpacked) -> int {
    MarkedPlan plan;
    const int status =
        lz_plan(dst, dst_offset, length, granule, bitmap, options,
                static_cast<bool>(source), &plan, error);
    if (status != kIoOk || plan.marked == 0) return status;
    const CallKey call(options.key);
    const int device = granule_kernel_device(dst, dst);
    if (device < 0) {
      return decompress_generic(dst, dst_offset, length, granule, bitmap,
                                options.staging_bytes, source,
                                options.dictionary, call.key, unpacked, error);
    }
    LzStream ls(device, dst, dst_offset, granule, plan, false, call.key,
                options.dictionary, nullptr);
    return decompress_gpu(ls, plan, bitmap, source, unpacked, error);
  });
}

}  // namespace hipstore
