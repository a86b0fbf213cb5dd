// MI355X (gfx950) BLAKE2s granule fingerprints ("HSFP2", fingerprint.h):
// hipstore::k_blake2s_granules and its launch. bulk_ops.hip's fingerprint
// windows call it; the host byte model is fingerprint.cpp's scalar
// BLAKE2s, which is deliberately another shape.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "blake2s_internal.h"

namespace hipstore {

namespace {

constexpr uint32_t kBlakeWaves = 4;        // 256-thread workgroups
constexpr uint32_t kBlakeQuads = 16;       // granules of one wave's group
constexpr uint32_t kBlakeUnroll = 4;       // blocks loaded ahead of their rounds
constexpr uint32_t kBlakeBlockWords = 256; // one staged block of a wave: 1 KiB
constexpr uint32_t kBlakeMaxWgs = 2048;

// --- the split ---------------------------------------------------------------
//
// A quad of lanes owns a granule and a wave 16 consecutive granules;
// waves grid-stride over such groups. Lane c = lane & 3 of a quad holds
// column c of the 4x4 state (v[c], v[4+c], v[8+c], v[12+c]) and the
// chaining words h[c], h[4+c]. The column step is one G per lane. For the
// diagonal step rows 1..3 rotate within the quad by DPP quad_perm
// (v[4+(c+1)%4], v[8+(c+2)%4], v[12+(c+3)%4] come to lane c), G runs
// again, and the rows rotate back. Nothing crosses a quad.
//
// --- the message -------------------------------------------------------------
//
// Lane c loads bytes 16c .. 16c+15 of a 64-byte block: message words
// 4c .. 4c+3. Which words a lane needs in a round depends on the lane
// (m[sigma[r][2c]], m[sigma[r][2c+1]], then m[sigma[r][8+2c]],
// m[sigma[r][8+2c+1]]), so a block goes through a wave-private LDS
// region: word i of quad q lies at word
//   ((i & 3) * 4 + (i >> 2)) * 16 + q
// of its 256. The four stores of a lane (i = 4c + j, j fixed per
// instruction) then go to word j * 64 + c * 16 + q, 64 different banks
// per instruction, and a load of one word index by all 16 quads touches
// 16 consecutive banks. Loads of a quad's four lanes fall in the same 16
// banks when two of their sigma entries agree in i >> 2.
//
// The 40 word offsets of a lane are loop-invariant: four 4-bit slots per
// (round, use) are packed at compile time and lane c takes nibble c.
// kBlakeUnroll blocks are in flight: the loads of the next four are
// issued before the rounds of the staged four. A wave orders its own LDS
// traffic (wave_sync); there is no workgroup barrier.

struct SigmaPack {
  uint16_t v[10][4];
};

constexpr uint32_t blake_slot(uint32_t i) { return ((i & 3) << 2) | (i >> 2); }

constexpr SigmaPack make_sigma_pack() {
  constexpr uint8_t sigma[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15},
      {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4},
      {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13},
      {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11},
      {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5},
      {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  SigmaPack pack = {};
  for (uint32_t r = 0; r < 10; ++r) {
    for (uint32_t c = 0; c < 4; ++c) {
      // use 0, 1: the column step; use 2, 3: the diagonal step
      const uint32_t at[4] = {2 * c, 2 * c + 1, 8 + 2 * c, 9 + 2 * c};
      for (uint32_t use = 0; use < 4; ++use) {
        pack.v[r][use] = static_cast<uint16_t>(
            pack.v[r][use] | blake_slot(sigma[r][at[use]]) << (4 * c));
      }
    }
  }
  return pack;
}

__device__ constexpr SigmaPack kSigmaPack = make_sigma_pack();

// Orders this wave's LDS accesses, as in compress_ops.hip: LDS serves a
// wave in issue order, so only the compiler has to be held.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// v_alignbit_b32: rotate right.
__device__ __forceinline__ uint32_t rotr(uint32_t v, uint32_t n) {
  return __builtin_amdgcn_alignbit(v, v, n);
}

// quad_perm controls: lane i of a quad takes the value of lane (i + k) & 3.
constexpr int kQuadNext1 = 0x39;  // [1, 2, 3, 0]
constexpr int kQuadNext2 = 0x4E;  // [2, 3, 0, 1]
constexpr int kQuadNext3 = 0x93;  // [3, 0, 1, 2]

template <int kCtrl>
__device__ __forceinline__ uint32_t quad_rotate(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(
      static_cast<int>(v), static_cast<int>(v), kCtrl, 0xF, 0xF, true));
}

__device__ __forceinline__ uint32_t pick(uint32_t c, uint32_t v0, uint32_t v1,
                                         uint32_t v2, uint32_t v3) {
  return c == 0 ? v0 : c == 1 ? v1 : c == 2 ? v2 : v3;
}

__device__ __forceinline__ void blake_g(uint32_t& a, uint32_t& b, uint32_t& c,
                                        uint32_t& d, uint32_t x, uint32_t y) {
  a = a + b + x;
  d = rotr(d ^ a, 16);
  c = c + d;
  b = rotr(b ^ c, 12);
  a = a + b + y;
  d = rotr(d ^ a, 8);
  c = c + d;
  b = rotr(b ^ c, 7);
}

__global__ __launch_bounds__(kBlakeWaves * 64) void k_blake2s_granules(
    const uint8_t* __restrict__ base, uint64_t n_granules,
    uint32_t granule_bytes, const Blake2sMidstate start,
    uint32_t* __restrict__ out) {
  __shared__ uint32_t staged[kBlakeWaves * kBlakeUnroll * kBlakeBlockWords];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t c = lane & 3;
  const uint32_t q = lane >> 2;
  uint32_t* const mine = staged + wave * (kBlakeUnroll * kBlakeBlockWords);

  // What a lane keeps for the whole call.
  const uint32_t h_lo = pick(c, start.h[0], start.h[1], start.h[2], start.h[3]);
  const uint32_t h_hi = pick(c, start.h[4], start.h[5], start.h[6], start.h[7]);
  const uint32_t iv_lo =
      pick(c, 0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au);
  const uint32_t iv_hi =
      pick(c, 0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u);
  uint32_t moff[10][4];
#pragma unroll
  for (uint32_t r = 0; r < 10; ++r) {
#pragma unroll
    for (uint32_t use = 0; use < 4; ++use) {
      moff[r][use] = ((kSigmaPack.v[r][use] >> (4 * c)) & 15u) * kBlakeQuads + q;
    }
  }
  const uint32_t store_at = c * kBlakeQuads + q;  // + 64 * j for word 4c + j

  const uint64_t n_blocks = (static_cast<uint64_t>(granule_bytes) + 63) / 64;
  const uint64_t n_groups = (n_granules + kBlakeQuads - 1) / kBlakeQuads;
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kBlakeWaves;
  for (uint64_t group = static_cast<uint64_t>(blockIdx.x) * kBlakeWaves + wave;
       group < n_groups; group += stride) {  // wave-uniform
    const uint64_t g = group * kBlakeQuads + q;
    // A quad past the last granule runs on zeros and skips the store: the
    // quad permutes below need every lane of the wave.
    const bool live = g < n_granules;
    const uint8_t* __restrict__ p =
        base + (live ? g : 0) * granule_bytes + 16 * c;
    // Bytes 16c .. 16c+15 of block `blk`, zeros past the granule's end.
    auto fetch = [&](uint64_t blk) {
      uint4 w = make_uint4(0, 0, 0, 0);
      if (live && blk * 64 + 16 * c < granule_bytes) {
        w = *reinterpret_cast<const uint4*>(p + blk * 64);
      }
      return w;
    };
    uint32_t ch_lo = h_lo;
    uint32_t ch_hi = h_hi;
    uint4 ahead[kBlakeUnroll];
#pragma unroll
    for (uint32_t k = 0; k < kBlakeUnroll; ++k) ahead[k] = fetch(k);
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += kBlakeUnroll) {
      wave_sync();  // the rounds before have read their words
#pragma unroll
      for (uint32_t k = 0; k < kBlakeUnroll; ++k) {
        uint32_t* const slot = mine + k * kBlakeBlockWords + store_at;
        slot[0] = ahead[k].x;
        slot[64] = ahead[k].y;
        slot[128] = ahead[k].z;
        slot[192] = ahead[k].w;
      }
      wave_sync();
      if (b0 + kBlakeUnroll < n_blocks) {
#pragma unroll
        for (uint32_t k = 0; k < kBlakeUnroll; ++k) {
          ahead[k] = fetch(b0 + kBlakeUnroll + k);
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < kBlakeUnroll; ++k) {
        const uint64_t blk = b0 + k;
        if (blk >= n_blocks) break;  // wave-uniform
        // The last block, full or not, is the final one: t counts the
        // granule's bytes, not the padding.
        const bool last = blk + 1 == n_blocks;
        const uint64_t t =
            start.t0 + (last ? static_cast<uint64_t>(granule_bytes)
                             : (blk + 1) * 64);
        const uint32_t tweak =
            pick(c, static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32),
                 last ? ~0u : 0u, 0u);
        const uint32_t* const m = mine + k * kBlakeBlockWords;
        uint32_t va = ch_lo;
        uint32_t vb = ch_hi;
        uint32_t vc = iv_lo;
        uint32_t vd = iv_hi ^ tweak;
#pragma unroll
        for (uint32_t r = 0; r < 10; ++r) {
          blake_g(va, vb, vc, vd, m[moff[r][0]], m[moff[r][1]]);
          vb = quad_rotate<kQuadNext1>(vb);
          vc = quad_rotate<kQuadNext2>(vc);
          vd = quad_rotate<kQuadNext3>(vd);
          blake_g(va, vb, vc, vd, m[moff[r][2]], m[moff[r][3]]);
          vb = quad_rotate<kQuadNext3>(vb);
          vc = quad_rotate<kQuadNext2>(vc);
          vd = quad_rotate<kQuadNext1>(vd);
        }
        ch_lo ^= va ^ vc;
        ch_hi ^= vb ^ vd;
      }
    }
    if (live) out[g * 4 + c] = ch_lo;
  }
}

}  // namespace

void launch_blake2s_granules(hipStream_t stream, const uint8_t* base,
                             uint64_t count, uint32_t granule,
                             const Blake2sMidstate& start, uint8_t* out) {
  const uint64_t per_wg = kBlakeWaves * kBlakeQuads;
  const uint32_t grid = static_cast<uint32_t>(std::max<uint64_t>(
      1, std::min<uint64_t>((count + per_wg - 1) / per_wg, kBlakeMaxWgs)));
  hipLaunchKernelGGL(k_blake2s_granules, dim3(grid), dim3(kBlakeWaves * 64), 0,
                     stream, base, count, granule, start,
                     reinterpret_cast<uint32_t*>(out));
}

}  // namespace hipstore
