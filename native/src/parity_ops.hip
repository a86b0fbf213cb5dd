// MI355X (gfx950) P+Q parity across HBM bdevs: encode, check, rebuild
// and update (definitions in hipstore/parity.h). Like bulk_ops.hip, each
// call owns its stream, runs to completion and returns.
//
// Data movement: HBM -> VGPR -> HBM, nothing is staged through LDS.
// Every byte of every member is read exactly once, by one lane, and no
// lane ever needs a byte another lane loaded, so LDS would only add a
// round trip. (k_parity_check uses 32 bytes of LDS to join the four
// waves' bitmap slices, never for data.) The same holds for
// k_parity_update: a lane's 16 bytes of a member, of its base and of the
// stored parity meet in that lane's registers; what the lanes of a slab
// share is one bit per decision, and a ballot carries that.
//
// Work split: a lane owns one 16-byte column of the range at a time and
// walks the k members of that column from k-1 down to 0 (Horner:
// Q = 2*Q ^ D_i). The member base pointers, offsets applied, arrive by
// value in one kernel-argument struct, so the member loop is
// wave-uniform, the pointers sit in scalar registers and a wave's 64
// loads of one member are 1 KiB contiguous. Members go four at a time:
// the four loads are issued before the dependent doubling chain of any
// of them, so several loads stay in flight behind the VALU work.
//
// Arithmetic: no lookup tables on the device. Doubling is done on four
// packed bytes per 32-bit word; multiplying by a wave-uniform constant
// (rebuild epilogue only) is a bit-Horner over the constant behind
// scalar branches: at most 7 doublings and conditional XORs.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "gpu_internal.h"
#include "hipstore/parity.h"

namespace hipstore {

namespace {

// --- GF(2^8) on 16 packed bytes ---------------------------------------------

__device__ __forceinline__ uint32_t gf_double4(uint32_t w) {
  return ((w & 0x7f7f7f7fu) << 1) ^ (((w >> 7) & 0x01010101u) * 0x1du);
}

__device__ __forceinline__ uint4 gf_double16(const uint4 v) {
  return make_uint4(gf_double4(v.x), gf_double4(v.y), gf_double4(v.z),
                    gf_double4(v.w));
}

__device__ __forceinline__ uint4 xor16(const uint4 a, const uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}

__device__ __forceinline__ uint32_t or_reduce16(const uint4 v) {
  return v.x | v.y | v.z | v.w;
}

// c * v for a wave-uniform c != 0: Horner over the bits of c below its
// top bit. c == 1 costs nothing.
__device__ __forceinline__ uint4 gf_mul_const16(const uint4 v, uint32_t c) {
  uint4 r = v;
  for (int b = 30 - __builtin_clz(c); b >= 0; --b) {  // scalar loop
    r = gf_double16(r);
    if ((c >> b) & 1u) r = xor16(r, v);  // scalar branch
  }
  return r;
}

// --- the member walk ---------------------------------------------------------
//
// P and / or Q of column `col` over the members of `set`. kLost: a null
// slot is a lost member; it skips the load and the XOR but keeps the
// doubling, so the survivors keep their powers of g.
constexpr uint32_t kParityUnroll = 4;  // members loaded ahead of their chain

template <bool kP, bool kQ, bool kLost>
__device__ __forceinline__ void parity_fold(bool have, const uint4 v,
                                            uint4& p, uint4& q) {
  if (kQ) q = gf_double16(q);
  if (!kLost || have) {  // wave-uniform
    if (kP) p = xor16(p, v);
    if (kQ) q = xor16(q, v);
  }
}

template <bool kP, bool kQ, bool kLost>
__device__ __forceinline__ void parity_walk(const ParitySet& set, uint64_t col,
                                            uint4& p, uint4& q) {
  const uint4 zero = make_uint4(0, 0, 0, 0);
  p = zero;
  q = zero;  // 2 * 0 ^ D_{k-1} = D_{k-1}: the first step needs no case
  uint32_t i = set.k;
  for (; i >= kParityUnroll; i -= kParityUnroll) {
    uint4 v[kParityUnroll];
    bool have[kParityUnroll];
#pragma unroll
    for (uint32_t j = 0; j < kParityUnroll; ++j) {
      const uint8_t* base = set.data[i - 1 - j];
      have[j] = !kLost || base != nullptr;
      v[j] = have[j] ? reinterpret_cast<const uint4*>(base)[col] : zero;
    }
#pragma unroll
    for (uint32_t j = 0; j < kParityUnroll; ++j) {
      parity_fold<kP, kQ, kLost>(have[j], v[j], p, q);
    }
  }
  while (i > 0) {
    --i;
    const uint8_t* base = set.data[i];
    const bool have = !kLost || base != nullptr;
    const uint4 v = have ? reinterpret_cast<const uint4*>(base)[col] : zero;
    parity_fold<kP, kQ, kLost>(have, v, p, q);
  }
}

// --- kernels -----------------------------------------------------------------

constexpr uint32_t kParityThreads = 256;
constexpr uint32_t kParityMaxWgs = 2048;  // as hbm_copy_sync: fills the chip

// Flat grid-stride over the 16-byte columns of the range.
template <bool kP, bool kQ>
__global__ __launch_bounds__(kParityThreads) void k_parity_encode(
    const ParitySet set, uint4* __restrict__ p_out, uint4* __restrict__ q_out,
    uint64_t n16) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kParityThreads;
  for (uint64_t col =
           static_cast<uint64_t>(blockIdx.x) * kParityThreads + threadIdx.x;
       col < n16; col += stride) {
    uint4 p, q;
    parity_walk<kP, kQ, false>(set, col, p, q);
    if (kP) p_out[col] = p;
    if (kQ) q_out[col] = q;
  }
}

// Work split of k_diff_granules: one workgroup per 64-granule bitmap
// word per grid-stride step, one wave per 16-granule slice, one whole
// granule at a time. The recomputed parity is XORed against the stored
// one and ORed into a lane-private accumulator; one ballot per granule
// decides its bit. Thread 0 writes each word with one plain store: no
// atomics, no pre-zeroed buffer, tail bits 0.
constexpr uint32_t kCheckGranulesPerWave = 64 / kWavesPerWg;

template <bool kP, bool kQ>
__global__ __launch_bounds__(kWavesPerWg * 64) void k_parity_check(
    const ParitySet set, const uint4* __restrict__ p_stored,
    const uint4* __restrict__ q_stored, uint64_t n_granules,
    uint32_t granule_bytes, unsigned long long* __restrict__ p_bitmap,
    unsigned long long* __restrict__ q_bitmap) {
  __shared__ uint32_t partial[2][kWavesPerWg];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint64_t n_words = (n_granules + 63) >> 6;
  for (uint64_t w = blockIdx.x; w < n_words; w += gridDim.x) {
    const uint64_t g0 = w * 64 + wave * kCheckGranulesPerWave;
    uint32_t p_bits = 0;
    uint32_t q_bits = 0;
    for (uint32_t j = 0; j < kCheckGranulesPerWave; ++j) {
      const uint64_t g = g0 + j;
      if (g >= n_granules) break;  // wave-uniform
      const uint64_t col0 = g * n16;
      uint32_t p_acc = 0;
      uint32_t q_acc = 0;
      for (uint32_t i = lane; i < n16; i += 64) {
        const uint64_t col = col0 + i;
        uint4 ps, qs, p, q;
        if (kP) ps = p_stored[col];  // in flight behind the walk
        if (kQ) qs = q_stored[col];
        parity_walk<kP, kQ, false>(set, col, p, q);
        if (kP) p_acc |= or_reduce16(xor16(p, ps));
        if (kQ) q_acc |= or_reduce16(xor16(q, qs));
      }
      if (kP && __ballot(p_acc != 0) != 0ull) p_bits |= 1u << j;
      if (kQ && __ballot(q_acc != 0) != 0ull) q_bits |= 1u << j;
    }
    if (lane == 0) {
      partial[0][wave] = p_bits;
      partial[1][wave] = q_bits;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long p_word = 0;
      unsigned long long q_word = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWavesPerWg; ++k) {
        p_word |= static_cast<unsigned long long>(partial[0][k])
                  << (k * kCheckGranulesPerWave);
        q_word |= static_cast<unsigned long long>(partial[1][k])
                  << (k * kCheckGranulesPerWave);
      }
      if (kP) p_bitmap[w] = p_word;
      if (kQ) q_bitmap[w] = q_word;
    }
    __syncthreads();  // partial[] is rewritten by the next step
  }
}

// Same flat column split as encode. kP / kQ: which syndromes the
// coefficients need (c_a != 0 / c_b != 0); the parity that is not needed
// is neither recomputed nor read. out_a = c_a * S_P ^ c_b * S_Q and,
// for a second lost data member, out_b = S_P ^ out_a.
template <bool kP, bool kQ>
__global__ __launch_bounds__(kParityThreads) void k_parity_rebuild(
    const ParitySet set, const uint4* __restrict__ p_stored,
    const uint4* __restrict__ q_stored, uint32_t c_a, uint32_t c_b,
    uint4* __restrict__ out_a, uint4* __restrict__ out_b, uint64_t n16) {
  const uint64_t stride = static_cast<uint64_t>(gridDim.x) * kParityThreads;
  for (uint64_t col =
           static_cast<uint64_t>(blockIdx.x) * kParityThreads + threadIdx.x;
       col < n16; col += stride) {
    uint4 sp, sq, p, q;
    if (kP) sp = p_stored[col];  // in flight behind the walk
    if (kQ) sq = q_stored[col];
    parity_walk<kP, kQ, true>(set, col, p, q);
    uint4 a = make_uint4(0, 0, 0, 0);
    if (kP) {
      sp = xor16(sp, p);
      a = gf_mul_const16(sp, c_a);
    }
    if (kQ) {
      sq = xor16(sq, q);
      a = xor16(a, gf_mul_const16(sq, c_b));
    }
    out_a[col] = a;
    if (kP && out_b != nullptr) out_b[col] = xor16(sp, a);  // wave-uniform
  }
}

// --- update ------------------------------------------------------------------
//
// One step of the update walk: member `idx` of one slab (64 lanes x one
// 16-byte column). `nw` / `old` are the member's and its base's columns,
// loaded by the caller ahead of this chain (zero in a lane past the
// granule's end, so such a lane contributes nothing). An untracked
// member keeps the doubling and nothing else. With kRefresh a member
// that differs from its base anywhere in the slab stores its column into
// the base's slab: one wave-uniform decision per member and slab.
template <bool kP, bool kQ, bool kRefresh>
__device__ __forceinline__ void update_fold(const ParitySet& bases,
                                            uint32_t idx, uint64_t col,
                                            bool active, const uint4 nw,
                                            const uint4 old, uint4& p,
                                            uint4& q, uint32_t& dirty) {
  if (kQ) q = gf_double16(q);
  const uint8_t* base = bases.data[idx];
  if (base == nullptr) return;  // wave-uniform
  const uint4 d = xor16(nw, old);
  const uint32_t any = or_reduce16(d);
  if (kP) p = xor16(p, d);
  if (kQ) q = xor16(q, d);
  dirty |= any;
  if (kRefresh && __ballot(any != 0) != 0ull && active) {
    reinterpret_cast<uint4*>(const_cast<uint8_t*>(base))[col] = nw;
  }
}

// Member `idx`'s and its base's column: zero for an untracked member
// (wave-uniform) and in a lane past the granule's end. A branch, not a
// conditional expression between a load and a zero: that one selects
// between two addresses and turns the loads into flat loads.
__device__ __forceinline__ void update_load(const ParitySet& set,
                                            const ParitySet& bases,
                                            uint32_t idx, uint64_t col,
                                            bool active, uint4& nw,
                                            uint4& old) {
  nw = make_uint4(0, 0, 0, 0);
  old = make_uint4(0, 0, 0, 0);
  const uint8_t* base = bases.data[idx];
  if (base != nullptr && active) {
    nw = reinterpret_cast<const uint4*>(set.data[idx])[col];
    old = reinterpret_cast<const uint4*>(base)[col];
  }
}

// The P and / or Q deltas of one slab over the tracked members below
// `top` (the highest tracked index + 1: the doublings of a still-zero q
// above it are never executed), Horner as parity_walk and with its
// unroll: the loads of the tracked members among kParityUnroll indices,
// two per member, are issued before any of their chains. Returns the
// lane's OR of its d_i, which decides the slab's bit and whether parity
// is touched: not p | q, which cancelling deltas leave zero.
template <bool kP, bool kQ, bool kRefresh>
__device__ __forceinline__ uint32_t update_walk(const ParitySet& set,
                                                const ParitySet& bases,
                                                uint32_t top, uint64_t col,
                                                bool active, uint4& p,
                                                uint4& q) {
  const uint4 zero = make_uint4(0, 0, 0, 0);
  p = zero;
  q = zero;
  uint32_t dirty = 0;
  uint32_t i = top;
  for (; i >= kParityUnroll; i -= kParityUnroll) {
    uint4 nw[kParityUnroll];
    uint4 old[kParityUnroll];
#pragma unroll
    for (uint32_t j = 0; j < kParityUnroll; ++j) {
      update_load(set, bases, i - 1 - j, col, active, nw[j], old[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kParityUnroll; ++j) {
      update_fold<kP, kQ, kRefresh>(bases, i - 1 - j, col, active, nw[j],
                                    old[j], p, q, dirty);
    }
  }
  while (i > 0) {
    --i;
    uint4 nw, old;
    update_load(set, bases, i, col, active, nw, old);
    update_fold<kP, kQ, kRefresh>(bases, i, col, active, nw, old, p, q, dirty);
  }
  return dirty;
}

// Diff, parity read-modify-write and base refresh in one pass. Work
// split of k_parity_check, because the output is a granule bitmap: a
// workgroup per 64-granule word per grid-stride step, a wave per
// 16-granule slice; inside a granule the wave takes one 1 KiB slab at a
// time, and in a ragged last slab (a 512-byte granule is half a slab)
// the lanes at or past n16 idle: they load nothing, store nothing and
// vote 0, and the slab loop itself stays wave-uniform so every ballot
// sees the whole wave.
//
// Per slab the wave decides by ballot: if no lane saw a difference the
// stored parity of the slab is neither read nor written; otherwise every
// active lane loads its P / Q column, XORs the delta in and stores it.
// The granule's bit is the OR of its slabs' ballots, so a clear bit
// means no parity byte of the granule was written. The write predicate
// is per slab, not per lane, so that a dirty slab is rewritten as whole
// 1 KiB runs and not as scattered 16-byte columns; a per-lane predicate
// would store fewer bytes. Nobody has measured one against the other.
//
// The bases are distinct from the members and the parities (validated
// on the host), so a refresh store never feeds a later load.
template <bool kP, bool kQ, bool kRefresh>
__global__ __launch_bounds__(kWavesPerWg * 64) void k_parity_update(
    const ParitySet set, const ParitySet bases, uint32_t top, uint4* p_io,
    uint4* q_io, uint64_t n_granules, uint32_t granule_bytes,
    unsigned long long* __restrict__ bitmap) {
  __shared__ uint32_t partial[kWavesPerWg];
  const uint32_t wave = threadIdx.x >> 6;
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n16 = granule_bytes >> 4;
  const uint64_t n_words = (n_granules + 63) >> 6;
  for (uint64_t w = blockIdx.x; w < n_words; w += gridDim.x) {
    const uint64_t g0 = w * 64 + wave * kCheckGranulesPerWave;
    uint32_t bits = 0;
    for (uint32_t j = 0; j < kCheckGranulesPerWave; ++j) {
      const uint64_t g = g0 + j;
      if (g >= n_granules) break;  // wave-uniform
      const uint64_t col0 = g * n16;
      for (uint32_t s = 0; s < n16; s += 64) {  // wave-uniform
        const bool active = s + lane < n16;
        const uint64_t col = col0 + s + lane;  // dereferenced if active
        uint4 p, q;
        const uint32_t dirty = update_walk<kP, kQ, kRefresh>(
            set, bases, top, col, active, p, q);
        if (__ballot(dirty != 0) == 0ull) continue;
        bits |= 1u << j;
        if (active) {
          uint4 ps, qs;
          if (kP) ps = p_io[col];
          if (kQ) qs = q_io[col];
          if (kP) p_io[col] = xor16(ps, p);
          if (kQ) q_io[col] = xor16(qs, q);
        }
      }
    }
    if (lane == 0) partial[wave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long word = 0;
#pragma unroll
      for (uint32_t k = 0; k < kWavesPerWg; ++k) {
        word |= static_cast<unsigned long long>(partial[k])
                << (k * kCheckGranulesPerWave);
      }
      bitmap[w] = word;
    }
    __syncthreads();  // partial[] is rewritten by the next step
  }
}

// --- launch helpers ----------------------------------------------------------

uint32_t column_grid(uint64_t n16) {
  return static_cast<uint32_t>(std::min<uint64_t>(
      (n16 + kParityThreads - 1) / kParityThreads, kParityMaxWgs));
}

uint32_t check_grid(uint64_t n_granules) {
  return static_cast<uint32_t>(
      std::min<uint64_t>((n_granules + 63) / 64, kParityMaxWgs));
}

// Calls `go` with the <kP, kQ> instantiation picked at run time; one of
// the two is always wanted.
template <typename Go>
void with_parity_flags(bool want_p, bool want_q, Go go) {
  if (want_p && want_q) {
    go(std::true_type{}, std::true_type{});
  } else if (want_p) {
    go(std::true_type{}, std::false_type{});
  } else {
    go(std::false_type{}, std::true_type{});
  }
}

// Per-thread pinned bitmaps of the check and (p_words only) the update:
// the kernel writes them in place (zero-copy, 1/4096 of the data at
// 512-byte granules).
struct CheckCtx {
  PinnedBuf<unsigned long long> p_words;
  PinnedBuf<unsigned long long> q_words;
};
constexpr uint64_t kMinCheckWords = 4096;

CheckCtx& check_ctx() {
  thread_local CheckCtx ctx;
  return ctx;
}

}  // namespace

int parity_kernel_device(const std::vector<Bdev*>& members) {
  if (members.empty() || !gpu_available()) return -1;
  for (Bdev* m : members) {
    if (m->device_base() == nullptr || m->gpu_device() < 0) return -1;
  }
  const int device = members[0]->gpu_device();
  for (Bdev* m : members) {
    const int other = m->gpu_device();
    if (other == device) continue;
    int can = 0;
    if (hipSetDevice(device) != hipSuccess ||
        hipDeviceCanAccessPeer(&can, device, other) != hipSuccess ||
        can == 0) {
      (void)hipGetLastError();
      return -1;
    }
    const hipError_t err = hipDeviceEnablePeerAccess(other, 0);
    (void)hipGetLastError();  // "already enabled" must not stick
    if (err != hipSuccess && err != hipErrorPeerAccessAlreadyEnabled) {
      return -1;
    }
  }
  return device;
}

int parity_encode_gpu(int device, const ParitySet& set, uint8_t* p, uint8_t* q,
                      uint64_t length) {
  if (set.k == 0 || set.k > kParityMaxData || (p == nullptr && q == nullptr) ||
      length == 0 || length % 16 != 0) {
    return kIoInvalid;
  }
  const uint64_t n16 = length / 16;
  return run_granule_kernel(device, [&](hipStream_t stream) {
    with_parity_flags(p != nullptr, q != nullptr, [&](auto kp, auto kq) {
      hipLaunchKernelGGL((k_parity_encode<kp.value, kq.value>),
                         dim3(column_grid(n16)), dim3(kParityThreads), 0,
                         stream, set, reinterpret_cast<uint4*>(p),
                         reinterpret_cast<uint4*>(q), n16);
    });
  });
}

int parity_check_gpu(int device, const ParitySet& set, const uint8_t* p,
                     const uint8_t* q, uint64_t n_granules, uint32_t granule,
                     std::vector<uint64_t>* p_words,
                     std::vector<uint64_t>* q_words) {
  if (set.k == 0 || set.k > kParityMaxData || (p == nullptr && q == nullptr) ||
      n_granules == 0 || granule == 0 || granule % 16 != 0) {
    return kIoInvalid;
  }
  const uint64_t n_words = (n_granules + 63) / 64;
  try {
    CheckCtx& ctx = check_ctx();
    const uint64_t room = std::max(n_words, kMinCheckWords);
    unsigned long long* pw = ctx.p_words.reserve(room);
    unsigned long long* qw = ctx.q_words.reserve(room);
    unsigned long long* dev_pw = device_view(pw);
    unsigned long long* dev_qw = device_view(qw);
    const int status = run_granule_kernel(device, [&](hipStream_t stream) {
      with_parity_flags(p != nullptr, q != nullptr, [&](auto kp, auto kq) {
        hipLaunchKernelGGL((k_parity_check<kp.value, kq.value>),
                           dim3(check_grid(n_granules)),
                           dim3(kWavesPerWg * 64), 0, stream, set,
                           reinterpret_cast<const uint4*>(p),
                           reinterpret_cast<const uint4*>(q), n_granules,
                           granule, dev_pw, dev_qw);
      });
    });
    if (status != kIoOk) return status;
    if (p != nullptr) p_words->assign(pw, pw + n_words);
    if (q != nullptr) q_words->assign(qw, qw + n_words);
    return kIoOk;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

int parity_rebuild_gpu(int device, const ParitySet& set, const uint8_t* p,
                       const uint8_t* q, ParityCoeffs coeffs, uint8_t* out_a,
                       uint8_t* out_b, uint64_t length) {
  const bool need_p = coeffs.a != 0;
  const bool need_q = coeffs.b != 0;
  if (set.k == 0 || set.k > kParityMaxData || (!need_p && !need_q) ||
      (need_p && p == nullptr) || (need_q && q == nullptr) ||
      (out_b != nullptr && !need_p) || out_a == nullptr || length == 0 ||
      length % 16 != 0) {
    return kIoInvalid;
  }
  const uint64_t n16 = length / 16;
  return run_granule_kernel(device, [&](hipStream_t stream) {
    with_parity_flags(need_p, need_q, [&](auto kp, auto kq) {
      hipLaunchKernelGGL((k_parity_rebuild<kp.value, kq.value>),
                         dim3(column_grid(n16)), dim3(kParityThreads), 0,
                         stream, set, reinterpret_cast<const uint4*>(p),
                         reinterpret_cast<const uint4*>(q),
                         static_cast<uint32_t>(coeffs.a),
                         static_cast<uint32_t>(coeffs.b),
                         reinterpret_cast<uint4*>(out_a),
                         reinterpret_cast<uint4*>(out_b), n16);
    });
  });
}

int parity_update_gpu(int device, const ParitySet& set, const ParitySet& bases,
                      uint8_t* p, uint8_t* q, uint64_t n_granules,
                      uint32_t granule, bool refresh,
                      std::vector<uint64_t>* words) {
  if (set.k == 0 || set.k > kParityMaxData || bases.k != set.k ||
      (p == nullptr && q == nullptr) || n_granules == 0 || granule == 0 ||
      granule % 16 != 0 || words == nullptr) {
    return kIoInvalid;
  }
  uint32_t top = 0;  // highest tracked index + 1
  for (uint32_t i = 0; i < set.k; ++i) {
    if (bases.data[i] == nullptr) continue;
    if (set.data[i] == nullptr) return kIoInvalid;
    top = i + 1;
  }
  if (top == 0) return kIoInvalid;
  const uint64_t n_words = (n_granules + 63) / 64;
  try {
    unsigned long long* host_words =
        check_ctx().p_words.reserve(std::max(n_words, kMinCheckWords));
    unsigned long long* dev_words = device_view(host_words);
    const int status = run_granule_kernel(device, [&](hipStream_t stream) {
      with_parity_flags(p != nullptr, q != nullptr, [&](auto kp, auto kq) {
        auto launch = [&](auto kr) {
          hipLaunchKernelGGL(
              (k_parity_update<kp.value, kq.value, kr.value>),
              dim3(check_grid(n_granules)), dim3(kWavesPerWg * 64), 0, stream,
              set, bases, top, reinterpret_cast<uint4*>(p),
              reinterpret_cast<uint4*>(q), n_granules, granule, dev_words);
        };
        if (refresh) {
          launch(std::true_type{});
        } else {
          launch(std::false_type{});
        }
      });
    });
    if (status != kIoOk) return status;
    words->assign(host_words, host_words + n_words);
    return kIoOk;
  } catch (const std::exception&) {
    return kIoFailed;
  }
}

}  // namespace hipstore
