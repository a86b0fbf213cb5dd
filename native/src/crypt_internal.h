// Private to native/src: what compress_ops.hip needs of crypt_ops.hip to
// run k_xts_var, the HSXTS2 pass over the variable-length pieces of a
// window, on its own stream between its own kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hipstore/crypt.h"
#include "marked_internal.h"

namespace hipstore {

// Little-endian words of two 240-byte schedules; travels in the
// kernel-argument struct. Whoever holds one clears it.
struct XtsKernelKeys {
  uint32_t data[60];   // K1: encryption, or equivalent inverse cipher
  uint32_t tweak[60];  // K2: encryption
};

void xts_load_kernel_keys(const XtsSchedules& schedules, bool encrypt,
                          XtsKernelKeys* keys);

// One k_xts_var launch on `stream` for the pieces of `win`; all pointers
// are device addresses. Piece r has sizes[r] bytes (cut to `granule`; 0
// is skipped) and is unit first_unit + its granule's index in the range.
//   encrypt: `from` holds slots of stride `granule`, piece r at the start
//            of slot r; ciphertext goes to to + offsets[r].
//   decrypt: ciphertext at from + offsets[r], plaintext to to + offsets[r].
// A piece occupies lz_padded(max(size, 16)) bytes at its offset; what lies
// behind its last byte there is written as zero.
void xts_var_launch(bool encrypt, hipStream_t stream, const uint8_t* from,
                    uint8_t* to, const uint32_t* sizes, const uint64_t* offsets,
                    const unsigned long long* bitmap,
                    const uint32_t* rank_before_word, const MarkedWindow& win,
                    uint32_t granule, uint64_t first_unit,
                    const XtsKernelKeys& keys);

}  // namespace hipstore
