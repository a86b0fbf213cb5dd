// Private to native/src: the launch of hipstore::k_blake2s_granules
// (blake2s_ops.hip), which bulk_ops.hip's fingerprint windows use for
// HSFP2 (fingerprint.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hipstore/fingerprint.h"

namespace hipstore {

// Enqueues the HSFP2 fingerprints of `count` >= 1 granules of `granule`
// bytes (a multiple of 16) at device address `base` (16-byte aligned)
// into out[0 .. count * 16), device-visible. `start` is passed by value in
// the kernel arguments; the kernel reads no key. The caller checks
// hipGetLastError.
void launch_blake2s_granules(hipStream_t stream, const uint8_t* base,
                             uint64_t count, uint32_t granule,
                             const Blake2sMidstate& start, uint8_t* out);

}  // namespace hipstore
