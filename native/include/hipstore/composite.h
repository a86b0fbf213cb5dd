// Striped / replicated composite bdevs (BASELINE config 5).
//
// On an 8-GPU MI355X node, a striped malloc bdev shards its block
// address space across per-GPU HBM children (stripe units round-robin
// over the children), and a replicated bdev mirrors writes to every
// child. Replica fan-out between HBM children uses direct xGMI
// point-to-point copies (hipMemcpyPeerAsync) from the primary's
// backing store — the per-link-direct topology SURVEY.md section 2.4
// calls for (7 x ~153 GB/s links per GPU; a host-side 8x PCIe write
// would bottleneck at ~63 GB/s) — overlapped on a dedicated stream.
// CPU children (tests) fall back to host-side mirrored writes.

#pragma once

#include <vector>

#include "hipstore/bdev.h"

namespace hipstore {

// `stripe_size` bytes per stripe unit; must be a multiple of the
// children's block size. All children must share block size and size.
BdevPtr create_striped_bdev(const std::string& name,
                            std::vector<BdevPtr> children,
                            uint64_t stripe_size);

// Mirror: every child holds a full copy. Reads round-robin across
// children; writes land on the primary and fan out over xGMI.
BdevPtr create_replicated_bdev(const std::string& name,
                               std::vector<BdevPtr> children);

// Replica scrub: compares every other child of a replicated bdev with
// child 0 over the whole device (bdev_diff_sync, so HBM children are
// compared on the GPU) and reports one entry per replica. Child 0, the
// primary, is authoritative: the write path already treats a primary
// failure as fatal and the replicas as followers.
//
// With `repair`, each replica's mismatching granules are then
// overwritten from the primary (bdev_copy_marked_sync). A repair racing
// a guest write could put stale primary data over a newer fan-out, so
// repair is refused with kIoFailed while the bdev is claimed() (the
// offline rule resize follows). A compare-only scrub is allowed at any
// time and is advisory: in-flight mirrored writes may show up as
// transient mismatches.
//
// `granule` 0 means the block size. status is kIoInvalid when `bdev` is
// not a replicated bdev or the granule is invalid; replicas compared
// before a failure stay in the result.
struct ScrubReplica {
  size_t child = 0;         // index among the children (>= 1)
  uint64_t granules = 0;
  uint64_t mismatched = 0;
  uint64_t repaired = 0;    // granules copied from the primary
  std::vector<uint64_t> first_mismatches;
};
struct ScrubResult {
  int status = kIoOk;  // IoStatus
  uint32_t granule = 0;
  std::vector<ScrubReplica> replicas;
};
ScrubResult replicated_scrub(Bdev* bdev, bool repair, uint32_t granule,
                             uint32_t max_report);

}  // namespace hipstore
