// GPU data-path engine API. The engines, bdev creation, the pinned
// helpers, the sync wrappers, IoQueue and bdevperf are implemented in
// gpu.hip; hbm_copy_sync and the bdev_diff / copy_marked / pack_marked /
// unpack_marked / fingerprint calls (and marked_copy_probe) in
// bulk_ops.hip.
//
// MI355X-native replacement for the reference's SPDK copy engine +
// malloc bdev pair (reference lib/copy/copy_engine.c,
// lib/bdev/malloc/bdev_malloc.c): block I/O executes as batched HIP
// kernel launches on per-queue streams, 4 KiB tiles staged through LDS
// (visible in rocprof as hipstore::k_copy_blocks), with pinned-host
// descriptor rings read by the GPU directly.

#pragma once

#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "hipstore/bdev.h"

namespace hipstore {

// True when at least one HIP device is present (cached).
bool gpu_available();
int gpu_device_count();
// PCI BDF string ("0000:c1:00.0") of a device, for registry <id>/pci.
std::string gpu_pci_address(int device);

// Create an HBM-resident malloc bdev on `device`. Throws std::runtime_error
// when no GPU or allocation fails. product_name stays "Malloc disk": the
// HBM bdev IS the malloc bdev on this platform, and the reference
// controller keys its keep-on-unmap logic on that string
// (reference controller.go:205).
// `persistent` selects the on-GPU polling service kernel (lowest
// latency; waves poll the submission ring and self-exit when idle)
// instead of batched per-poll launches.
BdevPtr create_hbm_bdev(const std::string& name, uint64_t block_size,
                        uint64_t num_blocks, int device,
                        bool persistent = false);

// Persistent-engine debug counters: 0=launches, 1=relaunches,
// 2=stall queries.
uint64_t persistent_stat(int which);

// Hardware liveness probe for the persistent-service idioms: launches
// a minimal leader+worker kernel pair and reports which legs of the
// host<->GPU polling contract work on this box (heartbeats, host-tail
// visibility, CQ publish, cross-workgroup relay). Keys: launch_err,
// hb_host_early/final, hb_dev_early/final, relay_final, cq0_ms,
// cq1_ms (-1 = never seen), stream_drained.
// flags: 1 atomics, 2 pre-launch pageable H2D memcpyAsync on the
// kernel's stream, 4 worker agent fetch_adds, 8 service-sized grid.
std::map<std::string, long long> persistent_probe(int device, int flags);

// Launches the real persistent-copy service kernel with a minimal
// standalone setup and serves one descriptor (0 = pinned->pinned,
// 1 = pinned->HBM, 2 = HBM->pinned).
std::map<std::string, long long> persistent_kernel_probe(int device,
                                                         int variant);

// HBM capacity of `device`: (total_bytes, free_bytes) via
// hipMemGetInfo; (0, 0) without a GPU.
std::pair<uint64_t, uint64_t> hbm_info(int device);

// Pinned-host buffer helpers (fall back to plain malloc without a GPU).
void* alloc_pinned(size_t bytes);
void free_pinned(void* ptr);

// Device-side range copy between HBM bdevs (volume clone / stripe
// rebuild): same-device copies run the LDS-staged block kernel at HBM
// rates; cross-device copies go over xGMI peer access. Returns
// IoStatus; kIoInvalid when either bdev is not HBM-resident or ranges
// are out of bounds/misaligned (offsets and length are multiples of
// 16: the kernel moves float4 elements) or overlap in device memory
// (a grid-stride copy is neither memcpy nor memmove on overlap).
int hbm_copy_sync(Bdev* src, uint64_t src_offset, Bdev* dst,
                  uint64_t dst_offset, uint64_t length);

// Granule-wise compare of two bdev ranges (clone verify, replica scrub,
// changed-block list). Bit g of the bitmap (word g/64, bit g%64) is set
// iff granule g of `a` differs from granule g of `b` in at least one
// byte; bits past the last granule are 0.
//
// When both bdevs are HBM-resident the compare runs on the GPU
// (hipstore::k_diff_granules; across devices the kernel runs on a's
// device and reads b over peer access). Every other pairing, and HBM
// pairs without peer access, read both sides through bdev_read_sync in
// chunks of at most 1 MiB and compare on the host; both paths give the
// same bitmap.
//
// Returns kIoInvalid unless: length > 0; both bdevs share a block size;
// `granule` is a multiple of that block size and of 16; offsets and
// length are multiples of `granule`; both ranges are in bounds.
struct DiffStats {
  uint64_t granules = 0;    // granules compared
  uint64_t mismatched = 0;  // popcount of the bitmap
  // First max_report mismatching granule indices, ascending.
  std::vector<uint64_t> first_mismatches;
};
int bdev_diff_sync(Bdev* a, uint64_t a_offset, Bdev* b, uint64_t b_offset,
                   uint64_t length, uint32_t granule, uint32_t max_report,
                   std::vector<uint64_t>* bitmap_out, DiffStats* stats);

// Default extent for the two calls here ("to the end of the shorter
// device"): min(size - offset) over both sides, rounded down to a
// multiple of `granule`; 0 when an offset lies past its device.
uint64_t bdev_common_length(Bdev* a, uint64_t a_offset, Bdev* b,
                            uint64_t b_offset, uint32_t granule);

// Copies the granules of [src_offset, +length) whose bit is set in
// `bitmap` (bdev_diff_sync layout) to the same granule of dst; other
// granules of dst are not written. Same validation and path selection
// as bdev_diff_sync (hipstore::k_copy_marked on the GPU path); also
// kIoInvalid when the bitmap is shorter than the range or the ranges
// overlap in one backing store. `copied` receives the number of
// granules copied.
int bdev_copy_marked_sync(Bdev* src, uint64_t src_offset, Bdev* dst,
                          uint64_t dst_offset, uint64_t length,
                          uint32_t granule,
                          const std::vector<uint64_t>& bitmap,
                          uint64_t* copied = nullptr);

// Gathers the granules of [src_offset, +length) whose bit is set in
// `bitmap` (bdev_diff_sync layout) into one dense stream, in ascending
// granule order, and hands it to `sink` in consecutive chunks:
// sink(data, first_rank, count) receives marked granules number
// first_rank .. first_rank + count - 1, `count * granule` bytes. A
// non-zero return aborts the call with that status. Bits at or past the
// last granule are ignored and not counted; no marked granule means no
// launch and no callback.
//
// An HBM-resident bdev with a usable GPU runs hipstore::k_pack_marked on
// its device, one launch per staging window, writing pinned host memory
// in place; the callback for one window overlaps the kernel of the next.
// Every other bdev reads runs of marked granules through bdev_read_sync
// in spans of at most 1 MiB. Both paths cut the same chunks: every chunk
// but the last holds max(1, staging_bytes / 2 / granule) granules
// (staging_bytes 0 = two halves of 16 MiB).
//
// Validation is that of bdev_copy_marked_sync on the one bdev; also
// kIoInvalid when the bitmap is shorter than the range or
// 0 < staging_bytes < granule. `packed` receives the granules delivered.
using PackSink =
    std::function<int(const uint8_t* data, uint64_t first_rank, uint64_t count)>;
int bdev_pack_marked_sync(Bdev* src, uint64_t src_offset, uint64_t length,
                          uint32_t granule,
                          const std::vector<uint64_t>& bitmap,
                          uint64_t staging_bytes, const PackSink& sink,
                          uint64_t* packed = nullptr);

// Inverse of bdev_pack_marked_sync: source(data, first_rank, count)
// fills the next chunk of the dense stream (same chunking), which is
// scattered to the marked granules of [dst_offset, +length)
// (hipstore::k_unpack_marked on the GPU path, bdev_write_sync
// otherwise). Unmarked granules of dst are never written. When `source`
// fails, chunks delivered before it stay written. `unpacked` receives
// the granules written.
using UnpackSource =
    std::function<int(uint8_t* data, uint64_t first_rank, uint64_t count)>;
int bdev_unpack_marked_sync(Bdev* dst, uint64_t dst_offset, uint64_t length,
                            uint32_t granule,
                            const std::vector<uint64_t>& bitmap,
                            uint64_t staging_bytes,
                            const UnpackSource& source,
                            uint64_t* unpacked = nullptr);

// Fingerprints (fingerprint.h, 16 bytes each) of the granules of
// [offset, +length), handed to `sink` in consecutive windows:
// sink(fps, first_granule, count) receives `count * 16` bytes for
// granules first_granule .. first_granule + count - 1 of the range. A
// non-zero return aborts the call with that status. Every window but the
// last holds max(1, staging_bytes / 2 / 16) granules (staging_bytes 0 =
// two halves of 16 MiB, a million granules each).
//
// An HBM-resident bdev with a usable GPU runs
// hipstore::k_fingerprint_granules on its device, one launch per window,
// writing pinned host memory in place; the callback for one window
// overlaps the kernel of the next. Every other bdev is read through
// bdev_read_sync in spans of at most 1 MiB and hashed on the host. Both
// paths cut the same windows and give the same bytes. The bdev is only
// read.
//
// Validation is that of bdev_diff_sync on the one bdev; also kIoInvalid
// when 0 < staging_bytes < 32 or the sink is empty. `done` receives the
// granules delivered.
using FingerprintSink = std::function<int(const uint8_t* fps,
                                          uint64_t first_granule,
                                          uint64_t count)>;
int bdev_fingerprint_sync(Bdev* bdev, uint64_t offset, uint64_t length,
                          uint32_t granule, uint64_t staging_bytes,
                          const FingerprintSink& sink,
                          uint64_t* done = nullptr);

// Measurement aid for tools/delta_bench.py: moves the marked bytes of
// an HBM bdev to pinned host memory by plain hipMemcpyAsync (mode 0: one
// copy of the same byte count, the PCIe ceiling; mode 1: one copy per
// run of marked granules; both into a pinned ring of `ring_bytes`) or by
// bdev_pack_marked_sync with `staging_bytes` and a sink that discards
// (mode 2), and reports the host-clock time.
struct MarkedCopyProbe {
  double seconds = 0;
  uint64_t granules = 0;  // marked granules moved
  uint64_t calls = 0;     // hipMemcpyAsync calls / sink callbacks
};
int marked_copy_probe(Bdev* src, uint32_t granule,
                      const std::vector<uint64_t>& bitmap, int mode,
                      uint64_t ring_bytes, uint64_t staging_bytes,
                      MarkedCopyProbe* out);

// Synchronous convenience wrappers (tests, NBD pump): create a
// throwaway channel, submit, poll to completion. Returns IoStatus.
int bdev_read_sync(Bdev* bdev, uint64_t offset, void* buf, uint64_t len);
int bdev_write_sync(Bdev* bdev, uint64_t offset, const void* buf, uint64_t len);
int bdev_fill_sync(Bdev* bdev, uint64_t offset, uint8_t value, uint64_t len);

// Queued-I/O primitive for tests: holds ONE channel from get_channel()
// for its lifetime (the way the daemon and the benchmark use channels)
// and runs a list of requests with all of them in flight at once.
// Works on any Bdev, so the same harness runs on the CPU malloc bdev.
class IoQueue {
 public:
  struct Op {
    IoOp op = IoOp::kRead;
    uint64_t offset = 0;
    uint64_t length = 0;   // writes: payload.size()
    uint8_t fill = 0;
    std::string payload;   // write data
  };
  struct Result {
    int status = kIoFailed;  // IoStatus
    bool has_data = false;   // successful read
    std::string data;
  };

  explicit IoQueue(BdevPtr bdev);

  // "batched" / "persistent" / "shared" for HBM channels (read from the
  // channel's own kind tag), "cpu" for bdevs without a device base.
  const char* kind() const;

  // Submits every op in order before the first poll(), then polls
  // until all completions fired. Requests go to the engine exactly as
  // given (no chunking, no validation). One pinned arena per call
  // carries write payloads in and read results out; it is kept and
  // reused (grown when a call needs more) and only freed with the
  // queue: hipHostFree waits for the device to go idle, so freeing
  // after every call would stall ~1 s on a resident service kernel
  // and force it through idle-exit + relaunch between any two calls.
  // The wait is bounded by the sync-I/O timeout; on expiry this throws
  // and leaks the arena (a descriptor may still point into it).
  std::vector<Result> run(const std::vector<Op>& ops);

  ~IoQueue();
  IoQueue(const IoQueue&) = delete;
  IoQueue& operator=(const IoQueue&) = delete;

 private:
  uint8_t* acquire_arena(uint64_t bytes);

  BdevPtr bdev_;
  std::shared_ptr<IoChannel> channel_;
  uint8_t* arena_ = nullptr;
  uint64_t arena_capacity_ = 0;
  std::vector<void*> retired_;  // outgrown arenas, freed with the queue
  bool busy_ = false;           // a run() left requests outstanding
};

// fio-shaped benchmark harness (SPDK bdevperf analog): `workload` is
// randread / randwrite / randrw; runs num_queues submitter threads each
// holding queue_depth I/Os in flight for `seconds`, then reports
// latency percentiles measured per-I/O.
struct PerfResult {
  double seconds = 0;
  uint64_t io_count = 0;
  double iops = 0;
  double throughput_mbps = 0;
  double lat_avg_us = 0;
  double lat_p50_us = 0;
  double lat_p90_us = 0;
  double lat_p99_us = 0;
  double lat_p999_us = 0;
  double lat_max_us = 0;
};

PerfResult run_bdevperf(Bdev* bdev, const std::string& workload,
                        uint32_t io_size, uint32_t queue_depth,
                        int num_queues, double seconds,
                        uint64_t max_ios = 0);

// Persistent-queue variant for stepped benchmarking (bench.py): queue
// threads, their I/O channels (HIP streams + pinned rings) and buffers
// live across step() calls, so a step measures steady-state IOPS
// without per-call setup.
class PerfSession {
 public:
  PerfSession(BdevPtr bdev, std::string workload, uint32_t io_size,
              uint32_t queue_depth, int num_queues);
  ~PerfSession();

  // Run until `total_ios` I/Os complete (spread over the queues);
  // returns the step's aggregate stats.
  PerfResult step(uint64_t total_ios);

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
};

}  // namespace hipstore
