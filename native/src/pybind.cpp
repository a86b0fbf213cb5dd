// Python bindings over the hipstore C++/HIP core (oim_amd._hipstore).
//
// Used by tests, the fio-shaped benchmark harness (bench.py) and the
// CSI driver's local mode. The daemon (hipstored) links the same core,
// so everything measured through these bindings is the same code the
// control plane drives over JSON-RPC.

#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <numeric>
#include <chrono>
#include <optional>
#include <stdexcept>

#include "hipstore/bdev.h"
#include "hipstore/composite.h"
#include "hipstore/crc32c.h"
#include "hipstore/compress.h"
#include "hipstore/crypt.h"
#include "hipstore/delta.h"
#include "hipstore/engine.h"
#include "hipstore/fingerprint.h"
#include "hipstore/nvmf.h"
#include "hipstore/parity.h"
#include "hipstore/rados.h"
#include "hipstore/vhost_master.h"

namespace py = pybind11;
using namespace hipstore;

namespace {

py::bytes bdev_read_py(Bdev& bdev, uint64_t offset, uint64_t length) {
  void* bounce = alloc_pinned(length);
  int status = bdev_read_sync(&bdev, offset, bounce, length);
  if (status != kIoOk) {
    free_pinned(bounce);
    throw std::runtime_error("bdev read failed: status " + std::to_string(status));
  }
  py::bytes out(static_cast<const char*>(bounce), length);
  free_pinned(bounce);
  return out;
}

void bdev_write_py(Bdev& bdev, uint64_t offset, py::buffer data) {
  py::buffer_info info = data.request();
  const uint64_t length = static_cast<uint64_t>(info.size) * info.itemsize;
  void* bounce = alloc_pinned(length);
  memcpy(bounce, info.ptr, length);
  int status = bdev_write_sync(&bdev, offset, bounce, length);
  free_pinned(bounce);
  if (status != kIoOk) {
    throw std::runtime_error("bdev write failed: status " + std::to_string(status));
  }
}

void bdev_fill_py(Bdev& bdev, uint64_t offset, int value, uint64_t length) {
  int status = bdev_fill_sync(&bdev, offset, static_cast<uint8_t>(value), length);
  if (status != kIoOk) {
    throw std::runtime_error("bdev fill failed: status " + std::to_string(status));
  }
}

// ("read", offset, length) / ("write", offset, bytes) /
// ("fill", offset, length, value) / ("flush",) -> IoQueue::Op. No
// validation of the request itself: that is the engine's job.
IoQueue::Op io_op_from_tuple(const py::tuple& t) {
  if (t.empty()) throw std::invalid_argument("IoQueue: empty op tuple");
  const std::string name = t[0].cast<std::string>();
  IoQueue::Op op;
  if (name == "read" && t.size() == 3) {
    op.op = IoOp::kRead;
    op.offset = t[1].cast<uint64_t>();
    op.length = t[2].cast<uint64_t>();
  } else if (name == "write" && t.size() == 3) {
    op.op = IoOp::kWrite;
    op.offset = t[1].cast<uint64_t>();
    py::buffer_info info = t[2].cast<py::buffer>().request();
    op.payload.assign(static_cast<const char*>(info.ptr),
                      static_cast<size_t>(info.size) * info.itemsize);
    op.length = op.payload.size();
  } else if (name == "fill" && t.size() == 4) {
    op.op = IoOp::kFill;
    op.offset = t[1].cast<uint64_t>();
    op.length = t[2].cast<uint64_t>();
    op.fill = static_cast<uint8_t>(t[3].cast<int>());
  } else if (name == "flush" && t.size() == 1) {
    op.op = IoOp::kFlush;
  } else {
    throw std::invalid_argument("IoQueue: unknown op tuple '" + name + "'");
  }
  return op;
}

py::list io_queue_run_py(IoQueue& q, const py::list& ops_py) {
  std::vector<IoQueue::Op> ops;
  ops.reserve(ops_py.size());
  for (py::handle item : ops_py) {
    ops.push_back(io_op_from_tuple(item.cast<py::tuple>()));
  }
  std::vector<IoQueue::Result> results;
  {
    py::gil_scoped_release release;
    results = q.run(ops);
  }
  py::list out;
  for (const IoQueue::Result& r : results) {
    if (r.has_data) {
      out.append(py::make_tuple(r.status, py::bytes(r.data)));
    } else {
      out.append(py::make_tuple(r.status, py::none()));
    }
  }
  return out;
}

py::dict perf_to_dict(const PerfResult& r) {
  py::dict d;
  d["seconds"] = r.seconds;
  d["io_count"] = r.io_count;
  d["iops"] = r.iops;
  d["throughput_mbps"] = r.throughput_mbps;
  d["lat_avg_us"] = r.lat_avg_us;
  d["lat_p50_us"] = r.lat_p50_us;
  d["lat_p90_us"] = r.lat_p90_us;
  d["lat_p99_us"] = r.lat_p99_us;
  d["lat_p999_us"] = r.lat_p999_us;
  d["lat_max_us"] = r.lat_max_us;
  return d;
}

// Bitmap bytes (granule g is byte g//8, bit g%8) -> bdev_diff_sync words.
std::vector<uint64_t> bitmap_words(const std::string& raw) {
  std::vector<uint64_t> words((raw.size() + 7) / 8, 0);
  for (size_t i = 0; i < raw.size(); ++i) {
    words[i / 8] |= static_cast<uint64_t>(static_cast<uint8_t>(raw[i]))
                    << (8 * (i % 8));
  }
  return words;
}

// Throws when `bitmap` (bytes) does not cover `length / granule`
// granules; the core validates the rest.
void check_bitmap_covers(const char* what, uint64_t length, uint32_t granule,
                         const std::string& bitmap) {
  if (granule == 0) return;
  const uint64_t n_granules = length / granule;
  if (bitmap.size() < n_granules / 8 + (n_granules % 8 != 0)) {
    throw std::runtime_error(std::string(what) +
                             ": bitmap shorter than range");
  }
}

// Range of the pack / unpack bindings: length None = to the end of the
// device, rounded down to whole granules. Throws when the bitmap does
// not cover it.
uint64_t marked_range(const char* what, Bdev& bdev, uint64_t offset,
                      std::optional<uint64_t> length, uint32_t granule,
                      const std::string& bitmap) {
  uint64_t len = 0;
  if (length) {
    len = *length;
  } else if (granule != 0 && offset <= bdev.size_bytes()) {
    len = (bdev.size_bytes() - offset) / granule * granule;
  }
  check_bitmap_covers(what, len, granule, bitmap);
  return len;
}

py::dict delta_info_to_dict(const DeltaInfo& info) {
  py::dict d;
  d["version"] = info.version;
  d["block_size"] = info.block_size;
  d["granule"] = info.granule;
  d["full"] = info.full;
  d["volume_bytes"] = info.volume_bytes;
  d["granules"] = info.n_granules;
  d["marked"] = info.n_marked;
  d["file_bytes"] = info.file_bytes;
  if (info.compressed) {  // version 1 keeps the keys it always had
    d["compressed"] = true;
    d["stored_bytes"] = info.stored_bytes;
  }
  if (info.encrypted) d["encrypted"] = true;
  if (info.dictionary) d["dictionary"] = true;
  return d;
}

// A key argument of the delta bindings: None = no key. Any length gets
// through; the core refuses what is not an HSXTS1 key.
struct KeyArg {
  std::vector<uint8_t> bytes;
  bool given = false;

  explicit KeyArg(const std::optional<py::bytes>& key) : given(key.has_value()) {
    if (given) {
      const std::string raw = *key;
      bytes.assign(raw.begin(), raw.end());
    }
  }
  ~KeyArg() {
    if (!bytes.empty()) explicit_bzero(bytes.data(), bytes.size());
  }
  const std::vector<uint8_t>* ptr() const { return given ? &bytes : nullptr; }
  // For the marked calls; None is no key.
  XtsKey xts(uint64_t first_unit) const {
    return {given ? bytes.data() : nullptr, bytes.size(), first_unit};
  }
};

// Marks of `words` below granule n_granules.
uint64_t marks_below(const std::vector<uint64_t>& words, uint64_t n_granules) {
  uint64_t marked = 0;
  for (uint64_t w = 0; w < n_granules / 64; ++w) {
    marked += static_cast<uint64_t>(__builtin_popcountll(words[w]));
  }
  if (n_granules % 64 != 0) {
    marked += static_cast<uint64_t>(__builtin_popcountll(
        words[n_granules / 64] & ((1ull << (n_granules % 64)) - 1)));
  }
  return marked;
}

// The whole-granule argument of the host codec bindings.
void check_units(const char* what, const std::string& data, uint32_t granule,
                 const std::string& key) {
  if (!xts_granule_ok(granule) || data.size() % granule != 0) {
    throw std::invalid_argument(std::string(what) +
                                ": granule must be a multiple of 16, at most "
                                "2^24, that divides the data length");
  }
  if (!xts_key_ok(reinterpret_cast<const uint8_t*>(key.data()), key.size())) {
    throw std::invalid_argument(std::string(what) +
                                ": the key must be 64 bytes whose halves "
                                "differ");
  }
}

py::dict map_info_to_dict(const FingerprintMapInfo& info) {
  py::dict d;
  d["version"] = info.version;
  d["block_size"] = info.block_size;
  d["granule"] = info.granule;
  d["algorithm"] = info.algorithm;
  d["volume_bytes"] = info.volume_bytes;
  d["granules"] = info.n_granules;
  d["file_bytes"] = info.file_bytes;
  // version 1 keeps the keys it always had
  if (info.version != kFingerprintMapVersion) d["keyed"] = info.keyed;
  return d;
}

// The map_algorithm / map_key arguments: None leaves the algorithm open.
MapKind map_kind(const std::optional<std::string>& algorithm,
                 const KeyArg& key) {
  MapKind kind;
  if (algorithm.has_value()) {
    if (*algorithm == "hsfp1") {
      kind.algorithm = kMapHsfp1;
    } else if (*algorithm == "blake2s") {
      kind.algorithm = kMapBlake2s;
    } else {
      throw std::invalid_argument(
          "map_algorithm must be \"hsfp1\" or \"blake2s\"");
    }
  }
  kind.key = key.ptr();
  return kind;
}

// The algorithm / key arguments of the fingerprint calls.
FingerprintKind fingerprint_kind(uint32_t algorithm, const KeyArg& key) {
  FingerprintKind kind;
  kind.algorithm = algorithm;
  if (key.given) {
    kind.key = key.bytes.data();
    kind.key_bytes = key.bytes.size();
  }
  return kind;
}

// Runs a call of the delta layer (delta.h), which takes the error string
// and returns a status, with the GIL released; kIoInvalid becomes
// ValueError, any other failure RuntimeError.
template <typename Call>
void delta_call(const char* what, Call call) {
  std::string error;
  int status;
  {
    py::gil_scoped_release release;
    status = call(&error);
  }
  if (status == kIoOk) return;
  const std::string text = std::string(what) + ": " + error + " (status " +
                           std::to_string(status) + ")";
  if (status == kIoInvalid) throw std::invalid_argument(text);
  throw std::runtime_error(text);
}

// The member set of the parity bindings. `offsets` empty = all zero;
// length 0 = what is left of the shortest member, in whole `unit`s.
struct ParityArgs {
  std::vector<ParityMember> data;
  ParityMember p;
  ParityMember q;
  uint64_t length = 0;
};

ParityArgs parity_args(const std::vector<BdevPtr>& data, const BdevPtr& p,
                       const BdevPtr& q,
                       const std::vector<uint64_t>& data_offsets,
                       uint64_t p_offset, uint64_t q_offset, uint64_t length,
                       uint64_t unit) {
  if (!data_offsets.empty() && data_offsets.size() != data.size()) {
    throw std::invalid_argument("parity: one offset per data member");
  }
  ParityArgs args;
  for (size_t i = 0; i < data.size(); ++i) {
    if (!data[i]) throw std::invalid_argument("parity: data member is None");
    args.data.push_back(
        {data[i].get(), data_offsets.empty() ? 0 : data_offsets[i]});
  }
  args.p = {p.get(), p_offset};
  args.q = {q.get(), q_offset};
  if (length == 0 && !data.empty()) {
    if (unit == 0) unit = std::lcm<uint64_t>(data[0]->block_size(), 16);
    length = parity_common_length(args.data, args.p, args.q, unit);
  }
  args.length = length;
  return args;
}

// kIoInvalid becomes ValueError, any other failure RuntimeError; the
// text names the rule that was broken.
void parity_raise(const char* what, int status, const ParityReport& report) {
  if (status == kIoOk) return;
  const std::string text = std::string(what) + ": " + report.error +
                           " (status " + std::to_string(status) + ")";
  if (status == kIoInvalid) throw std::invalid_argument(text);
  throw std::runtime_error(text);
}

// Little-endian bytes: granule g is byte g//8, bit g%8.
py::bytes bitmap_bytes(const std::vector<uint64_t>& words, uint64_t granules) {
  std::string raw((granules + 7) / 8, '\0');
  for (size_t i = 0; i < raw.size(); ++i) {
    raw[i] = static_cast<char>((words[i / 8] >> (8 * (i % 8))) & 0xFF);
  }
  return py::bytes(raw);
}

py::dict parity_stats_dict(const DiffStats& stats,
                           const std::vector<uint64_t>& words) {
  py::dict d;
  d["granules"] = stats.granules;
  d["mismatched"] = stats.mismatched;
  d["first_mismatches"] = stats.first_mismatches;
  d["bitmap"] = bitmap_bytes(words, stats.granules);
  return d;
}

}  // namespace

PYBIND11_MODULE(_hipstore, m) {
  m.doc() = "MI355X hipstore data-path core (HBM bdevs, LDS-staged block I/O)";

  m.def("gpu_available", &gpu_available);
  m.def("gpu_device_count", &gpu_device_count);
  m.def("gpu_pci_address", &gpu_pci_address, py::arg("device"));

  py::class_<Bdev, BdevPtr>(m, "Bdev")
      .def_property_readonly("name", &Bdev::name)
      .def_property_readonly("product_name", &Bdev::product_name)
      .def_property_readonly("uuid", &Bdev::uuid)
      .def_property_readonly("block_size", &Bdev::block_size)
      .def_property_readonly("num_blocks", &Bdev::num_blocks)
      .def_property_readonly("size_bytes", &Bdev::size_bytes)
      .def("resize",
           [](hipstore::Bdev& b, uint64_t num_blocks) {
             return b.resize(num_blocks);
           },
           py::arg("num_blocks"))
      .def("iostat",
           [](const hipstore::Bdev& b) {
             // The get_bdevs_iostat RPC's counters, by the same names.
             const hipstore::Bdev::IoStat st = b.iostat();
             py::dict d;
             d["num_read_ops"] = st.num_read_ops;
             d["num_write_ops"] = st.num_write_ops;
             d["num_unmap_ops"] = st.num_unmap_ops;
             d["bytes_read"] = st.bytes_read;
             d["bytes_written"] = st.bytes_written;
             return d;
           })
      .def("read", &bdev_read_py, py::arg("offset"), py::arg("length"),
           py::call_guard<py::gil_scoped_release>())
      .def("write", &bdev_write_py, py::arg("offset"), py::arg("data"))
      .def("fill", &bdev_fill_py, py::arg("offset"), py::arg("value"),
           py::arg("length"), py::call_guard<py::gil_scoped_release>());

  m.def("create_malloc_bdev", &create_malloc_bdev, py::arg("name"),
        py::arg("block_size"), py::arg("num_blocks"));
  m.def("create_hbm_bdev", &create_hbm_bdev, py::arg("name"),
        py::arg("block_size"), py::arg("num_blocks"), py::arg("device") = 0,
        py::arg("persistent") = false);
  m.def("create_file_bdev", &create_file_bdev, py::arg("name"),
        py::arg("path"), py::arg("block_size") = 512);
  m.def("create_striped_bdev", &create_striped_bdev, py::arg("name"),
        py::arg("children"), py::arg("stripe_size") = 131072);
  m.def("create_replicated_bdev", &create_replicated_bdev, py::arg("name"),
        py::arg("children"));

  py::class_<RadosCluster, std::shared_ptr<RadosCluster>>(m, "RadosCluster")
      .def("port", &RadosCluster::port)
      .def("object_count", &RadosCluster::object_count)
      .def("stop", &RadosCluster::stop,
           py::call_guard<py::gil_scoped_release>());
  m.def("start_rados_cluster", &start_rados_cluster, py::arg("port") = 0,
        py::arg("arena_mb") = 512, py::arg("use_hbm") = false,
        py::arg("device") = 0, py::arg("object_bytes") = 4ull << 20);
  m.def("create_rbd_bdev", &create_rbd_bdev, py::arg("name"),
        py::arg("mon_host"), py::arg("pool"), py::arg("image"),
        py::arg("block_size") = 512,
        py::arg("default_size_bytes") = 64ull << 20,
        py::arg("object_bytes") = 4ull << 20);

  py::class_<NvmfTcpTarget, std::shared_ptr<NvmfTcpTarget>>(m, "NvmfTcpTarget")
      .def_property_readonly("port", &NvmfTcpTarget::port)
      .def("add_namespace", &NvmfTcpTarget::add_namespace, py::arg("bdev"))
      .def("stop", &NvmfTcpTarget::stop,
           py::call_guard<py::gil_scoped_release>());
  m.def("start_nvmf_tcp_target", &start_nvmf_tcp_target,
        py::arg("listen_addr") = "", py::arg("port") = 0,
        py::arg("subnqn") = "nqn.2026-01.com.amd:oim-amd",
        py::arg("enable_digests") = true);
  m.def("create_nvmf_tcp_bdev", &create_nvmf_tcp_bdev, py::arg("name"),
        py::arg("traddr"), py::arg("trsvcid"), py::arg("subnqn"),
        py::arg("nsid") = 1, py::arg("enable_digests") = true,
        py::call_guard<py::gil_scoped_release>());

  py::class_<VhostMasterSession>(m, "VhostMasterSession")
      .def(py::init<const std::string&, const std::string&, int, int,
                    uint32_t, uint32_t, uint64_t>(),
           py::arg("socket_path"), py::arg("personality") = "scsi",
           py::arg("num_rings") = 4, py::arg("iodepth") = 32,
           py::arg("io_size") = 4096, py::arg("block_size") = 512,
           py::arg("capacity_bytes") = 0,
           py::call_guard<py::gil_scoped_release>())
      .def("run", [](VhostMasterSession& s, uint64_t total_ios,
                     const std::string& workload) {
        PerfResult r;
        {
          py::gil_scoped_release release;
          r = s.run(total_ios, workload);
        }
        return perf_to_dict(r);
      }, py::arg("total_ios"), py::arg("workload") = "randread");

  m.def(
      "vhost_master_bench",
      [](const std::string& socket_path, const std::string& personality,
         int num_rings, int iodepth, uint32_t io_size,
         const std::string& workload, uint64_t total_ios,
         uint32_t block_size, uint64_t capacity_bytes) {
        PerfResult r;
        {
          py::gil_scoped_release release;
          r = vhost_master_bench(socket_path, personality, num_rings,
                                 iodepth, io_size, workload, total_ios,
                                 block_size, capacity_bytes);
        }
        return perf_to_dict(r);
      },
      py::arg("socket_path"), py::arg("personality") = "scsi",
      py::arg("num_rings") = 4, py::arg("iodepth") = 32,
      py::arg("io_size") = 4096, py::arg("workload") = "randread",
      py::arg("total_ios") = 100000, py::arg("block_size") = 512,
      py::arg("capacity_bytes") = 0);

  py::class_<IoQueue>(m, "IoQueue",
                      "Queued I/O on one long-lived channel (tests): run() "
                      "submits every op before the first poll")
      .def(py::init<BdevPtr>(), py::arg("bdev"))
      .def_property_readonly("kind", &IoQueue::kind)
      .def("run", &io_queue_run_py, py::arg("ops"));

  py::class_<PerfSession>(m, "PerfSession")
      .def(py::init<BdevPtr, std::string, uint32_t, uint32_t, int>(),
           py::arg("bdev"), py::arg("workload") = "randread",
           py::arg("io_size") = 4096, py::arg("queue_depth") = 32,
           py::arg("num_queues") = 8)
      .def("step", [](PerfSession& s, uint64_t total_ios) {
        PerfResult r;
        {
          py::gil_scoped_release release;
          r = s.step(total_ios);
        }
        return perf_to_dict(r);
      }, py::arg("total_ios"));

  m.def(
      "run_bdevperf",
      [](BdevPtr bdev, const std::string& workload, uint32_t io_size,
         uint32_t queue_depth, int num_queues, double seconds,
         uint64_t max_ios) {
        PerfResult r;
        {
          py::gil_scoped_release release;
          r = run_bdevperf(bdev.get(), workload, io_size, queue_depth,
                           num_queues, seconds, max_ios);
        }
        return perf_to_dict(r);
      },
      py::arg("bdev"), py::arg("workload") = "randread",
      py::arg("io_size") = 4096, py::arg("queue_depth") = 32,
      py::arg("num_queues") = 1, py::arg("seconds") = 2.0,
      py::arg("max_ios") = 0);

  m.def("hbm_info", [](int device) {
    auto [total, free_bytes] = hbm_info(device);
    return py::make_tuple(total, free_bytes);
  }, py::arg("device") = 0);

  m.def("hbm_copy", [](BdevPtr src, uint64_t src_offset, BdevPtr dst,
                       uint64_t dst_offset, uint64_t length) {
    int status;
    {
      py::gil_scoped_release release;
      status = hbm_copy_sync(src.get(), src_offset, dst.get(), dst_offset,
                             length);
    }
    if (status != kIoOk) {
      throw std::runtime_error("hbm_copy failed: status " +
                               std::to_string(status));
    }
  }, py::arg("src"), py::arg("src_offset"), py::arg("dst"),
     py::arg("dst_offset"), py::arg("length"),
     "Device-side range copy between HBM bdevs (LDS-staged kernel "
     "same-device, xGMI peer copy cross-device)");

  m.def("bdev_diff", [](BdevPtr a, BdevPtr b, uint64_t a_offset,
                        uint64_t b_offset, uint64_t length, uint32_t granule,
                        uint32_t max_report) {
    if (granule == 0) granule = static_cast<uint32_t>(a->block_size());
    if (length == 0) length = bdev_common_length(a.get(), a_offset, b.get(),
                                                     b_offset, granule);
    std::vector<uint64_t> bitmap;
    DiffStats stats;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_diff_sync(a.get(), a_offset, b.get(), b_offset, length,
                              granule, max_report, &bitmap, &stats);
    }
    if (status != kIoOk) {
      throw std::runtime_error("bdev_diff failed: status " +
                               std::to_string(status));
    }
    // Little-endian bytes: granule g is byte g//8, bit g%8.
    const size_t n_bytes = (stats.granules + 7) / 8;
    std::string raw(n_bytes, '\0');
    for (size_t i = 0; i < n_bytes; ++i) {
      raw[i] = static_cast<char>((bitmap[i / 8] >> (8 * (i % 8))) & 0xFF);
    }
    py::dict d;
    d["granules"] = stats.granules;
    d["mismatched"] = stats.mismatched;
    d["first_mismatches"] = stats.first_mismatches;
    d["bitmap"] = py::bytes(raw);
    return d;
  }, py::arg("a"), py::arg("b"), py::arg("a_offset") = 0,
     py::arg("b_offset") = 0, py::arg("length") = 0, py::arg("granule") = 0,
     py::arg("max_report") = 16,
     "Granule-wise compare of two bdev ranges (on-GPU for HBM pairs). "
     "length=0: up to the end of the shorter device; granule=0: the "
     "block size");

  m.def("bdev_copy_marked", [](BdevPtr src, BdevPtr dst, py::bytes bitmap,
                               uint32_t granule, uint64_t src_offset,
                               uint64_t dst_offset, uint64_t length) {
    if (granule == 0) granule = static_cast<uint32_t>(src->block_size());
    if (length == 0) length = bdev_common_length(src.get(), src_offset, dst.get(),
                                                     dst_offset, granule);
    const std::string raw = bitmap;
    check_bitmap_covers("bdev_copy_marked", length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    uint64_t copied = 0;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_copy_marked_sync(src.get(), src_offset, dst.get(),
                                     dst_offset, length, granule, words,
                                     &copied);
    }
    if (status != kIoOk) {
      throw std::runtime_error("bdev_copy_marked failed: status " +
                               std::to_string(status));
    }
    return copied;
  }, py::arg("src"), py::arg("dst"), py::arg("bitmap"), py::arg("granule"),
     py::arg("src_offset") = 0, py::arg("dst_offset") = 0,
     py::arg("length") = 0,
     "Copy only the granules marked in `bitmap` (bdev_diff layout); "
     "returns the number copied");

  m.def("bdev_pack_marked", [](BdevPtr src, py::bytes bitmap, uint32_t granule,
                               uint64_t src_offset,
                               std::optional<uint64_t> length,
                               uint64_t staging_bytes) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_pack_marked", *src, src_offset,
                                      length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    std::string out;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_pack_marked_sync(
          src.get(), src_offset, len, granule, words, staging_bytes,
          [&out, granule](const uint8_t* data, uint64_t, uint64_t count) {
            out.append(reinterpret_cast<const char*>(data), count * granule);
            return 0;
          });
    }
    if (status != kIoOk) {
      throw std::runtime_error("bdev_pack_marked failed: status " +
                               std::to_string(status));
    }
    return py::bytes(out);
  }, py::arg("src"), py::arg("bitmap"), py::arg("granule"),
     py::arg("src_offset") = 0, py::arg("length") = py::none(),
     py::arg("staging_bytes") = 0,
     "Gather the granules marked in `bitmap` (bdev_diff layout) into one "
     "dense bytes object, ascending (on-GPU for HBM bdevs)");

  m.def("bdev_unpack_marked", [](BdevPtr dst, py::bytes bitmap,
                                 uint32_t granule, py::bytes data,
                                 uint64_t dst_offset,
                                 std::optional<uint64_t> length,
                                 uint64_t staging_bytes) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_unpack_marked", *dst, dst_offset,
                                      length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const std::string dense = data;
    if (granule != 0) {
      const uint64_t marked = marks_below(words, len / granule);
      if (dense.size() != marked * granule) {
        throw std::runtime_error(
            "bdev_unpack_marked: data length " + std::to_string(dense.size()) +
            " is not marked * granule = " + std::to_string(marked * granule));
      }
    }
    uint64_t unpacked = 0;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_unpack_marked_sync(
          dst.get(), dst_offset, len, granule, words, staging_bytes,
          [&dense, granule](uint8_t* out, uint64_t first_rank,
                            uint64_t count) {
            memcpy(out, dense.data() + first_rank * granule, count * granule);
            return 0;
          },
          &unpacked);
    }
    if (status != kIoOk) {
      throw std::runtime_error("bdev_unpack_marked failed: status " +
                               std::to_string(status));
    }
    return unpacked;
  }, py::arg("dst"), py::arg("bitmap"), py::arg("granule"), py::arg("data"),
     py::arg("dst_offset") = 0, py::arg("length") = py::none(),
     py::arg("staging_bytes") = 0,
     "Scatter a dense bytes object to the granules marked in `bitmap`; "
     "returns the number written");

  m.def("marked_copy_probe", [](BdevPtr src, py::bytes bitmap,
                                uint32_t granule, int mode,
                                uint64_t ring_bytes, uint64_t staging_bytes) {
    const std::vector<uint64_t> words = bitmap_words(bitmap);
    MarkedCopyProbe probe;
    int status;
    {
      py::gil_scoped_release release;
      status = marked_copy_probe(src.get(), granule, words, mode, ring_bytes,
                                 staging_bytes, &probe);
    }
    if (status != kIoOk) {
      throw std::runtime_error("marked_copy_probe failed: status " +
                               std::to_string(status));
    }
    py::dict d;
    d["seconds"] = probe.seconds;
    d["granules"] = probe.granules;
    d["calls"] = probe.calls;
    return d;
  }, py::arg("src"), py::arg("bitmap"), py::arg("granule"), py::arg("mode"),
     py::arg("ring_bytes") = 1ull << 30, py::arg("staging_bytes") = 0,
     "Measurement aid (tools/delta_bench.py): marked bytes to pinned host "
     "memory by one hipMemcpyAsync (0), one per run (1) or the pack "
     "kernel with a discarding sink (2)");

  m.def("bdev_export_delta", [](BdevPtr src, const std::string& path,
                                std::optional<BdevPtr> base,
                                std::optional<uint32_t> granule,
                                bool overwrite,
                                std::optional<std::string> base_map,
                                std::optional<std::string> map_out,
                                bool compress, std::optional<py::bytes> key,
                                std::optional<std::string> map_algorithm,
                                std::optional<py::bytes> map_key,
                                bool dictionary, bool cts) {
    DeltaInfo info;
    DeltaMaps maps;
    const KeyArg key_arg(key);
    const KeyArg map_key_arg(map_key);
    maps.kind = map_kind(map_algorithm, map_key_arg);
    maps.base_map = base_map.value_or("");
    maps.map_out = map_out.value_or("");
    delta_call("bdev_export_delta", [&](std::string* error) {
      return bdev_export_delta(src.get(), base ? base->get() : nullptr, path,
                               granule.value_or(0), overwrite, &maps, &info,
                               error, compress, key_arg.ptr(), dictionary,
                               cts);
    });
    py::dict d = delta_info_to_dict(info);
    if (!maps.map_out.empty()) d["map_bytes"] = maps.map_bytes;
    return d;
  }, py::arg("src"), py::arg("path"), py::arg("base") = py::none(),
     py::arg("granule") = py::none(), py::arg("overwrite") = false,
     py::arg("base_map") = py::none(), py::arg("map_out") = py::none(),
     py::arg("compress") = false, py::arg("key") = py::none(),
     py::arg("map_algorithm") = py::none(), py::arg("map_key") = py::none(),
     py::arg("dictionary") = false, py::arg("cts") = false,
     "Write the granules of src that differ from base, or from the state "
     "recorded in the fingerprint map base_map (every granule without "
     "either), to a hipstore delta file; map_out also writes the "
     "fingerprint map of src; compress writes a version-2 file of HSLZ1 "
     "pieces, key (64 bytes) a version-3 file of HSXTS1 ciphertext; "
     "map_algorithm \"blake2s\" and map_key (32 bytes) make map_out an "
     "HSFP2 map (base_map decides by itself); dictionary (with compress "
     "and base) a version-4 file of HSLZD1 pieces, every granule "
     "compressed against the same granule of base; cts (with compress "
     "and key, with or without dictionary) a version-5 file whose pieces "
     "are HSXTS2 ciphertext (ciphertext stealing)");

  m.def("xts_encrypt_units", [](py::bytes data, uint32_t granule,
                                py::bytes key, uint64_t first_unit) {
    const std::string in = data;
    const std::string raw_key = key;
    check_units("xts_encrypt_units", in, granule, raw_key);
    const XtsSchedules keys(reinterpret_cast<const uint8_t*>(raw_key.data()));
    std::string out(in.size(), '\0');
    for (uint64_t i = 0; i < in.size() / granule; ++i) {
      xts_encrypt_unit(keys, first_unit + i,
                       reinterpret_cast<const uint8_t*>(in.data()) + i * granule,
                       reinterpret_cast<uint8_t*>(&out[0]) + i * granule,
                       granule);
    }
    return py::bytes(out);
  }, py::arg("data"), py::arg("granule"), py::arg("key"),
     py::arg("first_unit") = 0,
     "HSXTS1 (AES-256-XTS) over whole granules, data unit i numbered "
     "first_unit + i (host codec, the byte model of k_xts_pack_marked)");

  m.def("xts_decrypt_units", [](py::bytes data, uint32_t granule,
                                py::bytes key, uint64_t first_unit) {
    const std::string in = data;
    const std::string raw_key = key;
    check_units("xts_decrypt_units", in, granule, raw_key);
    const XtsSchedules keys(reinterpret_cast<const uint8_t*>(raw_key.data()));
    std::string out(in.size(), '\0');
    for (uint64_t i = 0; i < in.size() / granule; ++i) {
      xts_decrypt_unit(keys, first_unit + i,
                       reinterpret_cast<const uint8_t*>(in.data()) + i * granule,
                       reinterpret_cast<uint8_t*>(&out[0]) + i * granule,
                       granule);
    }
    return py::bytes(out);
  }, py::arg("data"), py::arg("granule"), py::arg("key"),
     py::arg("first_unit") = 0, "The inverse of xts_encrypt_units (host codec)");

  m.def("xts_kcv", [](py::bytes key) {
    const std::string raw_key = key;
    check_units("xts_kcv", "", 16, raw_key);
    return xts_kcv(reinterpret_cast<const uint8_t*>(raw_key.data()));
  }, py::arg("key"),
     "Key check value of an HSXTS1 key, as in a version-3 delta header");

  // HSXTS2: one unit of any length >= 16 (ciphertext stealing).
  const auto xts_var = [](const char* what, bool encrypt, py::bytes data,
                          py::bytes key, uint64_t unit) {
    const std::string in = data;
    const std::string raw_key = key;
    check_units(what, "", 16, raw_key);
    if (in.size() < 16 || in.size() > kXtsMaxGranule) {
      throw std::invalid_argument(std::string(what) +
                                  ": 16 <= length <= 2^24");
    }
    const XtsSchedules keys(reinterpret_cast<const uint8_t*>(raw_key.data()));
    std::string out(in.size(), '\0');
    (encrypt ? xts_encrypt_var : xts_decrypt_var)(
        keys, unit, reinterpret_cast<const uint8_t*>(in.data()),
        reinterpret_cast<uint8_t*>(&out[0]), static_cast<uint32_t>(in.size()));
    return py::bytes(out);
  };
  m.def("xts_encrypt_var", [xts_var](py::bytes data, py::bytes key,
                                     uint64_t unit) {
    return xts_var("xts_encrypt_var", true, data, key, unit);
  }, py::arg("data"), py::arg("key"), py::arg("unit") = 0,
     "HSXTS2-encrypt `data` (16 bytes or more, any length) as data unit "
     "`unit` with ciphertext stealing (host codec, the byte model of "
     "k_xts_var)");
  m.def("xts_decrypt_var", [xts_var](py::bytes data, py::bytes key,
                                     uint64_t unit) {
    return xts_var("xts_decrypt_var", false, data, key, unit);
  }, py::arg("data"), py::arg("key"), py::arg("unit") = 0,
     "Inverse of xts_encrypt_var");

  m.def("bdev_xts_pack_marked", [](BdevPtr src, py::bytes bitmap,
                                   uint32_t granule, py::bytes key,
                                   uint64_t first_unit, uint64_t src_offset,
                                   std::optional<uint64_t> length,
                                   uint64_t staging_bytes) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_xts_pack_marked", *src, src_offset,
                                      length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const KeyArg key_arg(key);
    std::string out;
    delta_call("bdev_xts_pack_marked", [&](std::string* error) {
      *error = "bad key, granule, range or first_unit, or the pack failed";
      return bdev_xts_pack_marked_sync(
          src.get(), src_offset, len, granule, words, key_arg.xts(first_unit),
          staging_bytes,
          [&out, granule](const uint8_t* data, uint64_t, uint64_t count) {
            out.append(reinterpret_cast<const char*>(data), count * granule);
            return 0;
          });
    });
    return py::bytes(out);
  }, py::arg("src"), py::arg("bitmap"), py::arg("granule"), py::arg("key"),
     py::arg("first_unit") = 0, py::arg("src_offset") = 0,
     py::arg("length") = py::none(), py::arg("staging_bytes") = 0,
     "bdev_pack_marked with every granule HSXTS1-encrypted as data unit "
     "first_unit + its index in the range (k_xts_pack_marked for HBM bdevs)");

  m.def("bdev_xts_unpack_marked", [](BdevPtr dst, py::bytes bitmap,
                                     uint32_t granule, py::bytes data,
                                     py::bytes key, uint64_t first_unit,
                                     uint64_t dst_offset,
                                     std::optional<uint64_t> length,
                                     uint64_t staging_bytes) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_xts_unpack_marked", *dst,
                                      dst_offset, length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const std::string dense = data;
    if (granule != 0 &&
        dense.size() != marks_below(words, len / granule) * granule) {
      throw std::invalid_argument(
          "bdev_xts_unpack_marked: data length is not marked * granule");
    }
    const KeyArg key_arg(key);
    uint64_t unpacked = 0;
    delta_call("bdev_xts_unpack_marked", [&](std::string* error) {
      *error = "bad key, granule, range or first_unit, or the unpack failed";
      return bdev_xts_unpack_marked_sync(
          dst.get(), dst_offset, len, granule, words, key_arg.xts(first_unit),
          staging_bytes,
          [&dense, granule](uint8_t* out, uint64_t first_rank,
                            uint64_t count) {
            memcpy(out, dense.data() + first_rank * granule, count * granule);
            return 0;
          },
          &unpacked);
    });
    return unpacked;
  }, py::arg("dst"), py::arg("bitmap"), py::arg("granule"), py::arg("data"),
     py::arg("key"), py::arg("first_unit") = 0, py::arg("dst_offset") = 0,
     py::arg("length") = py::none(), py::arg("staging_bytes") = 0,
     "Decrypt the ciphertext of bdev_xts_pack_marked into the granules "
     "marked in `bitmap` (k_xts_unpack_marked for HBM bdevs); returns the "
     "number written");

  m.def("lz_compress_granule", [](py::bytes data,
                                  std::optional<py::bytes> dictionary) {
    const std::string in = data;
    if (!lz_granule_ok(in.size())) {
      throw std::invalid_argument(
          "lz_compress_granule: 512 <= length <= 16384, a multiple of 16");
    }
    std::string out(in.size(), '\0');
    uint32_t size = 0;
    if (dictionary) {
      const std::string dict = *dictionary;
      if (dict.size() != in.size()) {
        throw std::invalid_argument(
            "lz_compress_granule: the dictionary must be as long as the data");
      }
      size = lz_dict_compress_granule(
          reinterpret_cast<const uint8_t*>(in.data()),
          reinterpret_cast<const uint8_t*>(dict.data()),
          static_cast<uint32_t>(in.size()),
          reinterpret_cast<uint8_t*>(&out[0]));
    } else {
      size = lz_compress_granule(reinterpret_cast<const uint8_t*>(in.data()),
                                 static_cast<uint32_t>(in.size()),
                                 reinterpret_cast<uint8_t*>(&out[0]));
    }
    out.resize(size);
    return py::bytes(out);
  }, py::arg("data"), py::arg("dictionary") = py::none(),
     "The stored form of one granule: an LZ4 block, or the granule itself "
     "when that would not be smaller (host codec, the byte model of "
     "k_lz_compress_marked); with `dictionary` (as long as the data) the "
     "HSLZD1 form, the byte model of k_lz_compress_marked<true>");

  m.def("lz_decompress_granule", [](py::bytes piece, uint32_t granule,
                                    std::optional<py::bytes> dictionary) {
    const std::string in = piece;
    std::string out(lz_granule_ok(granule) ? granule : 0, '\0');
    std::string why;
    bool ok = false;
    if (dictionary) {
      const std::string dict = *dictionary;
      if (dict.size() != out.size()) {
        throw std::invalid_argument(
            "lz_decompress_granule: the dictionary must be one granule");
      }
      ok = lz_dict_decompress_granule(
          reinterpret_cast<const uint8_t*>(in.data()), in.size(), granule,
          reinterpret_cast<const uint8_t*>(dict.data()),
          reinterpret_cast<uint8_t*>(&out[0]), &why);
    } else {
      ok = lz_decompress_granule(reinterpret_cast<const uint8_t*>(in.data()),
                                 in.size(), granule,
                                 reinterpret_cast<uint8_t*>(&out[0]), &why);
    }
    if (!ok) throw std::invalid_argument("lz_decompress_granule: " + why);
    return py::bytes(out);
  }, py::arg("piece"), py::arg("granule"), py::arg("dictionary") = py::none(),
     "Decode one stored piece (host codec), an HSLZD1 piece with its "
     "`dictionary`; ValueError for a malformed one");

  m.def("lz_validate_granule", [](py::bytes piece, uint32_t granule,
                                  bool dictionary) {
    const std::string in = piece;
    const uint8_t* p = reinterpret_cast<const uint8_t*>(in.data());
    return dictionary ? lz_dict_validate_granule(p, in.size(), granule)
                      : lz_validate_granule(p, in.size(), granule);
  }, py::arg("piece"), py::arg("granule"), py::arg("dictionary") = false,
     "True when a stored piece passes the token walk import runs; "
     "`dictionary` selects the HSLZD1 walk, which needs no dictionary bytes");

  m.def("bdev_compress_marked", [](BdevPtr src, py::bytes bitmap,
                                   uint32_t granule, uint64_t src_offset,
                                   std::optional<uint64_t> length,
                                   uint64_t staging_bytes,
                                   std::optional<BdevPtr> base,
                                   uint64_t base_offset,
                                   std::optional<py::bytes> key,
                                   uint64_t first_unit) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_compress_marked", *src, src_offset,
                                      length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const KeyArg key_arg(key);
    std::vector<uint32_t> sizes;
    std::string out;
    const CompressSink sink = [&](const uint8_t* data, const uint32_t* window,
                                  uint64_t, uint64_t count) {
      for (uint64_t i = 0; i < count; ++i) {
        // Keyed: the piece as it lies in the stream, pad included.
        const uint64_t room =
            lz_padded(key_arg.given ? std::max(window[i], 16u) : window[i]);
        out.append(reinterpret_cast<const char*>(data),
                   key_arg.given ? room : window[i]);
        data += room;
      }
      sizes.insert(sizes.end(), window, window + count);
      return 0;
    };
    delta_call("bdev_compress_marked", [&](std::string* error) {
      LzOptions options;
      options.staging_bytes = staging_bytes;
      options.key = key_arg.xts(first_unit);
      if (base) {
        options.base = base->get();
        options.base_offset = base_offset;
      }
      return bdev_compress_marked_sync(src.get(), src_offset, len, granule,
                                       words, options, sink, nullptr, error);
    });
    return py::make_tuple(sizes, py::bytes(out));
  }, py::arg("src"), py::arg("bitmap"), py::arg("granule"),
     py::arg("src_offset") = 0, py::arg("length") = py::none(),
     py::arg("staging_bytes") = 0, py::arg("base") = py::none(),
     py::arg("base_offset") = 0, py::arg("key") = py::none(),
     py::arg("first_unit") = 0,
     "Compress the granules marked in `bitmap`, ascending (on-GPU for HBM "
     "bdevs): (stored sizes, the pieces back to back). With `base`, every "
     "granule is compressed against the same granule of the range of "
     "`base` at base_offset (HSLZD1). With `key` (64 bytes) every piece is "
     "HSXTS2 ciphertext of unit first_unit + its granule's index "
     "(k_xts_var for HBM bdevs) and the second item is the stream as "
     "stored: piece i, padded with zeros to a multiple of 16 and to at "
     "least 16 bytes, after the padded pieces before it");

  m.def("bdev_decompress_marked", [](BdevPtr dst, py::bytes bitmap,
                                     uint32_t granule,
                                     std::vector<uint32_t> sizes,
                                     py::bytes data, uint64_t dst_offset,
                                     std::optional<uint64_t> length,
                                     uint64_t staging_bytes, bool dictionary,
                                     std::optional<py::bytes> key,
                                     uint64_t first_unit) {
    const std::string raw = bitmap;
    const uint64_t len = marked_range("bdev_decompress_marked", *dst,
                                      dst_offset, length, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const KeyArg key_arg(key);
    const std::string pieces = data;
    // What piece i takes of `data`: its bytes, or with a key its padded
    // room in the stream.
    const auto room = [&](uint32_t size) -> uint64_t {
      return key_arg.given ? lz_padded(std::max(size, 16u)) : size;
    };
    // Where each piece starts; sizes that overrun `data` fail below.
    std::vector<uint64_t> starts(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); ++i) {
      starts[i + 1] = starts[i] + room(sizes[i]);
    }
    if (starts.back() != pieces.size()) {
      throw std::invalid_argument(
          "bdev_decompress_marked: sizes do not add up to the data length");
    }
    uint64_t unpacked = 0;
    const DecompressSource source = [&](uint8_t* out, uint32_t* window,
                                        uint64_t first_rank, uint64_t count) {
      if (first_rank + count > sizes.size()) return static_cast<int>(kIoInvalid);
      for (uint64_t i = 0; i < count; ++i) {
        const uint32_t size = sizes[first_rank + i];
        window[i] = size;
        if (size == 0 || size > granule) continue;  // refused after us
        const uint64_t have = room(size);
        const uint64_t take = lz_padded(have);
        memcpy(out, pieces.data() + starts[first_rank + i], have);
        memset(out + have, 0, take - have);
        out += take;
      }
      return 0;
    };
    delta_call("bdev_decompress_marked", [&](std::string* error) {
      LzOptions options;
      options.staging_bytes = staging_bytes;
      options.key = key_arg.xts(first_unit);
      options.dictionary = dictionary;
      return bdev_decompress_marked_sync(dst.get(), dst_offset, len, granule,
                                         words, options, source, &unpacked,
                                         error);
    });
    return unpacked;
  }, py::arg("dst"), py::arg("bitmap"), py::arg("granule"), py::arg("sizes"),
     py::arg("data"), py::arg("dst_offset") = 0, py::arg("length") = py::none(),
     py::arg("staging_bytes") = 0, py::arg("dictionary") = false,
     py::arg("key") = py::none(), py::arg("first_unit") = 0,
     "Decode the pieces of bdev_compress_marked into the granules marked in "
     "`bitmap`; every piece is validated on the host first. Returns the "
     "number written. `dictionary`: the pieces are HSLZD1 and the "
     "dictionary of a granule is what `dst` holds there before the call. "
     "With `key`, `data` is the keyed stream of bdev_compress_marked; HBM "
     "bdevs decrypt it on the GPU (k_xts_var) and validate while decoding");

  m.def("xts_marked_probe", [](BdevPtr bdev, py::bytes bitmap,
                               uint32_t granule, py::bytes key, bool unpack,
                               uint64_t staging_bytes) {
    const std::string raw = bitmap;
    const uint64_t len =
        marked_range("xts_marked_probe", *bdev, 0, std::nullopt, granule, raw);
    const std::vector<uint64_t> words = bitmap_words(raw);
    const KeyArg key_arg(key);
    uint64_t moved = 0;
    double seconds = 0;
    delta_call("xts_marked_probe", [&](std::string* error) {
      *error = "bad key, granule or range, or the call failed";
      const auto t0 = std::chrono::steady_clock::now();
      const int status =
          unpack ? bdev_xts_unpack_marked_sync(
                       bdev.get(), 0, len, granule, words, key_arg.xts(0),
                       staging_bytes,
                       [](uint8_t*, uint64_t, uint64_t) { return 0; }, &moved)
                 : bdev_xts_pack_marked_sync(
                       bdev.get(), 0, len, granule, words, key_arg.xts(0),
                       staging_bytes,
                       [](const uint8_t*, uint64_t, uint64_t) { return 0; },
                       &moved);
      seconds = std::chrono::duration<double>(
                    std::chrono::steady_clock::now() - t0).count();
      return status;
    });
    py::dict d;
    d["seconds"] = seconds;
    d["granules"] = moved;
    return d;
  }, py::arg("bdev"), py::arg("bitmap"), py::arg("granule"), py::arg("key"),
     py::arg("unpack") = false, py::arg("staging_bytes") = 0,
     "Measurement aid (tools/crypt_bench.py): bdev_xts_pack_marked with a "
     "discarding sink, or with unpack bdev_xts_unpack_marked with a source "
     "that leaves the staging buffer as it is (the volume is overwritten)");

  m.def("bdev_import_delta", [](BdevPtr dst, const std::string& path,
                                bool dry_run, std::optional<py::bytes> key) {
    DeltaInfo info;
    const KeyArg key_arg(key);
    delta_call("bdev_import_delta", [&](std::string* error) {
      return bdev_import_delta(dst.get(), path, dry_run, &info, error,
                               key_arg.ptr());
    });
    return delta_info_to_dict(info);
  }, py::arg("dst"), py::arg("path"), py::arg("dry_run") = false,
     py::arg("key") = py::none(),
     "Apply a hipstore delta file to dst; dry_run checks everything and "
     "writes nothing. A version-3 file needs its key (dry_run works "
     "without one)");

  m.def("delta_file_info", [](const std::string& path) {
    DeltaInfo info;
    delta_call("delta_file_info", [&](std::string* error) {
      return delta_file_info(path, &info, error);
    });
    return delta_info_to_dict(info);
  }, py::arg("path"), "Header fields of a delta file, after its structural checks");

  m.def("fingerprint_bytes", [](py::bytes data, uint32_t granule,
                                uint32_t algorithm,
                                std::optional<py::bytes> key) {
    const std::string raw = data;
    const KeyArg key_arg(key);
    const FingerprintKind kind = fingerprint_kind(algorithm, key_arg);
    if (!fingerprint_kind_ok(kind)) {
      throw std::invalid_argument(
          "fingerprint_bytes: algorithm 1 or 2 without a key, or 3 with a key "
          "of 32 bytes");
    }
    if (granule == 0 || granule % 16 != 0 || raw.size() % granule != 0) {
      throw std::invalid_argument(
          "fingerprint_bytes: granule must be a non-zero multiple of 16 that "
          "divides the data length");
    }
    const uint64_t n = raw.size() / granule;
    std::string out(n * kFingerprintBytes, '\0');
    {
      py::gil_scoped_release release;
      fingerprint_granules(raw.data(), n, granule, kind,
                           reinterpret_cast<uint8_t*>(&out[0]));
    }
    return py::bytes(out);
  }, py::arg("data"), py::arg("granule"), py::arg("algorithm") = 1,
     py::arg("key") = py::none(),
     "Granule fingerprints (16 bytes each) of a bytes object, on the host: "
     "algorithm 1 = HSFP1, 2 = HSFP2 (BLAKE2s), 3 = HSFP2 keyed (32 bytes)");

  m.def("bdev_fingerprint", [](BdevPtr bdev, uint32_t granule, uint64_t offset,
                               uint64_t length, uint64_t staging_bytes,
                               bool keep, uint32_t algorithm,
                               std::optional<py::bytes> key) {
    const KeyArg key_arg(key);
    const FingerprintKind kind = fingerprint_kind(algorithm, key_arg);
    if (length == 0 && granule != 0 && offset <= bdev->size_bytes()) {
      length = (bdev->size_bytes() - offset) / granule * granule;
    }
    std::string out;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_fingerprint_sync(
          bdev.get(), offset, length, granule, staging_bytes,
          [&out, keep](const uint8_t* fps, uint64_t, uint64_t count) {
            if (keep) {
              out.append(reinterpret_cast<const char*>(fps),
                         count * kFingerprintBytes);
            }
            return 0;
          },
          nullptr, kind);
    }
    if (status != kIoOk) {
      throw std::runtime_error("bdev_fingerprint failed: status " +
                               std::to_string(status));
    }
    return py::bytes(out);
  }, py::arg("bdev"), py::arg("granule"), py::arg("offset") = 0,
     py::arg("length") = 0, py::arg("staging_bytes") = 0,
     py::arg("keep") = true, py::arg("algorithm") = 1,
     py::arg("key") = py::none(),
     "Granule fingerprints (16 bytes each) of a bdev range (on-GPU for HBM "
     "bdevs). length=0: to the end of the device in whole granules. "
     "algorithm and key as fingerprint_bytes. "
     "keep=False discards them and returns b'' (tools/fingerprint_bench.py: "
     "the pass without the host copy)");

  m.def("bdev_fingerprint_file", [](BdevPtr bdev, const std::string& path,
                                    std::optional<uint32_t> granule,
                                    bool overwrite,
                                    std::optional<std::string> map_algorithm,
                                    std::optional<py::bytes> map_key) {
    FingerprintMapInfo info;
    const KeyArg key_arg(map_key);
    const MapKind kind = map_kind(map_algorithm, key_arg);
    delta_call("bdev_fingerprint_file", [&](std::string* error) {
      return bdev_fingerprint_file(bdev.get(), path, granule.value_or(0),
                                   overwrite, &info, error, kind);
    });
    return map_info_to_dict(info);
  }, py::arg("bdev"), py::arg("path"), py::arg("granule") = py::none(),
     py::arg("overwrite") = false, py::arg("map_algorithm") = py::none(),
     py::arg("map_key") = py::none(),
     "Write the fingerprint map of a whole bdev to a file (map_algorithm "
     "\"blake2s\": an HSFP2 map, keyed with map_key)");

  m.def("fingerprint_map_info", [](const std::string& path) {
    FingerprintMapInfo info;
    delta_call("fingerprint_map_info", [&](std::string* error) {
      return fingerprint_map_info(path, &info, error);
    });
    return map_info_to_dict(info);
  }, py::arg("path"),
     "Header fields of a fingerprint map, after every check of the file");

  m.def("bdev_verify_fingerprints", [](BdevPtr bdev, const std::string& path,
                                       uint32_t max_report,
                                       std::optional<std::string> map_algorithm,
                                       std::optional<py::bytes> map_key) {
    FingerprintVerify r;
    const KeyArg key_arg(map_key);
    const MapKind kind = map_kind(map_algorithm, key_arg);
    delta_call("bdev_verify_fingerprints", [&](std::string* error) {
      return bdev_verify_fingerprints(bdev.get(), path, max_report, &r, error,
                                      kind);
    });
    py::dict d;
    d["granule"] = r.granule;
    d["granules"] = r.granules;
    d["mismatched"] = r.mismatched;
    d["first_mismatches"] = r.first_mismatches;
    return d;
  }, py::arg("bdev"), py::arg("path"), py::arg("max_report") = 16,
     py::arg("map_algorithm") = py::none(), py::arg("map_key") = py::none(),
     "Recompute a bdev's fingerprints over a map's range and compare; a "
     "keyed map needs its map_key");

  m.def("replica_scrub", [](BdevPtr bdev, bool repair, uint32_t granule,
                            uint32_t max_report) {
    ScrubResult r;
    {
      py::gil_scoped_release release;
      r = replicated_scrub(bdev.get(), repair, granule, max_report);
    }
    if (r.status != kIoOk) {
      throw std::runtime_error("replica_scrub failed: status " +
                               std::to_string(r.status));
    }
    py::list replicas;
    for (const ScrubReplica& rep : r.replicas) {
      py::dict d;
      d["child"] = rep.child;
      d["granules"] = rep.granules;
      d["mismatched"] = rep.mismatched;
      d["repaired"] = rep.repaired;
      d["first_mismatches"] = rep.first_mismatches;
      replicas.append(d);
    }
    py::dict out;
    out["granule"] = r.granule;
    out["replicas"] = replicas;
    return out;
  }, py::arg("bdev"), py::arg("repair") = false, py::arg("granule") = 0,
     py::arg("max_report") = 16,
     "Compare every replica of a replicated bdev with child 0; with "
     "repair, overwrite mismatching granules from it (refused while the "
     "bdev is claimed)");

  m.def("parity_encode", [](std::vector<BdevPtr> data, BdevPtr p, BdevPtr q,
                            std::vector<uint64_t> data_offsets,
                            uint64_t p_offset, uint64_t q_offset,
                            uint64_t length) {
    const ParityArgs a = parity_args(data, p, q, data_offsets, p_offset,
                                     q_offset, length, 0);
    ParityReport report;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_parity_encode_sync(a.data, a.p, a.q, a.length, &report);
    }
    parity_raise("parity_encode", status, report);
    py::dict d;
    d["length"] = a.length;
    d["on_gpu"] = report.on_gpu;
    return d;
  }, py::arg("data"), py::arg("p") = py::none(), py::arg("q") = py::none(),
     py::arg("data_offsets") = std::vector<uint64_t>{},
     py::arg("p_offset") = 0, py::arg("q_offset") = 0, py::arg("length") = 0,
     "Write P (XOR) and / or Q (Reed-Solomon over GF(2^8)) parity of up to "
     "32 data bdevs (on-GPU for HBM sets). length=0: the whole of the "
     "shortest member");

  m.def("parity_check", [](std::vector<BdevPtr> data, BdevPtr p, BdevPtr q,
                           uint32_t granule, uint32_t max_report,
                           std::vector<uint64_t> data_offsets,
                           uint64_t p_offset, uint64_t q_offset,
                           uint64_t length) {
    if (granule == 0 && !data.empty() && data[0]) {
      granule = static_cast<uint32_t>(data[0]->block_size());
    }
    const ParityArgs a = parity_args(data, p, q, data_offsets, p_offset,
                                     q_offset, length, granule);
    ParityReport report;
    ParityCheck check;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_parity_check_sync(a.data, a.p, a.q, a.length, granule,
                                      max_report, &check, &report);
    }
    parity_raise("parity_check", status, report);
    py::dict d;
    d["granule"] = granule;
    d["on_gpu"] = report.on_gpu;
    d["p"] = parity_stats_dict(check.p, check.p_bitmap);
    d["q"] = parity_stats_dict(check.q, check.q_bitmap);
    return d;
  }, py::arg("data"), py::arg("p") = py::none(), py::arg("q") = py::none(),
     py::arg("granule") = 0, py::arg("max_report") = 16,
     py::arg("data_offsets") = std::vector<uint64_t>{},
     py::arg("p_offset") = 0, py::arg("q_offset") = 0, py::arg("length") = 0,
     "Recompute P / Q of the data bdevs and compare with the stored parity, "
     "granule by granule; \"p\" and \"q\" are shaped like bdev_diff results");

  m.def("parity_rebuild", [](std::vector<BdevPtr> data, py::list lost,
                             BdevPtr p, BdevPtr q,
                             std::vector<uint64_t> data_offsets,
                             uint64_t p_offset, uint64_t q_offset,
                             uint64_t length) {
    std::vector<int> lost_ids;
    for (py::handle item : lost) {
      if (py::isinstance<py::str>(item)) {
        const std::string name = item.cast<std::string>();
        if (name != "p" && name != "q") {
          throw std::invalid_argument("parity_rebuild: lost entries are data "
                                      "indices, \"p\" or \"q\"");
        }
        lost_ids.push_back(name == "p" ? kParityLostP : kParityLostQ);
      } else {
        const int64_t index = item.cast<int64_t>();
        // Anything that is no index stays invalid for the core to name.
        lost_ids.push_back(index < 0 || index > INT32_MAX
                               ? INT32_MAX
                               : static_cast<int>(index));
      }
    }
    const ParityArgs a = parity_args(data, p, q, data_offsets, p_offset,
                                     q_offset, length, 0);
    ParityReport report;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_parity_rebuild_sync(a.data, a.p, a.q, a.length, lost_ids,
                                        &report);
    }
    parity_raise("parity_rebuild", status, report);
    py::dict d;
    d["length"] = a.length;
    d["on_gpu"] = report.on_gpu;
    return d;
  }, py::arg("data"), py::arg("lost"), py::arg("p") = py::none(),
     py::arg("q") = py::none(),
     py::arg("data_offsets") = std::vector<uint64_t>{},
     py::arg("p_offset") = 0, py::arg("q_offset") = 0, py::arg("length") = 0,
     "Rewrite the one or two members named by `lost` (data indices, \"p\", "
     "\"q\") from the others; the bdevs in those slots are the targets");

  m.def("parity_update", [](std::vector<BdevPtr> data, BdevPtr p, BdevPtr q,
                            std::vector<BdevPtr> bases,
                            std::vector<uint64_t> data_offsets,
                            std::vector<uint64_t> base_offsets,
                            uint64_t p_offset, uint64_t q_offset,
                            uint64_t length, uint32_t granule,
                            uint32_t max_report, bool refresh) {
    if (!base_offsets.empty() && base_offsets.size() != bases.size()) {
      throw std::invalid_argument("parity_update: one offset per base slot");
    }
    std::vector<ParityMember> base_members;
    for (size_t i = 0; i < bases.size(); ++i) {
      base_members.push_back(
          {bases[i].get(),
           bases[i] && !base_offsets.empty() ? base_offsets[i] : 0});
    }
    if (granule == 0 && !data.empty() && data[0]) {
      granule = static_cast<uint32_t>(data[0]->block_size());
    }
    ParityArgs a = parity_args(data, p, q, data_offsets, p_offset, q_offset,
                               length, granule);
    if (length == 0) {  // the bases bound the default extent too
      std::vector<ParityMember> bound = a.data;
      bound.insert(bound.end(), base_members.begin(), base_members.end());
      a.length = parity_common_length(bound, a.p, a.q, granule);
    }
    ParityReport report;
    DiffStats changed;
    std::vector<uint64_t> words;
    int status;
    {
      py::gil_scoped_release release;
      status = bdev_parity_update_sync(a.data, a.p, a.q, base_members,
                                       a.length, granule, max_report, refresh,
                                       &changed, &words, &report);
    }
    parity_raise("parity_update", status, report);
    py::dict d;
    d["length"] = a.length;
    d["on_gpu"] = report.on_gpu;
    d["granule"] = granule;
    d["changed"] = parity_stats_dict(changed, words);
    return d;
  }, py::arg("data"), py::arg("p") = py::none(), py::arg("q") = py::none(),
     py::arg("bases") = std::vector<BdevPtr>{},
     py::arg("data_offsets") = std::vector<uint64_t>{},
     py::arg("base_offsets") = std::vector<uint64_t>{},
     py::arg("p_offset") = 0, py::arg("q_offset") = 0, py::arg("length") = 0,
     py::arg("granule") = 0, py::arg("max_report") = 16,
     py::arg("refresh") = false,
     "Bring stored P / Q up to date from the tracked data bdevs and the "
     "clones of their earlier state in `bases` (None = untracked, not "
     "read); \"changed\" is shaped like a bdev_diff result. refresh=True "
     "also stores the changed bytes into the bases");

  m.def("persistent_probe", &persistent_probe, py::arg("device") = 0,
        py::arg("flags") = 1,
        py::call_guard<py::gil_scoped_release>());
  m.def("persistent_kernel_probe", &persistent_kernel_probe,
        py::arg("device") = 0, py::arg("variant") = 0,
        py::call_guard<py::gil_scoped_release>());

  m.def("persistent_stats", [] {
    py::dict d;
    d["launches"] = hipstore::persistent_stat(0);
    d["relaunches"] = hipstore::persistent_stat(1);
    d["stall_queries"] = hipstore::persistent_stat(2);
    return d;
  });

  m.def("crc32c_combine", &crc32c_combine, py::arg("crc1"), py::arg("crc2"),
        py::arg("len2"));

  m.def("crc32c_table", [](py::buffer data, uint32_t init) {
    py::buffer_info info = data.request();
    return crc32c_table(init, info.ptr,
                        static_cast<size_t>(info.size) * info.itemsize);
  }, py::arg("data"), py::arg("init") = 0);
  m.def("crc32c", [](py::buffer data, uint32_t init) {
    py::buffer_info info = data.request();
    return crc32c_sw(init, info.ptr, static_cast<size_t>(info.size) * info.itemsize);
  }, py::arg("data"), py::arg("init") = 0);

  m.def("crc32c_gpu_blocks", [](BdevPtr bdev, uint64_t offset, uint32_t block,
                                uint32_t count) {
    std::vector<uint32_t> out(count);
    {
      py::gil_scoped_release release;
      crc32c_hbm_blocks(bdev.get(), offset, block, count, out.data());
    }
    return out;
  }, py::arg("bdev"), py::arg("offset"), py::arg("block"), py::arg("count"),
     "CRC32C of `count` consecutive `block`-byte blocks of an HBM bdev, "
     "computed on-GPU");

  m.def("crc32c_gpu_range", [](BdevPtr bdev, uint64_t offset,
                               uint64_t length) {
    py::gil_scoped_release release;
    return crc32c_hbm_range(bdev.get(), offset, length);
  }, py::arg("bdev"), py::arg("offset"), py::arg("length"),
     "CRC32C of one range: per-4 KiB block CRCs folded with "
     "crc32c_combine (the digest ladder of the NVMe-oF and rados paths)");
}
