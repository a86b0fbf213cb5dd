// NVMe-oF/TCP target: exports hipstored bdevs as namespaces.
//
// Counterpart of the SPDK nvmf target the reference's initiator would
// talk to (reference lib/nvme/nvme_tcp.c peer); one thread per
// connection (the control plane's scale; the polled initiator is the
// measured data path). HBM-namespace C2HData digests come from the GPU
// CRC32C kernel + host combine.

#include <arpa/inet.h>
#include <fcntl.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <pthread.h>
#include <sched.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "hipstore/engine.h"
#include "hipstore/nvmf.h"
#include "nvmf_common.h"

namespace hipstore {

namespace {

using namespace nvmf;

// CRC32C of a range the target is about to transmit. The host copy
// always exists here (TCP needs host bytes), and SSE4.2 runs at
// ~15 GB/s, so the GPU per-4KiB kernel only wins once the extent is
// large enough to amortize a launch+sync round trip (~100 us when
// resident service kernels hold the HW queues) against re-touching
// the bytes: measured crossover is around 1 MiB. Below that the
// hardware-CRC host path is strictly faster (128 KiB digest path:
// 0.57 -> ~5 GB/s).
// Consequence: the read path only digests PDUs of at most
// kMaxDataPerPdu (128 KiB) and always has a host copy, so the GPU
// branch below is currently unreachable from NVMe-oF; every C2HData
// digest comes from the host CRC. The shared ladder it would use is
// crc32c_hbm_range, which has its own tests.
uint32_t range_crc32c(Bdev* bdev, uint64_t offset, const void* host_copy,
                      uint32_t len) {
  if (bdev->device_base() != nullptr &&
      (host_copy == nullptr || len >= (1u << 20)) && len % 4096 == 0 &&
      len != 0 && offset % 4096 == 0) {
    return crc32c_hbm_range(bdev, offset, len);
  }
  return crc32c_sw(0, host_copy, len);
}

class TargetImpl : public NvmfTcpTarget,
                   public std::enable_shared_from_this<TargetImpl> {
 public:
  TargetImpl(const std::string& addr, uint16_t port, std::string subnqn,
             bool digests)
      : subnqn_(std::move(subnqn)), digests_(digests) {
    listen_fd_ = socket(AF_INET, SOCK_STREAM | SOCK_CLOEXEC, 0);
    if (listen_fd_ < 0) throw std::runtime_error("nvmf target: socket failed");
    int one = 1;
    setsockopt(listen_fd_, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in sa{};
    sa.sin_family = AF_INET;
    sa.sin_port = htons(port);
    sa.sin_addr.s_addr =
        addr.empty() ? htonl(INADDR_LOOPBACK) : inet_addr(addr.c_str());
    if (bind(listen_fd_, reinterpret_cast<sockaddr*>(&sa), sizeof(sa)) < 0 ||
        listen(listen_fd_, 16) < 0) {
      close(listen_fd_);
      throw std::runtime_error("nvmf target: bind/listen failed");
    }
    socklen_t slen = sizeof(sa);
    getsockname(listen_fd_, reinterpret_cast<sockaddr*>(&sa), &slen);
    port_ = ntohs(sa.sin_port);
  }

  ~TargetImpl() override { stop(); }

  void start() {
    running_.store(true);
    accept_thread_ = std::thread([this] { accept_loop(); });
  }

  uint16_t port() const override { return port_; }

  void add_namespace(BdevPtr bdev) override {
    std::lock_guard<std::mutex> lock(mutex_);
    namespaces_.push_back(std::move(bdev));
  }

  void stop() override {
    if (!running_.exchange(false)) return;
    shutdown(listen_fd_, SHUT_RDWR);
    close(listen_fd_);
    if (accept_thread_.joinable()) accept_thread_.join();
    decltype(connections_) conns;
    {
      std::lock_guard<std::mutex> lock(mutex_);
      conns.swap(connections_);
    }
    for (auto& [t, done] : conns) {
      if (t.joinable()) t.join();
    }
  }

 private:
  BdevPtr ns(uint32_t nsid) {
    std::lock_guard<std::mutex> lock(mutex_);
    if (nsid == 0 || nsid > namespaces_.size()) return nullptr;
    return namespaces_[nsid - 1];
  }

  void accept_loop() {
    while (running_.load()) {
      int fd = accept(listen_fd_, nullptr, nullptr);
      if (fd < 0) {
        if (!running_.load()) break;
        continue;
      }
      int one = 1;
      setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof(one));
      std::lock_guard<std::mutex> lock(mutex_);
      for (auto it = connections_.begin(); it != connections_.end();) {
        if (it->second->load()) {
          it->first.join();
          it = connections_.erase(it);
        } else {
          ++it;
        }
      }
      auto done = std::make_shared<std::atomic<bool>>(false);
      connections_.emplace_back(
          std::thread([this, fd, done] {
            // Optional pinning for this hot-polling connection thread
            // (HIPSTORE_NVMF_AFFINITY_BASE=<core>): unpinned spinners
            // migrate under CFS and crowd each other — the same
            // plateau measured and fixed on the vhost ring workers.
            if (const char* env = getenv("HIPSTORE_NVMF_AFFINITY_BASE")) {
              static std::atomic<int> next_slot{0};
              const long ncpu = sysconf(_SC_NPROCESSORS_ONLN);
              if (ncpu > 0) {
                cpu_set_t set;
                CPU_ZERO(&set);
                CPU_SET((atoi(env) + next_slot.fetch_add(1)) %
                            static_cast<int>(ncpu),
                        &set);
                (void)pthread_setaffinity_np(pthread_self(), sizeof(set),
                                             &set);
              }
            }
            serve(fd);
            close(fd);
            done->store(true);
          }),
          done);
    }
  }

  struct PendingWrite {
    Sqe sqe;
    std::vector<uint8_t> data;
    uint32_t received = 0;
  };

  void serve(int fd) {
    // --- ICReq / ICResp handshake ---------------------------------------
    IcReq icreq{};
    if (!read_exact(fd, &icreq, sizeof(icreq)) || icreq.ch.type != kIcReq) {
      return;
    }
    const bool hdgst = digests_ && (icreq.dgst & 0x1);
    const bool ddgst = digests_ && (icreq.dgst & 0x2);
    IcResp icresp{};
    icresp.ch = {kIcResp, 0, sizeof(IcResp), 0, sizeof(IcResp)};
    icresp.pfv = 0;
    icresp.cpda = 0;
    icresp.dgst = (hdgst ? 0x1 : 0) | (ddgst ? 0x2 : 0);
    icresp.maxh2cdata = kMaxDataPerPdu;
    if (!write_exact(fd, &icresp, sizeof(icresp))) return;

    // The connection is served as a polled pipeline: the socket goes
    // non-blocking, commands submit ASYNCHRONOUSLY to the bdev channel
    // and completions (fired from poll on this thread) send the
    // C2HData/CQE — so a connection sustains its full queue depth
    // instead of one command at a time. Outbound sends stay blocking
    // (write_exact spins on EAGAIN).
    uint32_t cc = 0;
    uint16_t next_ttag = 1;
    std::map<uint16_t, PendingWrite> pending_writes;  // by ttag
    bool dead = false;
    int inflight = 0;

    // Reusable pinned buffers: hipHostMalloc costs ~1 ms, so per-I/O
    // allocation is off the table; concurrent in-flight commands each
    // borrow from this pool.
    struct PoolBuf {
      uint8_t* ptr;
      size_t cap;
    };
    std::vector<PoolBuf> pool;
    auto pool_get = [&](size_t len) -> PoolBuf {
      for (auto it = pool.begin(); it != pool.end(); ++it) {
        if (it->cap >= len) {
          PoolBuf b = *it;
          pool.erase(it);
          return b;
        }
      }
      size_t cap = std::max<size_t>(len, 128 * 1024);
      return PoolBuf{static_cast<uint8_t*>(alloc_pinned(cap)), cap};
    };
    auto pool_put = [&](PoolBuf b) { pool.push_back(b); };

    std::map<Bdev*, std::shared_ptr<IoChannel>> channels;
    auto channel_of = [&](Bdev* bdev) -> IoChannel* {
      auto it = channels.find(bdev);
      if (it == channels.end()) {
        it = channels.emplace(bdev, bdev->get_channel()).first;
      }
      return it->second.get();
    };

    auto send_cqe = [&](uint16_t cid, uint16_t sc, uint64_t result = 0) {
      struct {
        CommonHeader ch;
        Cqe cqe;
      } __attribute__((packed)) resp{};
      resp.ch = {kCapsuleResp, static_cast<uint8_t>(hdgst ? kFlagHdgst : 0),
                 24, 0, static_cast<uint32_t>(24 + (hdgst ? 4 : 0))};
      resp.cqe.set_result64(result);
      resp.cqe.set_cid(cid);
      resp.cqe.set_status(sc);
      if (!send_pdu(fd, &resp, 24, hdgst, nullptr, 0, 0, false)) dead = true;
      return !dead;
    };

    auto send_c2h_data = [&](uint16_t cid, const uint8_t* data, uint32_t len,
                             uint32_t digest_all) {
      uint32_t offset = 0;
      while (offset < len) {
        const uint32_t chunk = std::min(len - offset, kMaxDataPerPdu);
        DataHeader dh{};
        const uint8_t pdo = 24 + (hdgst ? 4 : 0);
        const bool last = offset + chunk >= len;
        dh.ch = {kC2HData,
                 static_cast<uint8_t>((hdgst ? kFlagHdgst : 0) |
                                      (ddgst ? kFlagDdgst : 0) |
                                      (last ? kFlagLast : 0)),
                 24, pdo,
                 static_cast<uint32_t>(pdo + chunk + (ddgst ? 4 : 0))};
        dh.cccid = cid;
        dh.datao = offset;
        dh.datal = chunk;
        uint32_t dd = 0;
        if (ddgst) {
          dd = (chunk == len && digest_all != 0)
                   ? digest_all  // whole-range digest already on hand
                   : crc32c_sw(0, data + offset, chunk);
        }
        if (!send_pdu(fd, &dh, 24, hdgst, data + offset, chunk, dd, ddgst)) {
          dead = true;
          return false;
        }
        offset += chunk;
      }
      return true;
    };

    // Async bdev ops; `done` runs inline from the poll loop below.
    auto submit_io = [&](BdevPtr bdev, IoOp op, uint64_t off, void* buf,
                         uint64_t len, std::function<void(int)> done) {
      IoRequest req;
      req.op = op;
      req.offset = off;
      req.length = len;
      req.buffer = buf;
      req.fill = 0;
      ++inflight;
      req.on_complete = [&inflight, done = std::move(done)](int status) {
        --inflight;
        done(status);
      };
      bdev->submit(channel_of(bdev.get()), std::move(req));
    };

    auto handle_command = [&](const Sqe& sqe, std::vector<uint8_t>& capsule_data) {
      if (sqe.opc() == kOpcFabrics) {
        switch (sqe.fctype()) {
          case kFctypeConnect:
            return send_cqe(sqe.cid(), kScSuccess, 1);  // cntlid in dw0
          case kFctypePropertySet: {
            if (sqe.cdw(11) == kPropCc) cc = sqe.cdw(12);
            return send_cqe(sqe.cid(), kScSuccess);
          }
          case kFctypePropertyGet: {
            uint32_t ofst = sqe.cdw(11);
            uint64_t value = 0;
            if (ofst == kPropCap) {
              value = 0x3FFull | (1ull << 37);  // MQES=1023, NVM cmd set
            } else if (ofst == kPropCsts) {
              value = (cc & 1) ? 1 : 0;  // RDY follows CC.EN
            } else if (ofst == kPropCc) {
              value = cc;
            }
            return send_cqe(sqe.cid(), kScSuccess, value);
          }
          default:
            return send_cqe(sqe.cid(), kScInvalidField);
        }
      }
      switch (sqe.opc()) {
        case kOpcIdentify: {
          const uint8_t cns = sqe.cdw(10) & 0xFF;
          std::vector<uint8_t> data(4096, 0);
          if (cns == 0x00) {  // namespace
            BdevPtr bdev = ns(sqe.nsid());
            if (!bdev) return send_cqe(sqe.cid(), kScInvalidField);
            uint64_t nsze = bdev->num_blocks();
            memcpy(data.data() + 0, &nsze, 8);
            memcpy(data.data() + 8, &nsze, 8);
            memcpy(data.data() + 16, &nsze, 8);
            uint8_t lbads = 0;
            for (uint64_t bs = bdev->block_size(); bs > 1; bs >>= 1) ++lbads;
            data[128 + 2] = lbads;  // LBAF0.LBADS
          } else if (cns == 0x01) {  // controller: zeros suffice
          } else {
            return send_cqe(sqe.cid(), kScInvalidField);
          }
          if (!send_c2h_data(sqe.cid(), data.data(), data.size(), 0)) {
            return false;
          }
          return send_cqe(sqe.cid(), kScSuccess);
        }
        case kOpcKeepAlive:
          return send_cqe(sqe.cid(), kScSuccess);
        case kOpcRead: {
          BdevPtr bdev = ns(sqe.nsid());
          if (!bdev) return send_cqe(sqe.cid(), kScInvalidField);
          const uint64_t slba =
              sqe.cdw(10) | (static_cast<uint64_t>(sqe.cdw(11)) << 32);
          const uint32_t nlb = (sqe.cdw(12) & 0xFFFF) + 1;
          const uint64_t off = slba * bdev->block_size();
          const uint64_t len = static_cast<uint64_t>(nlb) * bdev->block_size();
          if (off + len > bdev->size_bytes()) {
            return send_cqe(sqe.cid(), kScLbaOutOfRange);
          }
          PoolBuf pb = pool_get(len);
          const uint16_t cid = sqe.cid();
          submit_io(bdev, IoOp::kRead, off, pb.ptr, len,
                    [&, bdev, pb, off, len, cid](int status) {
                      if (status != kIoOk) {
                        send_cqe(cid, kScInternalError);
                      } else {
                        // GPU digest for HBM namespaces (per-4KiB
                        // kernel + host combine).
                        uint32_t digest = 0;
                        if (ddgst && len <= kMaxDataPerPdu) {
                          digest = range_crc32c(bdev.get(), off, pb.ptr, len);
                        }
                        if (send_c2h_data(cid, pb.ptr, len, digest)) {
                          send_cqe(cid, kScSuccess);
                        }
                      }
                      pool_put(pb);
                    });
          return true;
        }
        case kOpcWrite: {
          BdevPtr bdev = ns(sqe.nsid());
          if (!bdev) return send_cqe(sqe.cid(), kScInvalidField);
          const uint64_t slba =
              sqe.cdw(10) | (static_cast<uint64_t>(sqe.cdw(11)) << 32);
          const uint32_t nlb = (sqe.cdw(12) & 0xFFFF) + 1;
          const uint64_t off = slba * bdev->block_size();
          const uint64_t len = static_cast<uint64_t>(nlb) * bdev->block_size();
          if (off + len > bdev->size_bytes()) {
            return send_cqe(sqe.cid(), kScLbaOutOfRange);
          }
          if (!capsule_data.empty()) {
            // In-capsule data (small writes).
            if (capsule_data.size() != len) {
              return send_cqe(sqe.cid(), kScInvalidField);
            }
            PoolBuf pb = pool_get(len);
            memcpy(pb.ptr, capsule_data.data(), len);
            const uint16_t cid = sqe.cid();
            submit_io(bdev, IoOp::kWrite, off, pb.ptr, len,
                      [&, pb, cid](int status) {
                        send_cqe(cid, status == kIoOk ? kScSuccess
                                                      : kScInternalError);
                        pool_put(pb);
                      });
            return true;
          }
          // Solicit the data with one R2T covering the whole transfer.
          PendingWrite pw;
          pw.sqe = sqe;
          pw.data.resize(len);
          uint16_t ttag = next_ttag++;
          pending_writes[ttag] = std::move(pw);
          DataHeader r2t{};
          r2t.ch = {kR2T, static_cast<uint8_t>(hdgst ? kFlagHdgst : 0), 24, 0,
                    static_cast<uint32_t>(24 + (hdgst ? 4 : 0))};
          r2t.cccid = sqe.cid();
          r2t.ttag = ttag;
          r2t.datao = 0;
          r2t.datal = len;
          if (!send_pdu(fd, &r2t, 24, hdgst, nullptr, 0, 0, false)) {
            dead = true;
            return false;
          }
          return true;
        }
        case kOpcFlush: {
          BdevPtr bdev = ns(sqe.nsid());
          if (!bdev) return send_cqe(sqe.cid(), kScSuccess);
          const uint16_t cid = sqe.cid();
          submit_io(bdev, IoOp::kFlush, 0, nullptr, 0, [&, cid](int status) {
            send_cqe(cid, status == kIoOk ? kScSuccess : kScInternalError);
          });
          return true;
        }
        case kOpcWriteZeroes: {
          BdevPtr bdev = ns(sqe.nsid());
          if (!bdev) return send_cqe(sqe.cid(), kScInvalidField);
          const uint64_t slba =
              sqe.cdw(10) | (static_cast<uint64_t>(sqe.cdw(11)) << 32);
          const uint32_t nlb = (sqe.cdw(12) & 0xFFFF) + 1;
          const uint16_t cid = sqe.cid();
          submit_io(bdev, IoOp::kFill, slba * bdev->block_size(), nullptr,
                    static_cast<uint64_t>(nlb) * bdev->block_size(),
                    [&, cid](int status) {
                      send_cqe(cid,
                               status == kIoOk ? kScSuccess : kScInternalError);
                    });
          return true;
        }
        default:
          return send_cqe(sqe.cid(), kScInvalidOpcode);
      }
    };

    auto handle_pdu = [&](const uint8_t* pdu, const CommonHeader& chh) {
      if (hdgst) {
        uint32_t hd;
        memcpy(&hd, pdu + chh.hlen, 4);
        if (hd != crc32c_sw(0, pdu, chh.hlen)) {
          dead = true;
          return;
        }
      }
      const uint32_t pdo = chh.pdo ? chh.pdo : chh.hlen + (hdgst ? 4 : 0);
      uint32_t data_len = 0;
      if (chh.plen > pdo) data_len = chh.plen - pdo - (ddgst ? 4 : 0);
      if (ddgst && data_len > 0) {
        uint32_t dd;
        memcpy(&dd, pdu + pdo + data_len, 4);
        if (dd != crc32c_sw(0, pdu + pdo, data_len)) {
          dead = true;  // a real target sends C2HTermReq
          return;
        }
      }
      if (chh.type == kCapsuleCmd) {
        Sqe sqe;
        memcpy(sqe.bytes, pdu + 8, 64);
        std::vector<uint8_t> capsule_data(pdu + pdo, pdu + pdo + data_len);
        handle_command(sqe, capsule_data);
      } else if (chh.type == kH2CData) {
        DataHeader dh;
        memcpy(&dh, pdu, sizeof(dh));
        auto it = pending_writes.find(dh.ttag);
        if (it == pending_writes.end()) {
          dead = true;
          return;
        }
        PendingWrite& pw = it->second;
        if (dh.datao + data_len > pw.data.size()) {
          dead = true;
          return;
        }
        memcpy(pw.data.data() + dh.datao, pdu + pdo, data_len);
        pw.received += data_len;
        if (pw.received >= pw.data.size()) {
          BdevPtr bdev = ns(pw.sqe.nsid());
          const uint64_t slba = pw.sqe.cdw(10) |
                                (static_cast<uint64_t>(pw.sqe.cdw(11)) << 32);
          PoolBuf pb = pool_get(pw.data.size());
          memcpy(pb.ptr, pw.data.data(), pw.data.size());
          const uint16_t cid = pw.sqe.cid();
          const uint64_t len = pw.data.size();
          pending_writes.erase(it);
          submit_io(bdev, IoOp::kWrite, slba * bdev->block_size(), pb.ptr,
                    len, [&, pb, cid](int status) {
                      send_cqe(cid, status == kIoOk ? kScSuccess
                                                    : kScInternalError);
                      pool_put(pb);
                    });
        }
      } else {
        dead = true;  // unexpected PDU
      }
    };

    // --- polled PDU/completion loop --------------------------------------
    {
      int flags = fcntl(fd, F_GETFL, 0);
      fcntl(fd, F_SETFL, flags | O_NONBLOCK);
    }
    std::string rx;
    uint32_t idle_spins = 0;
    while (running_.load() && !dead) {
      char tmp[65536];
      while (true) {
        ssize_t n = recv(fd, tmp, sizeof(tmp), 0);
        if (n > 0) {
          rx.append(tmp, n);
          if (rx.size() > (64u << 20)) dead = true;
          continue;
        }
        if (n < 0 && (errno == EAGAIN || errno == EWOULDBLOCK)) break;
        if (n < 0 && errno == EINTR) continue;
        dead = true;  // n == 0: peer closed
        break;
      }
      size_t start = 0;
      while (!dead && rx.size() - start >= sizeof(CommonHeader) &&
             inflight < 256) {
        CommonHeader chh;
        memcpy(&chh, rx.data() + start, sizeof(chh));
        if (chh.hlen < sizeof(chh) || chh.plen < chh.hlen ||
            chh.plen > (64u << 20)) {
          dead = true;
          break;
        }
        if (rx.size() - start < chh.plen) break;
        handle_pdu(reinterpret_cast<const uint8_t*>(rx.data()) + start, chh);
        start += chh.plen;
      }
      rx.erase(0, start);
      int completed = 0;
      for (auto& [bdev, channel] : channels) {
        completed += bdev->poll(channel.get());
      }
      if (completed == 0 && start == 0) {
        __builtin_ia32_pause();
        // Every 32nd idle spin, offer the core: when the scheduler has
        // placed the peer's polling thread on this core, a pure spinner
        // holds it until the next tick and each I/O costs milliseconds.
        if ((++idle_spins & 31) == 0) sched_yield();
      } else {
        idle_spins = 0;
      }
    }
    // Drain in-flight completions so pool buffers are not freed under
    // a pending I/O.
    const auto deadline =
        std::chrono::steady_clock::now() + std::chrono::seconds(10);
    while (inflight > 0 && std::chrono::steady_clock::now() < deadline) {
      for (auto& [bdev, channel] : channels) bdev->poll(channel.get());
    }
    for (auto& pb : pool) free_pinned(pb.ptr);
  }

  std::string subnqn_;
  bool digests_;
  int listen_fd_ = -1;
  uint16_t port_ = 0;
  std::atomic<bool> running_{false};
  std::thread accept_thread_;
  std::mutex mutex_;
  std::vector<std::pair<std::thread, std::shared_ptr<std::atomic<bool>>>>
      connections_;
  std::vector<BdevPtr> namespaces_;
};

}  // namespace

std::shared_ptr<NvmfTcpTarget> start_nvmf_tcp_target(
    const std::string& listen_addr, uint16_t port, const std::string& subnqn,
    bool enable_digests) {
  auto target = std::make_shared<TargetImpl>(listen_addr, port, subnqn,
                                             enable_digests);
  target->start();
  return target;
}

}  // namespace hipstore
