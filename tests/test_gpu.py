"""MI355X GPU tests: HBM bdev numerics + kernels vs CPU references.

All marked `gpu`; run via `pytest -m gpu` on a GPU box. Every data-path
result is compared against plain host-side byte operations (the CPU
reference), and CRC32C against the bit-exact software table.
"""

import os
import random

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")


@needs_gpu
class TestHbmBdev:
    @pytest.fixture(scope="class")
    def bdev(self):
        # 64 MiB HBM bdev
        return hs.create_hbm_bdev("gpu-test", 512, 131072, device=0)

    def test_roundtrip_single_block(self, bdev):
        payload = bytes(random.getrandbits(8) for _ in range(512))
        bdev.write(0, payload)
        assert bdev.read(0, 512) == payload

    def test_roundtrip_large_offsets(self, bdev):
        rng = random.Random(7)
        blob = bytes(rng.getrandbits(8) for _ in range(64 * 1024))
        offset = 32 * 1024 * 1024 + 4096
        bdev.write(offset, blob)
        assert bdev.read(offset, len(blob)) == blob
        # Neighbors untouched (bdev zero-initialized)
        assert bdev.read(offset - 512, 512) == b"\x00" * 512
        assert bdev.read(offset + len(blob), 512) == b"\x00" * 512

    def test_fill(self, bdev):
        bdev.fill(1024 * 1024, 0xCD, 8192)
        assert bdev.read(1024 * 1024, 8192) == b"\xcd" * 8192

    def test_unaligned_tail(self, bdev):
        # 512-byte granularity I/O smaller than one 4 KiB tile
        payload = bytes(random.getrandbits(8) for _ in range(1536))
        bdev.write(2048, payload)
        assert bdev.read(2048, 1536) == payload

    def test_out_of_bounds(self, bdev):
        with pytest.raises(RuntimeError):
            bdev.read(bdev.size_bytes, 512)
        with pytest.raises(RuntimeError):
            bdev.write(bdev.size_bytes - 512, b"x" * 1024)

    def test_persistence_across_channels(self, bdev):
        # Data survives independent I/O sessions (the Malloc bdev
        # contract: survives Map/Unmap, reference spec.md:116-119).
        bdev.write(4096, b"\xee" * 512)
        assert bdev.read(4096, 512) == b"\xee" * 512


@needs_gpu
class TestPersistentEngine:
    """The on-GPU polling service kernel: same numerics contract as the
    batched engine, verified against host byte references."""

    @pytest.fixture(scope="class")
    def bdev(self):
        return hs.create_hbm_bdev("gpu-pers", 512, 131072, device=0,
                                  persistent=True)

    def test_roundtrip(self, bdev):
        rng = random.Random(41)
        blob = bytes(rng.getrandbits(8) for _ in range(64 * 1024))
        bdev.write(8192, blob)
        assert bdev.read(8192, len(blob)) == blob

    def test_fill_and_small_blocks(self, bdev):
        bdev.fill(0, 0x3C, 4096)
        assert bdev.read(0, 512) == b"\x3c" * 512
        payload = bytes(random.getrandbits(8) for _ in range(512))
        bdev.write(512, payload)
        assert bdev.read(512, 512) == payload

    def test_idle_exit_and_relaunch(self, bdev):
        """I/O keeps working across an idle period longer than the
        service kernel's idle exit (~1 s).

        This does NOT exercise relaunch: every bdev.write/read takes a
        fresh channel, whose constructor launches a new service kernel
        with a zero completed prefix. Relaunch from poll() on a live
        channel (non-zero prefix) is covered by
        test_engine_matrix.py::test_relaunch_on_live_channel."""
        import time
        bdev.write(0, b"\x11" * 512)
        time.sleep(2.5)  # beyond the idle timeout
        bdev.write(512, b"\x22" * 512)
        assert bdev.read(0, 512) == b"\x11" * 512
        assert bdev.read(512, 512) == b"\x22" * 512

    def test_perf_sanity(self):
        bdev = hs.create_hbm_bdev("gpu-pers-perf", 4096, 262144, device=0,
                                  persistent=True)
        bdev.fill(0, 0x5A, bdev.size_bytes)
        r = hs.run_bdevperf(bdev, "randread", 4096, 32, 4, 1.0)
        assert r["iops"] > 100_000, r


@needs_gpu
class TestHbmCapacity:
    def test_quarter_terabyte_bdev(self):
        """Size for the hardware: a 256 GiB HBM bdev (of 288 GB) with
        I/O at the far end of the address space."""
        try:
            bdev = hs.create_hbm_bdev("huge", 4096, (256 << 30) // 4096,
                                      device=0)
        except RuntimeError as exc:
            pytest.skip(f"insufficient free HBM: {exc}")
        payload = bytes(random.getrandbits(8) for _ in range(4096))
        far = bdev.size_bytes - 4096
        bdev.write(far, payload)
        bdev.write(0, payload[::-1])
        assert bdev.read(far, 4096) == payload
        assert bdev.read(0, 4096) == payload[::-1]
        del bdev  # free 256 GiB before later tests


@needs_gpu
class TestCrc32c:
    def test_gpu_matches_software(self):
        bdev = hs.create_hbm_bdev("crc-test", 4096, 256, device=0)
        rng = random.Random(13)
        blocks = [bytes(rng.getrandbits(8) for _ in range(4096)) for _ in range(16)]
        for i, blk in enumerate(blocks):
            bdev.write(i * 4096, blk)
        gpu = hs.crc32c_gpu_blocks(bdev, 0, 4096, 16)
        sw = [hs.crc32c(blk) for blk in blocks]
        assert list(gpu) == sw

    def test_known_answer(self):
        assert hs.crc32c(b"123456789") == 0xE3069283

    @pytest.fixture(scope="class")
    def digest_rig(self):
        """8 MiB of random bytes on a 512-byte-block bdev + the same
        bytes on the host (the reference input, never modified)."""
        bdev = hs.create_hbm_bdev("crc-shapes", 512, 16384, device=0)
        data = random.Random(17).randbytes(bdev.size_bytes)
        bdev.write(0, data)
        return bdev, data

    @staticmethod
    def _table_blocks(data, offset, block, count):
        return [hs.crc32c_table(data[offset + i * block:
                                     offset + (i + 1) * block])
                for i in range(count)]

    @pytest.mark.parametrize("block", [512, 4096])
    def test_block_counts_and_offset(self, digest_rig, block):
        """One lane per block: counts across the wave (64) and workgroup
        (256) boundaries, several workgroups, and 1025 last so the
        thread-local result buffer (1024 entries at first) grows after
        smaller calls. Offset is block-aligned, not 4 KiB-aligned."""
        bdev, data = digest_rig
        offset = 3 * 512
        for count in (1, 63, 64, 65, 255, 256, 257, 1025):
            gpu = hs.crc32c_gpu_blocks(bdev, offset, block, count)
            assert list(gpu) == self._table_blocks(data, offset, block,
                                                   count), (block, count)
        # offset 0 and a smaller call after the buffer grew
        assert list(hs.crc32c_gpu_blocks(bdev, 0, block, 65)) == \
            self._table_blocks(data, 0, block, 65)

    def test_zero_count_is_empty(self, digest_rig):
        bdev, _ = digest_rig
        assert list(hs.crc32c_gpu_blocks(bdev, 512, 4096, 0)) == []

    def test_rejects_bad_arguments(self, digest_rig):
        bdev, _ = digest_rig
        with pytest.raises(RuntimeError):
            hs.crc32c_gpu_blocks(bdev, 0, 4098, 1)   # not a multiple of 4
        with pytest.raises(RuntimeError):
            hs.crc32c_gpu_blocks(bdev, bdev.size_bytes - 4096, 4096, 2)
        with pytest.raises(RuntimeError):
            hs.crc32c_gpu_blocks(bdev, 100, 512, 1)  # offset not on a block

    @pytest.mark.parametrize("offset,length", [
        (0, 4096), (0, 8192), (0, (1 << 20) + 4096),
        (5 * 512, 4096), (5 * 512, (1 << 20) + 4096)])
    def test_range_digest(self, digest_rig, offset, length):
        """Per-4 KiB GPU CRCs folded by the combine ladder (the digest
        of the NVMe-oF and rados large-extent paths) against the table
        CRC of the same bytes: one block (no combine), two, and 257."""
        bdev, data = digest_rig
        assert hs.crc32c_gpu_range(bdev, offset, length) == \
            hs.crc32c_table(data[offset:offset + length])

    def test_range_digest_rejects_partial_blocks(self, digest_rig):
        bdev, _ = digest_rig
        for length in (0, 512, 4096 + 512):
            with pytest.raises(RuntimeError):
                hs.crc32c_gpu_range(bdev, 0, length)


@needs_gpu
class TestPerf:
    def test_randread_sanity(self):
        bdev = hs.create_hbm_bdev("perf-gpu", 4096, 262144, device=0)  # 1 GiB
        bdev.fill(0, 0x5A, bdev.size_bytes)
        # An MI355X must beat 100k IOPS trivially; guards against a
        # silently serialized path. Warm up and allow one retry: some
        # pool boxes sit in a low-power state and the batched engine's
        # bursty launches eat multi-second clock-ramp stalls on the
        # first run (observed 6 s outliers; the always-busy persistent
        # engine is immune, and the same test is clean immediately
        # after — this is a sanity guard, not a benchmark).
        hs.run_bdevperf(bdev, "randread", 4096, 32, 4, 0.5)  # warm
        last = None
        for _ in range(2):
            last = hs.run_bdevperf(bdev, "randread", 4096, 32, 4, 1.0)
            if last["iops"] > 100_000 and last["lat_p99_us"] < 100_000:
                break
        assert last["iops"] > 100_000, last
        assert last["lat_p99_us"] < 100_000, last

    def test_randwrite_correct_and_fast(self):
        bdev = hs.create_hbm_bdev("perfw-gpu", 4096, 65536, device=0)
        hs.run_bdevperf(bdev, "randwrite", 4096, 32, 2, 0.3)  # warm
        last = None
        for _ in range(2):
            last = hs.run_bdevperf(bdev, "randwrite", 4096, 32, 2, 0.5)
            if last["iops"] > 50_000:
                break
        assert last["iops"] > 50_000, last


@needs_gpu
class TestCompositeGpu:
    def test_striped_hbm_correctness(self):
        # Two HBM children (same device on a 1-GPU box; stripe logic is
        # identical across devices).
        children = [hs.create_hbm_bdev(f"sg-{i}", 512, 65536, device=0)
                    for i in range(2)]
        bdev = hs.create_striped_bdev("sg", children, 65536)
        rng = random.Random(11)
        data = bytes(rng.getrandbits(8) for _ in range(4 * 65536))
        bdev.write(0, data)
        assert bdev.read(0, len(data)) == data
        # stripe unit 1 lives on child 1 at offset 0
        assert children[1].read(0, 65536) == data[65536:2 * 65536]
        r = hs.run_bdevperf(bdev, "randread", 4096, 32, 2, 0.5)
        assert r["iops"] > 50_000, r

    @pytest.mark.skipif(hs.gpu_device_count() < 2,
                        reason="needs >=2 GPUs for xGMI replication")
    def test_replicated_xgmi_fanout(self):
        children = [hs.create_hbm_bdev(f"rg-{i}", 512, 65536, device=i)
                    for i in range(2)]
        bdev = hs.create_replicated_bdev("rg", children)
        rng = random.Random(13)
        data = bytes(rng.getrandbits(8) for _ in range(16 * 4096))
        bdev.write(8192, data)
        # Every replica holds the data (replica 1 was filled over xGMI
        # peer copy from device 0).
        for child in children:
            assert child.read(8192, len(data)) == data

    @pytest.mark.skipif(hs.gpu_device_count() < 3,
                        reason="needs >=3 GPUs for RCCL broadcast fan-out")
    def test_replicated_rccl_broadcast(self):
        """>=3 replicas use ncclBroadcast over xGMI for the fan-out."""
        n = min(hs.gpu_device_count(), 4)
        children = [hs.create_hbm_bdev(f"rc-{i}", 512, 65536, device=i)
                    for i in range(n)]
        bdev = hs.create_replicated_bdev("rc", children)
        rng = random.Random(17)
        data = bytes(rng.getrandbits(8) for _ in range(64 * 4096))
        bdev.write(4096, data)
        for child in children:
            assert child.read(4096, len(data)) == data


@needs_gpu
class TestHbmCopy:
    def test_same_device_copy(self):
        a = hs.create_hbm_bdev("cp-a", 4096, 16384, device=0)  # 64 MiB
        b = hs.create_hbm_bdev("cp-b", 4096, 16384, device=0)
        rng = random.Random(51)
        blob = bytes(rng.getrandbits(8) for _ in range(1 << 20))
        a.write(4096, blob)
        hs.hbm_copy(a, 4096, b, 8192, len(blob))
        assert b.read(8192, len(blob)) == blob
        # sub-tile granularity (16-byte aligned lengths); read back a
        # whole block (bdev reads are block-granular)
        hs.hbm_copy(a, 4096, b, 0, 512)
        assert b.read(0, 4096)[:512] == blob[:512]

    SENTINEL = 0xEE

    @pytest.fixture(scope="class")
    def copy_rig(self):
        """Source bdev holding random bytes (the reference input) and a
        destination bdev; both 512-byte blocks, 16 MiB."""
        src = hs.create_hbm_bdev("cp-src", 512, 32768, device=0)
        dst = hs.create_hbm_bdev("cp-dst", 512, 32768, device=0)
        blob = random.Random(57).randbytes(src.size_bytes)
        src.write(0, blob)
        return src, dst, blob

    @pytest.mark.parametrize("length", [16, 4080, 4096 + 16,
                                        (8 << 20) + 48])
    def test_range_copy_edges(self, copy_rig, length):
        """k_copy_range at float4 counts that are no multiple of the
        256-thread workgroup; (8 MiB + 48) / 16 = 2048*256 + 3 elements
        makes the grid-stride loop run a second, ragged pass. Offsets
        are 16-aligned but not block- or tile-aligned; the destination
        is pre-filled so bytes on either side must stay untouched."""
        src, dst, blob = copy_rig
        src_off = 4096 + 48
        dst_off = 8192 + 80
        dst.fill(0, self.SENTINEL, dst.size_bytes)
        hs.hbm_copy(src, src_off, dst, dst_off, length)
        lo = (dst_off - 16) // 512 * 512
        hi = -(-(dst_off + length + 16) // 512) * 512
        region = dst.read(lo, hi - lo)
        head = dst_off - lo
        assert region[:head] == bytes([self.SENTINEL]) * head
        assert region[head:head + length] == blob[src_off:src_off + length]
        tail = len(region) - head - length
        assert tail >= 16
        assert region[head + length:] == bytes([self.SENTINEL]) * tail

    def test_rejects_misaligned_offsets(self, copy_rig):
        src, dst, _ = copy_rig
        for src_off, dst_off in ((8, 0), (0, 8), (4100, 4096), (16, 4097)):
            with pytest.raises(RuntimeError):
                hs.hbm_copy(src, src_off, dst, dst_off, 4096)

    def test_rejects_overlap_within_one_bdev(self, copy_rig):
        src, _, blob = copy_rig
        for src_off, dst_off, length in ((0, 16, 4096),       # forward
                                         (4096, 4096 - 16, 4096),  # backward
                                         (8192, 8192, 512),   # identical
                                         (0, 4096 - 16, 4096)):  # last 16 B
            with pytest.raises(RuntimeError):
                hs.hbm_copy(src, src_off, src, dst_off, length)
        # rejected before any launch: the source is unchanged
        assert src.read(0, 16384) == blob[:16384]

    def test_copy_within_one_bdev(self):
        bdev = hs.create_hbm_bdev("cp-self", 512, 4096, device=0)
        blob = random.Random(59).randbytes(8192)
        bdev.write(0, blob)
        # adjacent, not overlapping: [16, 4112) -> [4112, 8208)
        hs.hbm_copy(bdev, 16, bdev, 4096 + 16, 4096)
        expect = bytearray(blob + b"\0" * 512)
        expect[4112:8208] = blob[16:4112]
        assert len(expect) == 8704
        assert bdev.read(0, 8704) == bytes(expect)

    def test_rejects_cpu_bdev(self):
        a = hs.create_hbm_bdev("cp-c", 4096, 1024, device=0)
        c = hs.create_malloc_bdev("cp-d", 4096, 1024)
        with pytest.raises(RuntimeError):
            hs.hbm_copy(a, 0, c, 0, 4096)

    @pytest.mark.skipif(hs.gpu_device_count() < 2,
                        reason="needs >=2 GPUs for xGMI copy")
    def test_cross_device_copy(self):
        a = hs.create_hbm_bdev("cp-x0", 4096, 16384, device=0)
        b = hs.create_hbm_bdev("cp-x1", 4096, 16384, device=1)
        rng = random.Random(53)
        blob = bytes(rng.getrandbits(8) for _ in range(1 << 20))
        a.write(0, blob)
        hs.hbm_copy(a, 0, b, 0, len(blob))
        assert b.read(0, len(blob)) == blob


@needs_gpu
class TestNvmfGpu:
    def test_hbm_namespace_gpu_digest_roundtrip(self):
        """NVMe/TCP loopback with an HBM-resident namespace; the
        initiator verifies every C2HData digest in software, so a
        mismatch anywhere fails the read.

        The digests here come from the HOST CRC, not the GPU kernel:
        the target digests PDUs of at most 128 KiB and takes the GPU
        branch only from 1 MiB up when it holds a host copy, so that
        branch cannot be reached from the NVMe-oF read path. The GPU
        per-4 KiB CRC + combine ladder is tested directly by
        TestCrc32c::test_range_digest."""
        backing = hs.create_hbm_bdev("nvmf-hbm", 4096, 16384, device=0)
        target = hs.start_nvmf_tcp_target(
            "", 0, "nqn.2026-01.com.amd:gpu-ns", True)
        target.add_namespace(backing)
        try:
            bdev = hs.create_nvmf_tcp_bdev(
                "nvmf-gpu", "127.0.0.1", target.port,
                "nqn.2026-01.com.amd:gpu-ns")
            rng = random.Random(31)
            data = bytes(rng.getrandbits(8) for _ in range(128 * 1024))
            bdev.write(0, data)
            # 128 KiB aligned read -> one digested C2HData PDU
            assert bdev.read(0, len(data)) == data
            assert backing.read(0, len(data)) == data
            r = hs.run_bdevperf(bdev, "randread", 65536, 8, 2, 0.5)
            assert r["iops"] > 100, r
        finally:
            target.stop()


@needs_gpu
class TestDaemonHbm:
    def test_daemon_gpu_mode(self, tmp_path):
        fixture = launch_hipstored(tmp_path, cpu=False)
        try:
            with hipstore.Client(fixture.socket_path) as client:
                name = hipstore.construct_malloc_bdev(
                    client, num_blocks=262144, block_size=4096, name="hbm0")
                bdevs = hipstore.get_bdevs(client, name)
                assert bdevs[0].product_name == "Malloc disk"
                assert "hbm" in bdevs[0].driver_specific
                pci = bdevs[0].driver_specific["hbm"]["pci_address"]
                assert pci.count(":") == 2
                result = hipstore.perf_run(client, "hbm0", io_size=4096,
                                           queue_depth=32, num_queues=4,
                                           seconds=1.0)
                assert result["iops"] > 100_000, result
                hipstore.delete_bdev(client, name)
        finally:
            fixture.stop()


@needs_gpu
class TestCapacityReporting:
    def test_hbm_info(self):
        total, free = hs.hbm_info(0)
        assert total > 200 << 30  # 288 GB class
        assert 0 < free <= total

    def test_csi_get_capacity_local_mode(self, tmp_path):
        import grpc

        from oim_amd.common.server import grpc_target
        from oim_amd.csidriver import FakeExec, LocalBackend, Mounter, OIMDriver
        from oim_amd.spec import csi_v1 as csi
        from oim_amd.spec.rpc_csi import CSIControllerStub

        fixture = launch_hipstored(tmp_path, cpu=False)
        driver = OIMDriver(driver_name="oim-local", node_id="n0",
                           endpoint=f"unix://{tmp_path}/csi.sock",
                           backend=LocalBackend(fixture.socket_path),
                           mounter=Mounter(FakeExec()))
        driver.start()
        try:
            with grpc.insecure_channel(grpc_target(driver.addr())) as ch:
                stub = CSIControllerStub(ch)
                response = stub.GetCapacity(csi.GetCapacityRequest(), timeout=30)
                assert response.available_capacity > 100 << 30
                caps = stub.ControllerGetCapabilities(
                    csi.ControllerGetCapabilitiesRequest(), timeout=30)
                types = {c.rpc.type for c in caps.capabilities}
                assert csi.CTRL_CAP_GET_CAPACITY in types
        finally:
            driver.stop()
            fixture.stop()


@needs_gpu
class TestInvalidWorkload:
    def test_unaligned_io_size_fails_cleanly(self):
        """io_size below the block size must error out, not hang
        (regression: failed resubmissions mutated the immediate list
        mid-iteration)."""
        bdev = hs.create_hbm_bdev("inv-gpu", 4096, 65536, device=0,
                                  persistent=True)
        with pytest.raises(RuntimeError):
            hs.run_bdevperf(bdev, "randread", 512, 8, 2, 0.5)


@needs_gpu
class TestChannelAutoFallback:
    """Past the per-device HW-queue cap (18 per-queue service kernels),
    new channels transparently fall back to the batched engine; IO on
    a mixed per-queue + batched channel set stays correct.

    Round-1's "mixed-engine wedge" was a HOST bug, not a GPU mystery:
    HbmBdev::poll() dispatched on bdev-level flags, so fallback
    channels were polled through the wrong class (batched-on-
    persistent read garbage and stalled; shared fallbacks segfaulted).
    poll() now dispatches on the channel's kind like submit() always
    did, and these run by default again. Every wait is bounded, so a
    regression costs seconds, not the suite budget.
    """

    @pytest.mark.timeout(120)
    def test_low_cap_mixed_engines(self, monkeypatch):
        """4 per-queue + 2 batched via HIPSTORE_PERQ_CAP=4 — exercises
        the fallback decision and mixed-kind dispatch with small
        resident-kernel counts."""
        import subprocess, sys, os
        script = os.path.join(os.path.dirname(__file__), "_qsweep_debug.py")
        env = dict(os.environ, HIPSTORE_PERQ_CAP="4")
        proc = subprocess.run([sys.executable, script, "6"], env=env,
                              capture_output=True, text=True, timeout=100)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        assert "ios=" in proc.stdout

    @pytest.mark.timeout(180)
    def test_22_queues_mixed_engines(self):
        bdev = hs.create_hbm_bdev("fallback-0", 4096, 262144, device=0,
                                  persistent=True)
        result = hs.run_bdevperf(bdev, "randread", 4096, 8, 22, 20.0,
                                 max_ios=200000)
        assert result["io_count"] >= 200000
        del bdev, result
        # shared-fallback flavour at a tiny cap (the round-1
        # segfaulting config), isolated in its own process
        import subprocess
        import sys as sys_mod
        script = os.path.join(os.path.dirname(__file__),
                              "_qsweep_debug.py")
        env = dict(os.environ, HIPSTORE_PERQ_CAP="4",
                   HIPSTORE_FALLBACK="shared")
        proc = subprocess.run([sys_mod.executable, script, "6"],
                              env=env, capture_output=True, text=True,
                              timeout=100)
        assert proc.returncode == 0, proc.stdout + proc.stderr
        bdev = hs.create_hbm_bdev("fallback-1", 4096, 262144, device=0,
                                  persistent=True)
        result = hs.run_bdevperf(bdev, "randread", 4096, 8, 2, 5.0,
                                 max_ios=20000)
        assert result["io_count"] >= 20000
        # correctness across the cap boundary
        import random
        rng = random.Random(11)
        data = bytes(rng.getrandbits(8) for _ in range(8 * 4096))
        bdev.write(64 * 4096, data)
        assert bdev.read(64 * 4096, len(data)) == data


@needs_gpu
class TestHbmResize:
    """Offline HBM bdev expansion: data survives the backing-store
    move; live channels refuse the resize (kIoFailed)."""

    def test_grow_preserves_data(self):
        import os as _os
        bdev = hs.create_hbm_bdev("resize-0", 512, 2048, device=0,
                                  persistent=True)
        data = _os.urandom(4096)
        bdev.write(0, data)
        session = hs.PerfSession(bdev, "randread", 512, 1, 1)
        session.step(10)
        assert bdev.resize(65536) == -5  # busy: channels hold the base
        del session
        assert bdev.resize(65536) == 0
        assert bdev.num_blocks == 65536
        assert bdev.read(0, 4096) == data  # moved with the store
        tail = _os.urandom(512)
        bdev.write(65535 * 512, tail)  # new extent is addressable
        assert bdev.read(65535 * 512, 512) == tail
        # grown region arrived zeroed
        assert bdev.read(4096, 512) == b"\0" * 512

    def test_grow_from_three_blocks(self):
        """Kept prefix of 1536 bytes: 96 float4s, less than one
        workgroup and no multiple of a tile."""
        bdev = hs.create_hbm_bdev("resize-1", 512, 3, device=0)
        data = random.Random(61).randbytes(1536)
        bdev.write(0, data)
        assert bdev.resize(64) == 0
        assert bdev.num_blocks == 64
        assert bdev.read(0, 64 * 512) == data + b"\0" * (61 * 512)

    def test_shrink_then_grow_shows_zeros(self):
        bdev = hs.create_hbm_bdev("resize-2", 512, 24, device=0)
        data = random.Random(62).randbytes(24 * 512)
        bdev.write(0, data)
        assert bdev.resize(5) == 0            # shrink keeps the prefix
        assert bdev.num_blocks == 5
        assert bdev.read(0, 5 * 512) == data[:5 * 512]
        with pytest.raises(RuntimeError):
            bdev.read(5 * 512, 512)           # cut off
        assert bdev.resize(24) == 0           # grow again
        # the old tail is gone: zeros, not blocks 5..23 of `data`
        assert bdev.read(0, 24 * 512) == data[:5 * 512] + b"\0" * (19 * 512)


@pytest.mark.gpu
class TestEngineContractProbes:
    """Hardware-contract probes (round-2 diagnosis tooling, kept as
    regression guards): every leg of the host<->GPU polling contract,
    and the real service kernel serving a descriptor from a minimal
    standalone harness. A red here pinpoints WHICH leg broke (e.g. the
    firmware __threadfence_system wave-hang this caught)."""

    def test_polling_contract_legs(self):
        r = hs.persistent_probe(0, 1)
        assert r["launch_err"] == 0
        assert r["hb_host_early"] > 0, "GPU->host pinned heartbeat"
        assert r["hb_dev_early"] > 0, "kernel runs at all"
        assert r["cq0_ms"] >= 0, "host tail -> leader -> CQ publish"
        assert r["cq1_ms"] >= 0, "leader -> worker agent relay"
        assert r["stream_drained"] == 1

    @pytest.mark.parametrize("variant", [0, 1, 2])
    def test_service_kernel_serves(self, variant):
        r = hs.persistent_kernel_probe(0, variant)
        assert r["launch_err"] == 0
        assert r["cq_ms"] >= 0, "service kernel must publish its CQ"
        if variant != 1:
            assert r["data_ok"] == 1
        assert r["dev_known"] == 1
        assert r["stream_drained"] == 1
