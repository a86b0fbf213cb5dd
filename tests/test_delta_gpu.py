"""hipstore::k_pack_marked / k_unpack_marked on HBM bdevs, and delta
files of HBM volumes through the daemon.

The yardsticks are a Python byte model (every granule carries its own
index) and the generic host path on a malloc twin with the same
content. Shapes mirror test_bdev_diff_gpu.py: the same work split can
go wrong in the same places. All ranges are validated on the host
before any launch."""

import random

import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

BLOCK = 512
MAX_WGS = 2048
# More bitmap words than workgroups, twice over, plus a ragged tail.
N = 2 * MAX_WGS * 64 + 65
FIXED = [0, 63, 64, 65, MAX_WGS * 64 - 1, MAX_WGS * 64, N - 1]


def indexed_bytes(n_blocks, salt=0):
    """Block i is the u32 (i + salt) repeated: every granule distinct."""
    return np.repeat(np.arange(salt, salt + n_blocks, dtype=np.uint32),
                     BLOCK // 4).tobytes()


def model_bitmap(n_granules, marked, stray=()):
    out = bytearray((n_granules + 7) // 8)
    for g in marked:
        assert 0 <= g < n_granules
        out[g // 8] |= 1 << (g % 8)
    for g in stray:
        assert n_granules <= g < 8 * len(out)
        out[g // 8] |= 1 << (g % 8)
    return bytes(out)


def model_pack(data, granule, marked, offset=0):
    return b"".join(data[offset + g * granule:offset + (g + 1) * granule]
                    for g in sorted(marked))


def model_unpack(target, granule, marked, dense, offset=0):
    out = bytearray(target)
    for i, g in enumerate(sorted(marked)):
        out[offset + g * granule:offset + (g + 1) * granule] = \
            dense[i * granule:(i + 1) * granule]
    return bytes(out)


@pytest.fixture(scope="module")
def volume():
    """HBM bdev and malloc twin with the same indexed content, the
    content itself and the sparse set of 512 B granules. Read-only."""
    data = indexed_bytes(N)
    hbm = hs.create_hbm_bdev("pk-h", BLOCK, N, device=0)
    twin = hs.create_malloc_bdev("pk-m", BLOCK, N)
    for bdev in (hbm, twin):
        bdev.write(0, data)
    rng = random.Random(20262)
    sparse = sorted(set(FIXED) | set(rng.sample(range(N), 50)))
    return {"hbm": hbm, "twin": twin, "data": data, "sparse": sparse}


@needs_gpu
class TestPackKernel:
    def test_sparse_matches_model_and_generic_path(self, volume):
        marked = volume["sparse"]
        bitmap = model_bitmap(N, marked)
        got = hs.bdev_pack_marked(volume["hbm"], bitmap, BLOCK)
        assert got == model_pack(volume["data"], BLOCK, marked)
        assert got == hs.bdev_pack_marked(volume["twin"], bitmap, BLOCK)

    @pytest.mark.parametrize("granule", [1024, 1536, 4096])
    def test_other_granules(self, volume, granule):
        per = granule // BLOCK
        n = N // per
        marked = sorted({g // per for g in volume["sparse"] if g // per < n})
        bitmap = model_bitmap(n, marked)
        got = hs.bdev_pack_marked(volume["hbm"], bitmap, granule,
                                  length=n * granule)
        assert got == model_pack(volume["data"], granule, marked)
        assert got == hs.bdev_pack_marked(volume["twin"], bitmap, granule,
                                          length=n * granule)

    def test_shifted_offset(self, volume):
        off = 7 * BLOCK
        n = N - 7
        marked = sorted({g - 7 for g in volume["sparse"] if g >= 7} | {0})
        bitmap = model_bitmap(n, marked)
        got = hs.bdev_pack_marked(volume["hbm"], bitmap, BLOCK,
                                  src_offset=off)
        assert got == model_pack(volume["data"], BLOCK, marked, offset=off)
        assert got == hs.bdev_pack_marked(volume["twin"], bitmap, BLOCK,
                                          src_offset=off)

    @pytest.mark.parametrize("every", [1, 3])
    def test_dense_windows(self, every):
        """Every bit, then every third: 3-granule staging cuts windows
        inside bitmap words, 64 granules cuts them at half words."""
        n = 64 * 40 + 5
        data = indexed_bytes(n, salt=7)
        hbm = hs.create_hbm_bdev(f"pk-d{every}", BLOCK, n, device=0)
        twin = hs.create_malloc_bdev(f"pk-dm{every}", BLOCK, n)
        hbm.write(0, data)
        twin.write(0, data)
        marked = list(range(0, n, every))
        bitmap = model_bitmap(n, marked)
        want = model_pack(data, BLOCK, marked)
        for staging in (3 * BLOCK, 64 * BLOCK, 0):
            assert hs.bdev_pack_marked(hbm, bitmap, BLOCK,
                                       staging_bytes=staging) == want
            assert hs.bdev_pack_marked(twin, bitmap, BLOCK,
                                       staging_bytes=staging) == want

    def test_stray_tail_bits_and_empty(self, volume):
        n = 70
        marked = [0, 64, 69]
        stray = [70, 71]
        want = model_pack(volume["data"], BLOCK, marked)
        for staging in (0, 3 * BLOCK):
            got = hs.bdev_pack_marked(
                volume["hbm"], model_bitmap(n, marked, stray), BLOCK,
                length=n * BLOCK, staging_bytes=staging)
            assert got == want
        # stray bits in a word of their own past the range
        long_bitmap = model_bitmap(n, marked) + b"\x00\x00\x00\xff" * 4
        assert hs.bdev_pack_marked(volume["hbm"], long_bitmap, BLOCK,
                                   length=n * BLOCK) == want
        assert hs.bdev_pack_marked(volume["hbm"], bytes((N + 7) // 8),
                                   BLOCK) == b""
        assert hs.bdev_pack_marked(volume["hbm"], model_bitmap(n, [], stray),
                                   BLOCK, length=n * BLOCK) == b""


@needs_gpu
class TestUnpackKernel:
    @pytest.mark.parametrize("staging", [0, 3 * BLOCK])
    def test_scatter_into_filled_target(self, volume, staging):
        marked = volume["sparse"]
        bitmap = model_bitmap(N, marked)
        dense = model_pack(volume["data"], BLOCK, marked)
        target = hs.create_hbm_bdev(f"pk-t{staging}", BLOCK, N, device=0)
        target.fill(0, 0xA5, N * BLOCK)
        assert hs.bdev_unpack_marked(target, bitmap, BLOCK, dense,
                                     staging_bytes=staging) == len(marked)
        want = model_unpack(b"\xA5" * (N * BLOCK), BLOCK, marked, dense)
        assert target.read(0, N * BLOCK) == want

    def test_coarse_granule_with_offset_and_stray_bits(self):
        granule = 1536
        n = 64 * 3 + 9
        off = 2 * granule
        total = (n + 4) * granule
        target = hs.create_hbm_bdev("pk-u", BLOCK, total // BLOCK, device=0)
        twin = hs.create_malloc_bdev("pk-um", BLOCK, total // BLOCK)
        for bdev in (target, twin):
            bdev.fill(0, 0xA5, total)
        marked = [0, 1, 15, 16, 63, 64, 127, 128, n - 1]
        dense = indexed_bytes(len(marked) * granule // BLOCK, salt=1000)
        bitmap = model_bitmap(n, marked, stray=[n, n + 5])
        for bdev in (target, twin):
            assert hs.bdev_unpack_marked(
                bdev, bitmap, granule, dense, dst_offset=off,
                length=n * granule, staging_bytes=4 * granule) == len(marked)
        want = model_unpack(b"\xA5" * total, granule, marked, dense,
                            offset=off)
        assert target.read(0, total) == want
        assert twin.read(0, total) == want

    def test_round_trip_leaves_unmarked_differences(self, volume):
        """Pack from a, unpack into a copy of b: bdev_diff(a, copy) shows
        exactly the differing granules that were not marked."""
        a = volume["hbm"]
        differing = volume["sparse"]
        copy = hs.create_hbm_bdev("pk-c", BLOCK, N, device=0)
        hs.hbm_copy(a, 0, copy, 0, N * BLOCK)
        for g in differing:  # b: a with the sparse granules overwritten
            copy.write(g * BLOCK, b"\xEE" * BLOCK)
        marked = differing[::2]
        left = differing[1::2]
        extra = [g for g in (1000, MAX_WGS * 64 + 7) if g not in differing]
        bitmap = model_bitmap(N, marked + extra)
        dense = hs.bdev_pack_marked(a, bitmap, BLOCK)
        assert hs.bdev_unpack_marked(copy, bitmap, BLOCK, dense) == \
            len(marked + extra)
        r = hs.bdev_diff(a, copy, max_report=1024)
        assert r["first_mismatches"] == left
        assert r["bitmap"] == model_bitmap(N, left)


@needs_gpu
class TestRejectedBeforeLaunch:
    def test_pack(self, volume):
        hbm = volume["hbm"]
        full = bytes([0xFF]) * ((N + 7) // 8)
        for granule, kwargs in (
                (768, {}),
                (BLOCK, {"src_offset": 100, "length": BLOCK}),
                (BLOCK, {"length": (N + 1) * BLOCK}),
                (BLOCK, {"src_offset": N * BLOCK, "length": BLOCK}),
                (BLOCK, {"src_offset": 2**64 - BLOCK}),
                (BLOCK, {"src_offset": 2**64 - BLOCK, "length": 2 * BLOCK}),
                (4096, {"staging_bytes": 4095})):
            with pytest.raises(RuntimeError):
                hs.bdev_pack_marked(hbm, full, granule, **kwargs)
        with pytest.raises(RuntimeError):  # short bitmap
            hs.bdev_pack_marked(hbm, b"\xff", BLOCK, length=9 * BLOCK)

    def test_unpack(self):
        target = hs.create_hbm_bdev("pk-r", BLOCK, 128, device=0)
        target.fill(0, 0xA5, 128 * BLOCK)
        one = bytes(BLOCK)
        for granule, data, kwargs in (
                (768, bytes(768), {}),
                (BLOCK, one, {"dst_offset": 100, "length": BLOCK}),
                (BLOCK, one, {"length": 129 * BLOCK}),
                (BLOCK, one, {"dst_offset": 2**64 - BLOCK}),
                (BLOCK, one, {"dst_offset": 2**64 - BLOCK,
                              "length": 2 * BLOCK}),
                (BLOCK, one, {"staging_bytes": BLOCK - 1}),
                (BLOCK, one + b"x", {}),        # wrong data length
                (BLOCK, b"", {})):
            with pytest.raises(RuntimeError):
                hs.bdev_unpack_marked(target, b"\x01" + bytes(15), granule,
                                      data, **kwargs)
        with pytest.raises(RuntimeError):  # short bitmap
            hs.bdev_unpack_marked(target, b"\x01", BLOCK, one,
                                  length=9 * BLOCK)
        assert target.read(0, 128 * BLOCK) == b"\xA5" * (128 * BLOCK)


@needs_gpu
class TestDeltaDaemonHbm:
    def test_export_import(self, tmp_path):
        fixture = launch_hipstored(tmp_path, cpu=False)
        full_path = str(tmp_path / "vol.full")
        delta_path = str(tmp_path / "vol.delta")
        try:
            with hipstore.Client(fixture.socket_path) as client:
                hipstore.construct_malloc_bdev(
                    client, num_blocks=16384, block_size=4096, name="dlt")
                # perf_run draws the same offsets every run: the second
                # run below is longer, so it reaches new blocks
                perf = hipstore.perf_run(client, "dlt", workload="randwrite",
                                         io_size=4096, queue_depth=4,
                                         num_queues=1, seconds=5.0,
                                         max_ios=8)
                assert perf["io_count"] >= 1
                hipstore.bdev_clone(client, "dlt", "dlt-snap")
                info = hipstore.get_bdevs(client, "dlt-snap")[0]
                assert "hbm" in info.driver_specific
                full = hipstore.bdev_export_delta(client, "dlt", full_path)
                assert full["full"] and full["saved"] == 16384
                assert full["granule"] == 4096
                perf = hipstore.perf_run(client, "dlt", workload="randwrite",
                                         io_size=4096, queue_depth=4,
                                         num_queues=1, seconds=5.0,
                                         max_ios=32)
                assert perf["io_count"] >= 1
                cmp = hipstore.bdev_compare(client, "dlt-snap", "dlt")
                delta = hipstore.bdev_export_delta(client, "dlt", delta_path,
                                                   base="dlt-snap")
                assert not delta["full"]
                assert delta["saved"] == cmp["mismatched"]
                assert 1 <= delta["saved"] <= perf["io_count"]
                assert delta["file_bytes"] == \
                    (tmp_path / "vol.delta").stat().st_size
                # the snapshot holds the state of the full file: apply
                # the delta to a fresh volume restored from the full file
                hipstore.construct_malloc_bdev(
                    client, num_blocks=16384, block_size=4096, name="dlt-new")
                r = hipstore.bdev_import_delta(client, "dlt-new", full_path)
                assert r["applied"] == 16384
                assert hipstore.bdev_compare(
                    client, "dlt-snap", "dlt-new")["mismatched"] == 0
                r = hipstore.bdev_import_delta(client, "dlt-new", delta_path,
                                               dry_run=True)
                assert r["applied"] == delta["saved"]
                assert hipstore.bdev_compare(
                    client, "dlt-snap", "dlt-new")["mismatched"] == 0
                r = hipstore.bdev_import_delta(client, "dlt-new", delta_path)
                assert r["applied"] == delta["saved"]
                assert hipstore.bdev_compare(
                    client, "dlt", "dlt-new")["mismatched"] == 0
        finally:
            fixture.stop()
