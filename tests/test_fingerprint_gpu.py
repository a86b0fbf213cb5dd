"""hipstore::k_fingerprint_granules on HBM bdevs, and base-less
incremental checkpoints of HBM volumes through the daemon.

The yardsticks are the numpy model of the definition (test_fingerprint)
and the host path on a malloc twin with the same content. All ranges
are validated on the host before any launch."""

import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored
from test_fingerprint import model, random_bytes

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

BLOCK = 512
MAX_WGS = 2048
WAVES = 4
# More granules than waves in the grid, twice over, plus a ragged tail.
N = 2 * MAX_WGS * WAVES + 5


@pytest.fixture(scope="module")
def volume():
    """HBM bdev and malloc twin with the same content, and the model's
    fingerprints per granule size, computed once. Read-only."""
    data = bytearray(random_bytes(N * BLOCK, 20263))
    data[3 * BLOCK:4 * BLOCK] = bytes(BLOCK)
    data[4 * BLOCK:5 * BLOCK] = b"\xFF" * BLOCK
    # one granule at three indices
    for g in (MAX_WGS * WAVES + 1, N - 1):
        data[g * BLOCK:(g + 1) * BLOCK] = data[9 * BLOCK:10 * BLOCK]
    data = bytes(data)
    hbm = hs.create_hbm_bdev("fp-h", BLOCK, N, device=0)
    twin = hs.create_malloc_bdev("fp-m", BLOCK, N)
    for bdev in (hbm, twin):
        bdev.write(0, data)
    return {"hbm": hbm, "twin": twin, "data": data, "models": {}}


def expect(volume, granule, offset=0):
    key = (granule, offset)
    if key not in volume["models"]:
        n = (N * BLOCK - offset) // granule
        volume["models"][key] = model(
            volume["data"][offset:offset + n * granule], granule)
    return volume["models"][key]


@needs_gpu
class TestFingerprintKernel:
    @pytest.mark.parametrize("granule", [512, 1024, 1536, 4096, 65536])
    def test_granules(self, volume, granule):
        """32 active lanes, exactly one row, a ragged second row, four
        rows (one unrolled group), 64 groups."""
        want = expect(volume, granule)
        assert hs.bdev_fingerprint(volume["hbm"], granule) == want
        assert hs.bdev_fingerprint(volume["twin"], granule) == want

    def test_content_only(self, volume):
        fps = hs.bdev_fingerprint(volume["hbm"], BLOCK)

        def at(g):
            return fps[g * 16:(g + 1) * 16]

        assert at(9) == at(MAX_WGS * WAVES + 1) == at(N - 1)
        assert at(3) == hs.fingerprint_bytes(bytes(BLOCK), BLOCK)
        assert at(4) == hs.fingerprint_bytes(b"\xFF" * BLOCK, BLOCK)
        assert len({at(g) for g in (3, 4, 9, 10)}) == 4

    @pytest.mark.parametrize("granule", [512, 1536])
    def test_shifted_offset(self, volume, granule):
        off = 7 * BLOCK if granule == BLOCK else 7 * granule
        want = expect(volume, granule, off)
        assert hs.bdev_fingerprint(volume["hbm"], granule, offset=off) == want
        assert hs.bdev_fingerprint(volume["twin"], granule,
                                   offset=off) == want

    @pytest.mark.parametrize("staging", [32, 96, 0])
    def test_staging_windows(self, staging):
        """One granule per window, three per window, the default."""
        n = 64 * 5 + 3
        data = random_bytes(n * BLOCK, 7)
        hbm = hs.create_hbm_bdev(f"fp-w{staging}", BLOCK, n, device=0)
        twin = hs.create_malloc_bdev(f"fp-wm{staging}", BLOCK, n)
        hbm.write(0, data)
        twin.write(0, data)
        want = model(data, BLOCK)
        assert hs.bdev_fingerprint(hbm, BLOCK, staging_bytes=staging) == want
        assert hs.bdev_fingerprint(twin, BLOCK, staging_bytes=staging) == want

    def test_rejected_before_launch(self):
        n = 128
        hbm = hs.create_hbm_bdev("fp-r", BLOCK, n, device=0)
        data = random_bytes(n * BLOCK, 9)
        hbm.write(0, data)
        for granule, kwargs in (
                (768, {}),
                (0, {}),
                (BLOCK, {"offset": 100, "length": BLOCK}),
                (BLOCK, {"length": (n + 1) * BLOCK}),
                (BLOCK, {"offset": n * BLOCK, "length": BLOCK}),
                (BLOCK, {"offset": 2**64 - BLOCK}),
                (BLOCK, {"offset": 2**64 - BLOCK, "length": 2 * BLOCK}),
                (BLOCK, {"staging_bytes": 31})):
            with pytest.raises(RuntimeError):
                hs.bdev_fingerprint(hbm, granule, **kwargs)
        assert hbm.read(0, n * BLOCK) == data


@needs_gpu
class TestFingerprintDaemonHbm:
    def test_base_map_chain(self, tmp_path):
        fixture = launch_hipstored(tmp_path, cpu=False)
        full_path = str(tmp_path / "vol.full")
        delta_path = str(tmp_path / "vol.delta")
        clone_path = str(tmp_path / "vol.by-clone")
        map_path = str(tmp_path / "vol.map")
        try:
            with hipstore.Client(fixture.socket_path) as client:
                hipstore.construct_malloc_bdev(
                    client, num_blocks=16384, block_size=4096, name="fpd")
                # perf_run draws the same offsets every run: the second
                # run below is longer, so it reaches new blocks
                perf = hipstore.perf_run(client, "fpd", workload="randwrite",
                                         io_size=4096, queue_depth=4,
                                         num_queues=1, seconds=5.0,
                                         max_ios=8)
                assert perf["io_count"] >= 1
                info = hipstore.get_bdevs(client, "fpd")[0]
                assert "hbm" in info.driver_specific
                full = hipstore.bdev_export_delta(client, "fpd", full_path,
                                                  map_out=map_path)
                assert full["full"] and full["saved"] == 16384
                assert full["map_bytes"] == \
                    (tmp_path / "vol.map").stat().st_size
                hipstore.bdev_clone(client, "fpd", "fpd-snap")
                perf = hipstore.perf_run(client, "fpd", workload="randwrite",
                                         io_size=4096, queue_depth=4,
                                         num_queues=1, seconds=5.0,
                                         max_ios=32)
                assert perf["io_count"] >= 1
                cmp = hipstore.bdev_compare(client, "fpd-snap", "fpd")
                delta = hipstore.bdev_export_delta(
                    client, "fpd", delta_path, base_map=map_path,
                    map_out=map_path, overwrite=True)
                assert not delta["full"]
                assert delta["saved"] == cmp["mismatched"]
                assert 1 <= delta["saved"] <= perf["io_count"]
                hipstore.bdev_export_delta(client, "fpd", clone_path,
                                           base="fpd-snap")
                assert open(delta_path, "rb").read() == \
                    open(clone_path, "rb").read()
                hipstore.construct_malloc_bdev(
                    client, num_blocks=16384, block_size=4096, name="fpd-new")
                hipstore.bdev_import_delta(client, "fpd-new", full_path)
                r = hipstore.bdev_verify_fingerprints(client, "fpd-new",
                                                      map_path)
                assert r["mismatched"] == delta["saved"]
                hipstore.bdev_import_delta(client, "fpd-new", delta_path)
                r = hipstore.bdev_verify_fingerprints(client, "fpd-new",
                                                      map_path)
                assert (r["granules"], r["mismatched"]) == (16384, 0)
                assert hipstore.bdev_compare(
                    client, "fpd", "fpd-new")["mismatched"] == 0
        finally:
            fixture.stop()
