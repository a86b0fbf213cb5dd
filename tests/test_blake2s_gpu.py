"""hipstore::k_blake2s_granules (HSFP2) on HBM bdevs and keyed maps of
HBM volumes through the daemon, exactly equal to hashlib.blake2s
(test_blake2s.model) and to the host path on a malloc twin."""

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored
from test_blake2s import BAD_KINDS, KEY, KINDS, OTHER_KEY, model
from test_fingerprint import random_bytes

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

SMALL = 16                 # block size of the volume with small granules
SMALL_BYTES = 2 * 61440    # a multiple of every granule below
GRANULES = [16, 48, 64, 80, 128, 512, 4096]
MANY = 2 * 2048 * 4 * 16 + 21


@pytest.fixture(scope="module")
def small():
    """16-byte blocks; a stretch of zeros, one of 0xFF, and 4096 bytes of
    content at three places. Read-only."""
    data = bytearray(random_bytes(SMALL_BYTES, 20264))
    data[3 * 4096:4 * 4096] = bytes(4096)
    data[4 * 4096:5 * 4096] = b"\xFF" * 4096
    for at in (9, 17):
        data[at * 4096:(at + 1) * 4096] = data[4096:2 * 4096]
    data = bytes(data)
    hbm = hs.create_hbm_bdev("b2s-h", SMALL, len(data) // SMALL, device=0)
    twin = hs.create_malloc_bdev("b2s-m", SMALL, len(data) // SMALL)
    hbm.write(0, data)
    twin.write(0, data)
    return {"hbm": hbm, "twin": twin, "data": data}


@pytest.fixture(scope="module")
def many():
    data = random_bytes(MANY * 64, 20265)
    hbm = hs.create_hbm_bdev("b2many", 64, MANY, device=0)
    hbm.write(0, data)
    return {"hbm": hbm, "data": data}


@needs_gpu
@pytest.mark.parametrize("algorithm, key", KINDS)
class TestBlake2sKernel:
    @pytest.mark.parametrize("granule", GRANULES)
    def test_granules(self, small, granule, algorithm, key):
        """One lane of the quad live, three, one final full block, a full
        and a partial block, two full blocks, 8 blocks, 64 blocks (16
        batches of four). The whole volume, then 1, 16 and 17 granules."""
        kind = {"algorithm": algorithm, "key": key}
        want = model(small["data"], granule, key)
        got = hs.bdev_fingerprint(small["hbm"], granule, **kind)
        assert got == want
        assert hs.bdev_fingerprint(small["twin"], granule, **kind) == want
        assert hs.bdev_fingerprint(small["hbm"], granule, offset=7 * granule,
                                   **kind) == want[7 * 16:]
        if granule == 4096:  # content only: one fingerprint at three indices
            assert got[16:32] == got[9 * 16:10 * 16] == got[17 * 16:18 * 16]
        for n in (1, 16, 17):
            assert hs.bdev_fingerprint(small["hbm"], granule,
                                       length=n * granule,
                                       **kind) == want[:n * 16]

    def test_more_groups_than_the_grid(self, many, algorithm, key):
        """Twice the waves of the largest grid, and a ragged last group."""
        assert hs.bdev_fingerprint(many["hbm"], 64, algorithm=algorithm,
                                   key=key) == model(many["data"], 64, key)

    @pytest.mark.parametrize("staging", [32, 96, 0])
    def test_staging_windows(self, small, staging, algorithm, key):
        """One granule per window, three per window, the default."""
        length = 40 * 80
        want = model(small["data"][:length], 80, key)
        for bdev in (small["hbm"], small["twin"]):
            assert hs.bdev_fingerprint(bdev, 80, length=length,
                                       staging_bytes=staging,
                                       algorithm=algorithm, key=key) == want


@needs_gpu
def test_rejected_before_launch():
    block, n = 512, 128
    hbm = hs.create_hbm_bdev("b2-r", block, n, device=0)
    data = random_bytes(n * block, 9)
    hbm.write(0, data)
    for granule, kwargs in (
            (768, {}), (0, {}), (block, {"offset": 100, "length": block}),
            (block, {"length": (n + 1) * block}),
            (block, {"offset": n * block, "length": block}),
            (block, {"offset": 2**64 - block}),
            (block, {"offset": 2**64 - block, "length": 2 * block}),
            (block, {"staging_bytes": 31})):
        with pytest.raises(RuntimeError):
            hs.bdev_fingerprint(hbm, granule, algorithm=3, key=KEY, **kwargs)
    for algorithm, key in BAD_KINDS:
        with pytest.raises(RuntimeError):
            hs.bdev_fingerprint(hbm, block, algorithm=algorithm, key=key)
    assert hbm.read(0, n * block) == data


@needs_gpu
def test_keyed_chain_through_the_daemon(tmp_path):
    """Writes reach the daemon's volumes as delta files of malloc twins."""
    granule, n = 4096, 300
    states = [bytearray(random_bytes(n * granule, 41))]
    for touched in ((0, 7, 64, n - 1), (123,)):
        states.append(bytearray(states[-1]))
        for g in touched:
            states[-1][g * granule + 5] ^= 0x80
    twins = []
    for i, state in enumerate(states):
        twins.append(hs.create_malloc_bdev(f"b2d-t{i}", granule, n))
        twins[i].write(0, bytes(state))
    seed, writes, one_byte, full, delta, map_path = (
        str(tmp_path / f) for f in ("seed", "writes", "one-byte", "full",
                                    "delta", "vol.map"))
    hs.bdev_export_delta(twins[0], seed)
    hs.bdev_export_delta(twins[1], writes, base=twins[0])
    hs.bdev_export_delta(twins[2], one_byte, base=twins[1])
    key_file, wrong_file = str(tmp_path / "key"), str(tmp_path / "wrong")
    open(key_file, "wb").write(KEY)
    open(wrong_file, "wb").write(OTHER_KEY)
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            for name in ("b2d", "b2d-new"):
                hipstore.construct_malloc_bdev(client, num_blocks=n,
                                               block_size=granule, name=name)
            assert "hbm" in hipstore.get_bdevs(client, "b2d")[0].driver_specific
            hipstore.bdev_import_delta(client, "b2d", seed)
            r = hipstore.bdev_export_delta(
                client, "b2d", full, map_out=map_path,
                map_algorithm="blake2s", map_key_file=key_file)
            assert r["full"] and r["saved"] == n
            hipstore.bdev_import_delta(client, "b2d", writes)
            r = hipstore.bdev_export_delta(
                client, "b2d", delta, base_map=map_path, map_out=map_path,
                overwrite=True, map_key_file=key_file)
            assert (r["full"], r["saved"]) == (False, 4)
            assert open(delta, "rb").read() == open(writes, "rb").read()
            for path in (full, delta):
                hipstore.bdev_import_delta(client, "b2d-new", path)
            r = hipstore.bdev_verify_fingerprints(client, "b2d-new", map_path,
                                                  map_key_file=key_file)
            assert (r["granules"], r["mismatched"]) == (n, 0)
            with pytest.raises(hipstore.RpcError):
                hipstore.bdev_verify_fingerprints(client, "b2d-new", map_path,
                                                  map_key_file=wrong_file)
            hipstore.bdev_import_delta(client, "b2d-new", one_byte)
            r = hipstore.bdev_verify_fingerprints(client, "b2d-new", map_path,
                                                  map_key_file=key_file)
            assert (r["mismatched"], r["first_mismatches"]) == (1, [123])
    finally:
        fixture.stop()
