"""HSFP2 (BLAKE2s granule fingerprints) on the host: the byte model, the
generic path, version-2 maps and keyed export chains on malloc bdevs,
against hashlib.blake2s and a map layout built here from delta.h."""

import hashlib
import os
import struct

import pytest

from oim_amd import _hipstore as hs

from test_fingerprint import random_bytes

BLOCK = 512
KEY = bytes(range(100, 132))
OTHER_KEY = bytes(range(101, 133))
KINDS = [pytest.param(2, None, id="unkeyed"), pytest.param(3, KEY, id="keyed")]


def model(data, granule, key=None):
    return b"".join(
        hashlib.blake2s(data[i:i + granule], digest_size=16, key=key or b"",
                        person=b"HSFP2").digest()
        for i in range(0, len(data), granule))


def kcv(key):
    return hashlib.blake2s(b"", digest_size=16, key=key,
                           person=b"HSFP2kcv").digest()[:4]


def build_map_file(data, granule, key=None, version=2, algorithm=None):
    """The documented version-2 layout, one record (n <= 65536)."""
    fps = model(data, granule, key)
    n = len(data) // granule
    if algorithm is None:
        algorithm = 3 if key else 2
    head = b"HSFPMAP1" + struct.pack(
        "<IIIIQQ", version, BLOCK, granule, algorithm, len(data), n) + \
        (kcv(key) if key else bytes(4)) + bytes(16)
    out = [head, struct.pack("<I", hs.crc32c(head))]
    out += [struct.pack("<II", n, hs.crc32c(fps)), fps,
            b"HSFPEND1" + struct.pack("<Q", n)]
    return b"".join(out)


@pytest.mark.parametrize("algorithm, key", KINDS)
class TestHasher:
    @pytest.mark.parametrize("granule", [16, 48, 64, 80, 4096])
    def test_matches_hashlib(self, granule, algorithm, key):
        data = random_bytes(5 * granule, granule) + bytes(granule) + \
            b"\xFF" * granule
        got = hs.fingerprint_bytes(data, granule, algorithm=algorithm, key=key)
        assert got == model(data, granule, key)

    @pytest.mark.parametrize("staging", [32, 0])
    def test_bdev_windows(self, staging, algorithm, key):
        n = 64 * 2 + 3
        data = random_bytes(n * BLOCK, 12)
        bdev = hs.create_malloc_bdev(f"b2-w{staging}-{algorithm}", BLOCK, n)
        bdev.write(0, data)
        assert hs.bdev_fingerprint(bdev, BLOCK, staging_bytes=staging,
                                   algorithm=algorithm, key=key) == \
            model(data, BLOCK, key)

    def test_granule_larger_than_a_read_span(self, algorithm, key):
        """1.5 MiB granules cross the 1 MiB reads of the generic path."""
        granule = 3 << 19
        data = random_bytes(2 * granule, 8)
        bdev = hs.create_malloc_bdev(f"b2-big{algorithm}", BLOCK,
                                     len(data) // BLOCK)
        bdev.write(0, data)
        assert hs.bdev_fingerprint(bdev, granule, algorithm=algorithm,
                                   key=key) == model(data, granule, key)


BAD_KINDS = ((1, KEY), (2, KEY), (3, None), (3, KEY[:31]), (3, KEY + b"\0"),
             (0, None), (4, None))


N = 64 * 2 + 5


@pytest.fixture(scope="module")
def volume():
    data = random_bytes(N * BLOCK, 2027)
    bdev = hs.create_malloc_bdev("b2-src", BLOCK, N)
    bdev.write(0, data)
    return {"bdev": bdev, "data": data}


class TestMapFile:
    @pytest.mark.parametrize("key", [None, KEY], ids=["unkeyed", "keyed"])
    def test_round_trip_matches_documented_layout(self, volume, tmp_path, key):
        path = str(tmp_path / "v.map")
        bdev = volume["bdev"]
        r = hs.bdev_fingerprint_file(bdev, path, map_algorithm="blake2s",
                                     map_key=key)
        want = build_map_file(volume["data"], BLOCK, key)
        assert open(path, "rb").read() == want
        assert r == {"version": 2, "block_size": BLOCK, "granule": BLOCK,
                     "algorithm": 3 if key else 2, "volume_bytes": N * BLOCK,
                     "granules": N, "file_bytes": len(want),
                     "keyed": key is not None}
        assert hs.fingerprint_map_info(path) == r
        assert hs.bdev_verify_fingerprints(
            bdev, path, map_algorithm="blake2s", map_key=key)["mismatched"] == 0

    def test_refusals_leave_no_file(self, volume, tmp_path):
        bdev = volume["bdev"]
        for algorithm, key in BAD_KINDS:
            with pytest.raises(ValueError):
                hs.fingerprint_bytes(bytes(64), 64, algorithm=algorithm,
                                     key=key)
        keyed = str(tmp_path / "keyed.map")
        plain = str(tmp_path / "plain.map")
        old = str(tmp_path / "old.map")
        hs.bdev_fingerprint_file(bdev, keyed, map_algorithm="blake2s",
                                 map_key=KEY)
        hs.bdev_fingerprint_file(bdev, plain, map_algorithm="blake2s")
        hs.bdev_fingerprint_file(bdev, old)
        out = str(tmp_path / "never")
        for path, kwargs in (
                (keyed, {}), (keyed, {"map_key": OTHER_KEY}),
                (plain, {"map_key": KEY}), (plain, {"map_algorithm": "hsfp1"}),
                (old, {"map_key": KEY}), (old, {"map_algorithm": "blake2s"})):
            with pytest.raises(ValueError):
                hs.bdev_verify_fingerprints(bdev, path, **kwargs)
            with pytest.raises(ValueError):
                hs.bdev_export_delta(bdev, out, base_map=path,
                                     map_out=str(tmp_path / "never.map"),
                                     **kwargs)
        for kwargs in ({"map_key": KEY},
                       {"map_algorithm": "blake2s", "map_key": KEY[:31]},
                       {"map_algorithm": "md5"}):
            with pytest.raises(ValueError):
                hs.bdev_fingerprint_file(bdev, out, **kwargs)
        hostile = str(tmp_path / "hostile.map")
        for version, algorithm in ((1, 3), (2, 1)):
            with open(hostile, "wb") as f:
                f.write(build_map_file(volume["data"], BLOCK, KEY,
                                       version=version, algorithm=algorithm))
            with pytest.raises(ValueError):
                hs.fingerprint_map_info(hostile)
        assert sorted(os.listdir(tmp_path)) == [
            "hostile.map", "keyed.map", "old.map", "plain.map"]


def test_keyed_map_chain_equals_clone_chain(tmp_path):
    """The delta by a keyed base_map is byte for byte the one by a clone."""
    n = 64 * 3 + 9
    live = hs.create_malloc_bdev("b2-live", BLOCK, n)
    live.write(0, random_bytes(n * BLOCK, 3))
    map_path = str(tmp_path / "v.map")
    r = hs.bdev_export_delta(live, str(tmp_path / "full"), map_out=map_path,
                             map_algorithm="blake2s", map_key=KEY)
    assert r["full"] and r["map_bytes"] == os.path.getsize(map_path)
    snap = hs.create_malloc_bdev("b2-snap", BLOCK, n)
    snap.write(0, live.read(0, n * BLOCK))
    touched = [0, 5, 64, n - 1]
    for g in touched:
        live.write(g * BLOCK, bytes([g % 251]) * BLOCK)
    delta = str(tmp_path / "delta")
    r = hs.bdev_export_delta(live, delta, base_map=map_path, map_out=map_path,
                             overwrite=True, map_key=KEY)
    assert (r["full"], r["marked"]) == (False, len(touched))
    by_clone = str(tmp_path / "by-clone")
    hs.bdev_export_delta(live, by_clone, base=snap)
    assert open(delta, "rb").read() == open(by_clone, "rb").read()
    assert open(map_path, "rb").read() == \
        build_map_file(live.read(0, n * BLOCK), BLOCK, KEY)
    hs.bdev_import_delta(snap, delta)
    assert hs.bdev_verify_fingerprints(snap, map_path,
                                       map_key=KEY)["mismatched"] == 0
