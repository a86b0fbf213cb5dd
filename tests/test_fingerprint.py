"""Granule fingerprints on the host: the hasher, bdev_fingerprint on the
generic path, fingerprint map files, base-less incremental checkpoints
and their RPC, oim.v0 and oimctl surfaces (CPU: malloc bdevs and a
CPU-mode daemon).

The yardstick is the numpy model of the definition below
(native/include/hipstore/fingerprint.h), itself checked against known
answers; map files are also built here from the documented layout."""

import os
import random
import struct

import grpc
import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore, spec
from oim_amd.cmd import oimctl

from fixtures import hipstored  # noqa: F401
from test_delta import (  # noqa: F401
    METADATA, build_delta_file, indexed_bytes, provision, serve_volume, stack)

BLOCK = 512

_P1 = np.uint64(0x9E3779B185EBCA87)
_P2 = np.uint64(0xC2B2AE3D27D4EB4F)
_P3 = np.uint64(0x165667B19E3779F9)


def _rotl(v, r):
    return (v << np.uint64(r)) | (v >> np.uint64(64 - r))


def _round(acc, q):
    return _rotl(acc + q * _P2, 31) * _P1


def _mix(h):
    h = h ^ (h >> np.uint64(33))
    h = h * _P2
    h = h ^ (h >> np.uint64(29))
    h = h * _P3
    return h ^ (h >> np.uint64(32))


def model(data, granule):
    """HSFP1 of every granule of `data`: all granules at once, stream s
    is column s, one row of 64 vectors per step."""
    assert granule % 16 == 0 and len(data) % granule == 0
    n = len(data) // granule
    n16 = granule // 16
    q = np.frombuffer(data, dtype="<u8").reshape(n, n16, 2)
    seeds = np.arange(1, 65, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = np.tile(_P1 * seeds, (n, 1))
        b = np.tile(_P2 * seeds, (n, 1))
        for row in range(0, n16, 64):
            w = min(64, n16 - row)
            a[:, :w] = _round(a[:, :w], q[:, row:row + w, 0])
            b[:, :w] = _round(b[:, :w], q[:, row:row + w, 1])
        d0 = _mix(a ^ _mix(b))
        d1 = _mix(b + _mix(a))
        out = np.stack([d0.sum(axis=1, dtype=np.uint64),
                        d1.sum(axis=1, dtype=np.uint64)], axis=1)
    return out.astype("<u8").tobytes()


def random_bytes(n, seed):
    return np.random.default_rng(seed).integers(
        0, 256, n, dtype=np.uint8).tobytes()


KNOWN = {
    16: ("00c519eb36c3428b97192e3b7b542f0b",
         "09eae38b6605564a138ca3cde17c090f"),
    512: ("1b2cfc71e7e87e172ec9db42b27e6dfd",
          "5eee1862c9499f66d816ffc3de4a3246"),
    1536: ("2d3bea27aefcc973f6e22a527de92335",
           "8cf6ec658ee8b4551d329908c968ae7e"),
    4096: ("c2b912c327c89cdd6c3fdeb886e56cdf",
           "d622a19b56e094d7c38414a6a9c2c8c1"),
}


class TestHasher:
    @pytest.mark.parametrize("granule", sorted(KNOWN))
    def test_known_answers(self, granule):
        zero, ramp = KNOWN[granule]
        ramp_data = bytes((7 * i + 3) & 255 for i in range(granule))
        assert model(bytes(granule), granule).hex() == zero
        assert model(ramp_data, granule).hex() == ramp
        assert hs.fingerprint_bytes(bytes(granule), granule).hex() == zero
        assert hs.fingerprint_bytes(ramp_data, granule).hex() == ramp

    @pytest.mark.parametrize("granule",
                             [16, 48, 512, 1008, 1024, 1536, 4096, 65552])
    def test_random_data_matches_model(self, granule):
        data = random_bytes(9 * granule, granule)
        got = hs.fingerprint_bytes(data, granule)
        assert len(got) == 9 * 16
        assert got == model(data, granule)

    @pytest.mark.parametrize("granule", [512, 4096])
    def test_single_bit_flips_are_distinct(self, granule):
        base = np.frombuffer(random_bytes(granule, 77), dtype=np.uint8)
        bits = granule * 8
        flipped = np.tile(base, (bits, 1))
        k = np.arange(bits)
        flipped[k, k // 8] ^= (1 << (k % 8)).astype(np.uint8)
        data = flipped.tobytes()
        got = hs.fingerprint_bytes(data, granule)
        assert got == model(data, granule)
        prints = {got[i * 16:(i + 1) * 16] for i in range(bits)}
        assert len(prints) == bits
        assert hs.fingerprint_bytes(base.tobytes(), granule) not in prints

    def test_equal_granules_equal_fingerprints(self):
        g = random_bytes(1536, 5)
        other = random_bytes(1536, 6)
        got = hs.fingerprint_bytes(g + other + g + other + other + g, 1536)
        fps = [got[i * 16:(i + 1) * 16] for i in range(6)]
        assert fps[0] == fps[2] == fps[5]
        assert fps[1] == fps[3] == fps[4] != fps[0]

    def test_bad_arguments(self):
        for data, granule in ((bytes(32), 0), (bytes(24), 24),
                              (bytes(48), 32)):
            with pytest.raises(ValueError):
                hs.fingerprint_bytes(data, granule)
        assert hs.fingerprint_bytes(b"", 16) == b""


N = 64 * 5 + 3  # 512 B blocks


@pytest.fixture(scope="module")
def volume():
    data = random_bytes(N * BLOCK, 2026)
    bdev = hs.create_malloc_bdev("fp-src", BLOCK, N)
    bdev.write(0, data)
    return {"bdev": bdev, "data": data}


class TestBdevFingerprint:
    @pytest.mark.parametrize("staging", [32, 96, 0])
    def test_staging_windows(self, volume, staging):
        assert hs.bdev_fingerprint(volume["bdev"], BLOCK,
                                   staging_bytes=staging) == \
            model(volume["data"], BLOCK)

    @pytest.mark.parametrize("granule", [1024, 1536, 3584])
    def test_shifted_offset_and_granules(self, volume, granule):
        off = granule
        n = (N * BLOCK - off) // granule
        want = model(volume["data"][off:off + n * granule], granule)
        assert hs.bdev_fingerprint(volume["bdev"], granule, offset=off) == want
        assert hs.bdev_fingerprint(volume["bdev"], granule, offset=off,
                                   length=2 * granule,
                                   staging_bytes=32) == want[:32]

    def test_granule_larger_than_a_read_span(self):
        """1.5 MiB granules: the hasher carries a granule across the
        1 MiB reads of the generic path."""
        granule = 3 << 19
        data = random_bytes(3 * granule, 8)
        bdev = hs.create_malloc_bdev("fp-big", BLOCK, len(data) // BLOCK)
        bdev.write(0, data)
        assert hs.bdev_fingerprint(bdev, granule) == model(data, granule)
        assert hs.bdev_fingerprint(bdev, granule, offset=granule,
                                   staging_bytes=32) == \
            model(data[granule:], granule)

    def test_rejections(self, volume):
        bdev = volume["bdev"]
        for granule, kwargs in (
                (768, {}),
                (0, {}),
                (BLOCK, {"offset": 100, "length": BLOCK}),
                (BLOCK, {"length": (N + 1) * BLOCK}),
                (BLOCK, {"offset": N * BLOCK, "length": BLOCK}),
                (BLOCK, {"offset": 2**64 - BLOCK}),
                (BLOCK, {"offset": 2**64 - BLOCK, "length": 2 * BLOCK}),
                (BLOCK, {"staging_bytes": 31})):
            with pytest.raises(RuntimeError):
                hs.bdev_fingerprint(bdev, granule, **kwargs)
        assert bdev.read(0, N * BLOCK) == volume["data"]


# --- map files -------------------------------------------------------------

MAP_HEADER = 64
MAP_TRAILER = 16


def build_map_file(data, granule, block_size=BLOCK):
    """The documented version-1 layout."""
    fps = model(data, granule)
    n = len(data) // granule
    head = b"HSFPMAP1" + struct.pack("<IIIIQQ", 1, block_size, granule, 1,
                                     len(data), n) + bytes(20)
    assert len(head) == 60
    out = [head, struct.pack("<I", hs.crc32c(head))]
    for first in range(0, n, 65536):
        payload = fps[first * 16:(first + 65536) * 16]
        out.append(struct.pack("<II", len(payload) // 16, hs.crc32c(payload)))
        out.append(payload)
    out.append(b"HSFPEND1" + struct.pack("<Q", n))
    return b"".join(out)


def refresh_header_crc(blob):
    blob = bytearray(blob)
    blob[60:64] = struct.pack("<I", hs.crc32c(bytes(blob[:60])))
    return bytes(blob)


class TestMapFile:
    def test_round_trip_matches_documented_layout(self, volume, tmp_path):
        path = str(tmp_path / "v.map")
        r = hs.bdev_fingerprint_file(volume["bdev"], path)
        want = build_map_file(volume["data"], BLOCK)
        assert open(path, "rb").read() == want
        assert r == {"version": 1, "block_size": BLOCK, "granule": BLOCK,
                     "algorithm": 1, "volume_bytes": N * BLOCK, "granules": N,
                     "file_bytes": len(want)}
        assert hs.fingerprint_map_info(path) == r
        assert hs.bdev_verify_fingerprints(volume["bdev"], path) == {
            "granule": BLOCK, "granules": N, "mismatched": 0,
            "first_mismatches": []}
        with pytest.raises(RuntimeError, match="exists"):
            hs.bdev_fingerprint_file(volume["bdev"], path, granule=17 * BLOCK)
        assert open(path, "rb").read() == want
        r = hs.bdev_fingerprint_file(volume["bdev"], path, granule=17 * BLOCK,
                                     overwrite=True)
        assert r["granules"] == N // 17
        assert open(path, "rb").read() == \
            build_map_file(volume["data"], 17 * BLOCK)
        with pytest.raises(ValueError):
            hs.bdev_fingerprint_file(volume["bdev"], str(tmp_path / "bad"),
                                     granule=768)
        with pytest.raises(RuntimeError):
            hs.bdev_fingerprint_file(volume["bdev"],
                                     str(tmp_path / "no-dir" / "m"))
        assert sorted(os.listdir(tmp_path)) == ["v.map"]

    def test_several_records(self, tmp_path):
        """65536 + 5 granules: a full record and a short one."""
        n = 65536 + 5
        data = random_bytes(n * BLOCK, 4)
        bdev = hs.create_malloc_bdev("fp-rec", BLOCK, n)
        bdev.write(0, data)
        path = str(tmp_path / "rec.map")
        r = hs.bdev_fingerprint_file(bdev, path)
        want = build_map_file(data, BLOCK)
        assert r["file_bytes"] == MAP_HEADER + 2 * 8 + n * 16 + MAP_TRAILER
        assert open(path, "rb").read() == want
        bdev.write(65537 * BLOCK, bytes(BLOCK))
        r = hs.bdev_verify_fingerprints(bdev, path)
        assert (r["mismatched"], r["first_mismatches"]) == (1, [65537])

    def test_hostile_maps_are_refused(self, volume, tmp_path):
        valid = build_map_file(volume["data"], BLOCK)

        def flip(at):
            blob = bytearray(valid)
            blob[at] ^= 0x40
            return bytes(blob)

        def header_field(offset, fmt, value):
            blob = bytearray(valid)
            blob[offset:offset + struct.calcsize(fmt)] = \
                struct.pack(fmt, value)
            return refresh_header_crc(blob)

        variants = [
            ("header byte", flip(30)),
            ("header crc", flip(61)),
            ("record payload", flip(MAP_HEADER + 8 + 5 * 16 + 3)),
            ("record crc", flip(MAP_HEADER + 5)),
            ("record count", flip(MAP_HEADER)),
            ("truncated", valid[:-1]),
            ("truncated in a record", valid[:MAP_HEADER + 100]),
            ("truncated header", valid[:40]),
            ("empty", b""),
            ("one extra byte", valid + b"\0"),
            ("magic", b"HSFPMAP2" + valid[8:]),
            ("end magic", flip(len(valid) - 12)),
            ("trailer count", flip(len(valid) - 8)),
            ("version 2", header_field(8, "<I", 2)),
            ("algorithm 2", header_field(20, "<I", 2)),
            ("reserved u64", header_field(40, "<Q", 1)),
            ("reserved u32", header_field(52, "<I", 1)),
            ("reserved last", header_field(56, "<I", 1 << 31)),
            ("granule 24", header_field(16, "<I", 24)),
            ("n_granules + 1", header_field(32, "<Q", N + 1)),
            ("volume_bytes", header_field(24, "<Q", N * BLOCK + 16)),
        ]
        path = str(tmp_path / "hostile.map")
        out = str(tmp_path / "never.delta")
        for name, blob in variants:
            with open(path, "wb") as f:
                f.write(blob)
            with pytest.raises(ValueError):
                hs.fingerprint_map_info(path)
            with pytest.raises(ValueError):
                hs.bdev_verify_fingerprints(volume["bdev"], path)
            with pytest.raises(ValueError):
                hs.bdev_export_delta(volume["bdev"], out, base_map=path)
            assert sorted(os.listdir(tmp_path)) == ["hostile.map"], name
        # a sound map that does not fit the volume
        small = hs.create_malloc_bdev("fp-small", BLOCK, N - 1)
        coarse = hs.create_malloc_bdev("fp-4k", 4096, N)
        with open(path, "wb") as f:
            f.write(valid)
        for bdev in (small, coarse):
            with pytest.raises(ValueError):
                hs.bdev_verify_fingerprints(bdev, path)
            with pytest.raises(ValueError):
                hs.bdev_export_delta(bdev, out, base_map=path)
        with pytest.raises(RuntimeError):
            hs.fingerprint_map_info(str(tmp_path / "missing"))
        assert sorted(os.listdir(tmp_path)) == ["hostile.map"]


# --- base-less incremental checkpoints -----------------------------------------

class TestChain:
    def test_map_chain_equals_clone_chain(self, tmp_path):
        """full + map_out; write; delta with base_map / map_out; again.
        Every delta is byte for byte the delta against a clone of the
        base state, and the chain restores the volume."""
        rng = random.Random(31)
        n = 64 * 5 + 9
        live = hs.create_malloc_bdev("fc-live", BLOCK, n)
        live.write(0, indexed_bytes(n))
        map_path = str(tmp_path / "v.map")
        paths = [str(tmp_path / f"c{i}") for i in range(3)]
        r = hs.bdev_export_delta(live, paths[0], map_out=map_path)
        assert r["full"] and r["marked"] == n
        assert r["map_bytes"] == os.path.getsize(map_path)
        assert open(paths[0], "rb").read() == \
            build_delta_file(indexed_bytes(n), BLOCK)
        assert open(map_path, "rb").read() == \
            build_map_file(indexed_bytes(n), BLOCK)
        for i in (1, 2):
            snap = hs.create_malloc_bdev(f"fc-snap{i}", BLOCK, n)
            snap.write(0, live.read(0, n * BLOCK))
            touched = sorted(set(rng.sample(range(n), 9)) | {0, n - 1})
            for g in touched:
                live.write(g * BLOCK, bytes([i * 16 + g % 13]) * BLOCK)
            r = hs.bdev_export_delta(live, paths[i], base_map=map_path,
                                     map_out=map_path, overwrite=True)
            assert not r["full"]
            assert (r["granule"], r["marked"]) == (BLOCK, len(touched))
            assert r["map_bytes"] == os.path.getsize(map_path)
            by_clone = str(tmp_path / f"clone{i}")
            hs.bdev_export_delta(live, by_clone, base=snap)
            assert open(paths[i], "rb").read() == \
                open(by_clone, "rb").read()
            assert open(map_path, "rb").read() == \
                build_map_file(live.read(0, n * BLOCK), BLOCK)
        fresh = hs.create_malloc_bdev("fc-fresh", BLOCK, n)
        for path in paths:
            hs.bdev_import_delta(fresh, path)
        assert fresh.read(0, n * BLOCK) == live.read(0, n * BLOCK)
        r = hs.bdev_verify_fingerprints(fresh, map_path)
        assert (r["granules"], r["mismatched"]) == (n, 0)
        fresh.write(77 * BLOCK, b"\xEE" * BLOCK)
        r = hs.bdev_verify_fingerprints(fresh, map_path)
        assert (r["mismatched"], r["first_mismatches"]) == (1, [77])
        assert hs.bdev_verify_fingerprints(
            fresh, map_path, max_report=0)["first_mismatches"] == []
        assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]

    def test_unchanged_volume_gives_empty_delta(self, volume, tmp_path):
        map_path = str(tmp_path / "m")
        hs.bdev_fingerprint_file(volume["bdev"], map_path)
        r = hs.bdev_export_delta(volume["bdev"], str(tmp_path / "d"),
                                 base_map=map_path)
        assert r["marked"] == 0 and not r["full"] and "map_bytes" not in r
        assert open(tmp_path / "d", "rb").read() == \
            build_delta_file(volume["data"], BLOCK, [])

    def test_coarse_granule_comes_from_the_map(self, tmp_path):
        n = 64 * 8
        data = indexed_bytes(n)
        live = hs.create_malloc_bdev("fc-4k", BLOCK, n)
        live.write(0, data)
        map_path = str(tmp_path / "m")
        hs.bdev_export_delta(live, str(tmp_path / "full"), granule=4096,
                             map_out=map_path)
        live.write(9 * BLOCK, b"\x11" * BLOCK)
        live.write(n * BLOCK - BLOCK, b"\x22" * BLOCK)
        for granule in (None, 4096):
            r = hs.bdev_export_delta(live, str(tmp_path / "d"),
                                     base_map=map_path, granule=granule,
                                     overwrite=True)
            assert (r["granule"], r["marked"]) == (4096, 2)
        want = build_delta_file(live.read(0, n * BLOCK), 4096, [1, n // 8 - 1])
        assert open(tmp_path / "d", "rb").read() == want
        with pytest.raises(ValueError):
            hs.bdev_export_delta(live, str(tmp_path / "x"), base_map=map_path,
                                 granule=BLOCK)

    def test_grown_volume_marks_every_new_granule(self, tmp_path):
        n = 100
        live = hs.create_malloc_bdev("fc-grow", BLOCK, n)
        live.write(0, indexed_bytes(n))
        map_path = str(tmp_path / "m")
        hs.bdev_export_delta(live, str(tmp_path / "full"), map_out=map_path)
        live.resize(n + 37)
        live.write(5 * BLOCK, b"\x55" * BLOCK)
        r = hs.bdev_export_delta(live, str(tmp_path / "d"), base_map=map_path,
                                 map_out=map_path, overwrite=True)
        assert (r["granules"], r["marked"]) == (n + 37, 38)
        want = build_delta_file(live.read(0, (n + 37) * BLOCK), BLOCK,
                                [5] + list(range(n, n + 37)))
        assert open(tmp_path / "d", "rb").read() == want
        assert hs.fingerprint_map_info(map_path)["granules"] == n + 37
        # the old, shorter map still verifies the range it covers
        hs.bdev_fingerprint_file(live, map_path, overwrite=True)
        assert hs.bdev_verify_fingerprints(live, map_path)["mismatched"] == 0

    def test_export_refusals(self, volume, tmp_path):
        bdev = volume["bdev"]
        map_path = str(tmp_path / "m")
        hs.bdev_fingerprint_file(bdev, map_path)
        before = open(map_path, "rb").read()
        out = str(tmp_path / "d")
        with pytest.raises(ValueError):  # both bases
            hs.bdev_export_delta(bdev, out, base=bdev, base_map=map_path)
        with pytest.raises(ValueError):  # the map would replace the delta
            hs.bdev_export_delta(bdev, out, map_out=out)
        with pytest.raises(RuntimeError, match="exists"):
            hs.bdev_export_delta(bdev, out, base_map=map_path,
                                 map_out=map_path)
        with pytest.raises(RuntimeError):
            hs.bdev_export_delta(bdev, out, base_map=str(tmp_path / "nope"))
        with pytest.raises(RuntimeError):
            hs.bdev_export_delta(bdev, out,
                                 map_out=str(tmp_path / "no-dir" / "m"))
        assert open(map_path, "rb").read() == before
        assert sorted(os.listdir(tmp_path)) == ["m"]


class TestPublishAndCleanup:
    """What is left behind when a file cannot take its final name."""

    def test_delta_path_is_a_directory(self, volume, tmp_path):
        os.mkdir(tmp_path / "dir")
        with pytest.raises(RuntimeError):
            hs.bdev_export_delta(volume["bdev"], str(tmp_path / "dir"),
                                 overwrite=True, map_out=str(tmp_path / "m"))
        assert os.listdir(tmp_path) == ["dir"]
        assert os.listdir(tmp_path / "dir") == []

    def test_map_path_is_a_directory(self, volume, tmp_path):
        os.mkdir(tmp_path / "mapdir")
        with pytest.raises(RuntimeError, match="was written"):
            hs.bdev_export_delta(volume["bdev"], str(tmp_path / "d"),
                                 overwrite=True,
                                 map_out=str(tmp_path / "mapdir"))
        assert open(tmp_path / "d", "rb").read() == \
            build_delta_file(volume["data"], BLOCK)
        assert sorted(os.listdir(tmp_path)) == ["d", "mapdir"]
        assert os.listdir(tmp_path / "mapdir") == []

    def test_fingerprint_file_to_a_directory(self, volume, tmp_path):
        os.mkdir(tmp_path / "mapdir")
        with pytest.raises(RuntimeError):
            hs.bdev_fingerprint_file(volume["bdev"], str(tmp_path / "mapdir"),
                                     overwrite=True)
        assert os.listdir(tmp_path) == ["mapdir"]
        assert os.listdir(tmp_path / "mapdir") == []

    def test_info_calls_on_a_directory(self, tmp_path):
        with pytest.raises(ValueError):
            hs.delta_file_info(str(tmp_path))
        with pytest.raises(ValueError):
            hs.fingerprint_map_info(str(tmp_path))

    def test_same_path_for_base_map_and_map_out(self, tmp_path):
        data = bytearray(random_bytes(N * BLOCK, 12))
        bdev = hs.create_malloc_bdev("fp-same", BLOCK, N)
        bdev.write(0, bytes(data))
        m = str(tmp_path / "m")
        hs.bdev_fingerprint_file(bdev, m)
        data[70 * BLOCK:71 * BLOCK] = b"\x3C" * BLOCK
        bdev.write(70 * BLOCK, b"\x3C" * BLOCK)
        r = hs.bdev_export_delta(bdev, str(tmp_path / "d"), base_map=m,
                                 map_out=m, overwrite=True)
        assert r["marked"] == 1
        assert open(m, "rb").read() == build_map_file(bytes(data), BLOCK)
        assert hs.bdev_verify_fingerprints(bdev, m)["mismatched"] == 0
        assert sorted(os.listdir(tmp_path)) == ["d", "m"]


# --- the daemon, oim.v0 and oimctl ---------------------------------------------

class TestDaemon:
    def test_fingerprint_verify_and_base_map(self, hipstored, tmp_path):  # noqa: F811
        n = 64 * 5 + 9
        data = indexed_bytes(n)
        with hipstore.Client(hipstored.socket_path) as client:
            methods = client.invoke("get_rpc_methods")
            assert "bdev_fingerprint" in methods
            assert "bdev_verify_fingerprints" in methods
            serve_volume(client, "fd", data, tmp_path)
            map_path = str(tmp_path / "fd.map")
            r = hipstore.bdev_fingerprint(client, "fd", map_path)
            want = build_map_file(data, BLOCK)
            assert r == {"granule": BLOCK, "granules": n,
                         "map_bytes": len(want)}
            assert open(map_path, "rb").read() == want
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_fingerprint(client, "fd", map_path)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert hipstore.bdev_verify_fingerprints(client, "fd", map_path) \
                == {"granule": BLOCK, "granules": n, "mismatched": 0,
                    "first_mismatches": []}
            # change three granules by importing a delta built here
            hipstore.bdev_clone(client, "fd", "fd-snap")
            live = bytearray(data)
            planted = [0, 64, n - 1]
            for g in planted:
                live[g * BLOCK:(g + 1) * BLOCK] = bytes([g % 251 + 1]) * BLOCK
            edit = str(tmp_path / "edit")
            with open(edit, "wb") as f:
                f.write(build_delta_file(bytes(live), BLOCK, planted))
            hipstore.bdev_import_delta(client, "fd", edit)
            r = hipstore.bdev_verify_fingerprints(client, "fd", map_path,
                                                  max_report=2)
            assert (r["mismatched"], r["first_mismatches"]) == (3, [0, 64])
            d1 = str(tmp_path / "fd.d1")
            r = hipstore.bdev_export_delta(client, "fd", d1,
                                           base_map=map_path,
                                           map_out=map_path, overwrite=True)
            assert r == {"granule": BLOCK, "granules": n, "saved": 3,
                         "file_bytes": os.path.getsize(d1), "full": False,
                         "map_bytes": len(want)}
            assert open(d1, "rb").read() == open(edit, "rb").read()
            by_clone = str(tmp_path / "fd.clone")
            hipstore.bdev_export_delta(client, "fd", by_clone, base="fd-snap")
            assert open(by_clone, "rb").read() == open(d1, "rb").read()
            assert open(map_path, "rb").read() == \
                build_map_file(bytes(live), BLOCK)
            out = str(tmp_path / "never")
            with open(tmp_path / "junk", "wb") as f:
                f.write(b"HSFPMAP1" + bytes(100))
            for method, params in (
                    ("bdev_export_delta", {"name": "fd", "path": out,
                                           "base": "fd-snap",
                                           "base_map": map_path}),
                    ("bdev_export_delta", {"name": "fd", "path": out,
                                           "base_map": map_path,
                                           "granule": 1024}),
                    ("bdev_export_delta", {"name": "fd", "path": out,
                                           "base_map": ""}),
                    ("bdev_export_delta", {"name": "fd", "path": out,
                                           "base_map": str(tmp_path / "junk")}),
                    ("bdev_fingerprint", {"name": "fd"}),
                    ("bdev_fingerprint", {"name": "nope", "path": out}),
                    ("bdev_fingerprint", {"name": "fd", "path": out,
                                          "granule": 768}),
                    ("bdev_verify_fingerprints", {"name": "fd"}),
                    ("bdev_verify_fingerprints", {"name": "nope",
                                                  "path": map_path}),
                    ("bdev_verify_fingerprints", {"name": "fd",
                                                  "path": str(tmp_path / "junk")})):
                with pytest.raises(hipstore.RpcError) as err:
                    client.invoke(method, params)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS, params
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_verify_fingerprints(client, "fd", out)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert not os.path.exists(out)
            # a claimed volume may be fingerprinted and verified
            hipstore.construct_vhost_scsi_controller(client, "fd-ctrl")
            hipstore.add_vhost_scsi_lun(client, "fd-ctrl", 0, "fd")
            assert hipstore.bdev_verify_fingerprints(
                client, "fd", map_path)["mismatched"] == 0
            hipstore.bdev_fingerprint(client, "fd", map_path, overwrite=True)
            hipstore.remove_vhost_controller(client, "fd-ctrl")


class TestOimV0:
    def test_checkpoint_with_maps_and_verify(self, stack, tmp_path):
        n = 64 * 5 + 9
        base = indexed_bytes(n)
        live = bytearray(base)
        planted = [0, 63, 200]
        for g in planted:
            live[g * BLOCK:(g + 1) * BLOCK] = bytes([g % 251 + 1]) * BLOCK
        for name, blob in (("seed", build_delta_file(base, BLOCK)),
                           ("edit", build_delta_file(bytes(live), BLOCK,
                                                     planted))):
            with open(tmp_path / name, "wb") as f:
                f.write(blob)

        def checkpoint(**kwargs):
            return stack.CheckpointMallocBDev(
                spec.CheckpointMallocBDevRequest(**kwargs),
                metadata=METADATA, timeout=30)

        def restore(name, path):
            return stack.RestoreMallocBDev(
                spec.RestoreMallocBDevRequest(bdev_name=name,
                                              path=str(tmp_path / path)),
                metadata=METADATA, timeout=30)

        def verify(**kwargs):
            return stack.VerifyMallocBDev(
                spec.VerifyMallocBDevRequest(**kwargs),
                metadata=METADATA, timeout=30)

        map_path = str(tmp_path / "fv.map")
        provision(stack, "fv", n * BLOCK)
        restore("fv", "seed")
        full = checkpoint(bdev_name="fv", path=str(tmp_path / "fv.full"),
                          map_out=map_path)
        assert (full.granules, full.saved) == (n, n)
        assert open(map_path, "rb").read() == build_map_file(base, BLOCK)
        reply = verify(bdev_name="fv", path=map_path)
        assert (reply.granules, reply.mismatched) == (n, 0)
        restore("fv", "edit")
        reply = verify(bdev_name="fv", path=map_path)
        assert (reply.granules, reply.mismatched) == (n, len(planted))
        delta = checkpoint(bdev_name="fv", path=str(tmp_path / "fv.d1"),
                           base_map=map_path, map_out=map_path,
                           overwrite=True)
        assert (delta.granules, delta.saved) == (n, len(planted))
        assert open(tmp_path / "fv.d1", "rb").read() == \
            open(tmp_path / "edit", "rb").read()
        provision(stack, "fv-new", n * BLOCK)
        restore("fv-new", "fv.full")
        restore("fv-new", "fv.d1")
        assert verify(bdev_name="fv-new", path=map_path).mismatched == 0
        cases = (
            (checkpoint, {"bdev_name": "fv", "base_name": "fv-new",
                          "base_map": map_path,
                          "path": str(tmp_path / "x")},
             grpc.StatusCode.INVALID_ARGUMENT),
            (checkpoint, {"bdev_name": "fv", "base_map": map_path,
                          "map_out": map_path, "path": str(tmp_path / "x")},
             grpc.StatusCode.ALREADY_EXISTS),
            (checkpoint, {"bdev_name": "fv",
                          "base_map": str(tmp_path / "seed"),
                          "path": str(tmp_path / "x")},
             grpc.StatusCode.INVALID_ARGUMENT),
            (verify, {"bdev_name": "nope", "path": map_path},
             grpc.StatusCode.NOT_FOUND),
            (verify, {"bdev_name": "fv"}, grpc.StatusCode.INVALID_ARGUMENT),
            (verify, {"bdev_name": "fv", "path": str(tmp_path / "seed")},
             grpc.StatusCode.INVALID_ARGUMENT),
        )
        for call, kwargs, code in cases:
            with pytest.raises(grpc.RpcError) as err:
                call(**kwargs)
            assert err.value.code() == code, kwargs
        assert not os.path.exists(tmp_path / "x")

    def test_oimctl_verbs(self, stack, tmp_path, capsys):
        provision(stack, "ov")
        granules = (1 << 20) // BLOCK
        base = ["--registry", stack.endpoint]
        full = str(tmp_path / "ov.full")
        map_path = str(tmp_path / "ov.map")
        assert oimctl.main(base + ["checkpoint", "--controller", "c0", "ov",
                                   full, "--map-out", map_path]) == 0
        assert f"{granules} of {granules} granules" in capsys.readouterr().out
        assert oimctl.main(base + ["verify", "--controller", "c0", "ov",
                                   map_path]) == 0
        assert f"0 of {granules} granules differ" in capsys.readouterr().out
        assert oimctl.main(base + ["checkpoint", "--controller", "c0", "ov",
                                   str(tmp_path / "ov.d1"), "--base-map",
                                   map_path, "--map-out", map_path,
                                   "--overwrite"]) == 0
        assert f"0 of {granules} granules" in capsys.readouterr().out
