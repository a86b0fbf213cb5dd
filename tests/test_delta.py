"""Marked pack / unpack on the generic path, hipstore delta files and
their RPC, oim.v0 and oimctl surfaces (CPU: malloc bdevs and a CPU-mode
daemon).

The yardsticks are a Python byte model (every 512 B block carries its
own index) and a delta file built here from the documented layout with
hs.crc32c."""

import os
import random
import struct

import grpc
import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore, spec
from oim_amd.cmd import oimctl
from oim_amd.common.server import grpc_target
from oim_amd.controller import Controller, ControllerServer
from oim_amd.registry import MemRegistryDB, Registry, RegistryServer

from fixtures import hipstored  # noqa: F401

BLOCK = 512
HEADER = 64
TRAILER = 16


def indexed_bytes(n_blocks, salt=0):
    """Block i is the u32 (i + salt) repeated: every granule distinct."""
    return np.repeat(np.arange(salt, salt + n_blocks, dtype=np.uint32),
                     BLOCK // 4).tobytes()


def model_bitmap(n_granules, marked, stray=(), pad_to_words=False):
    size = (n_granules + 63) // 64 * 8 if pad_to_words \
        else (n_granules + 7) // 8
    out = bytearray(size)
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


def build_delta_file(data, granule, marked=None, block_size=BLOCK):
    """The documented version-1 layout; marked=None is a full file."""
    n = len(data) // granule
    assert n * granule == len(data)
    full = marked is None
    marked = list(range(n)) if full else sorted(marked)
    bitmap = model_bitmap(n, marked, pad_to_words=True)
    head = b"HSDELTA1" + struct.pack(
        "<IIIIQQQIII", 1, block_size, granule, 1 if full else 0, len(data),
        n, len(marked), hs.crc32c(bitmap), 0, 0)
    assert len(head) == 60
    out = [head, struct.pack("<I", hs.crc32c(head)), bitmap]
    per_record = max(1, (1 << 20) // granule)
    for i in range(0, len(marked), per_record):
        payload = model_pack(data, granule, marked[i:i + per_record])
        out.append(struct.pack("<II", len(payload) // granule,
                               hs.crc32c(payload)))
        out.append(payload)
    out.append(b"HSDEND1\0" + struct.pack("<Q", len(marked)))
    return b"".join(out)


def refresh_header_crc(blob):
    """A header edited on purpose, with its CRC made right again."""
    blob = bytearray(blob)
    blob[60:64] = struct.pack("<I", hs.crc32c(bytes(blob[:60])))
    return bytes(blob)


N = 64 * 5 + 9  # 512 B blocks; a ragged last bitmap word


@pytest.fixture(scope="module")
def volume():
    data = indexed_bytes(N)
    bdev = hs.create_malloc_bdev("dl-src", BLOCK, N)
    bdev.write(0, data)
    return {"bdev": bdev, "data": data}


class TestPackUnpackModel:
    @pytest.mark.parametrize("granule", [512, 1024, 1536, 4096])
    def test_granules(self, volume, granule):
        n = N * BLOCK // granule
        rng = random.Random(granule)
        marked = sorted({0, n - 1, min(63, n - 1), min(64, n - 1)}
                        | set(rng.sample(range(n), n // 5)))
        bitmap = model_bitmap(n, marked)
        want = model_pack(volume["data"], granule, marked)
        results = [hs.bdev_pack_marked(volume["bdev"], bitmap, granule,
                                       length=n * granule,
                                       staging_bytes=staging)
                   for staging in (3 * granule, 64 * granule, 0)]
        assert results == [want] * 3
        target = hs.create_malloc_bdev(f"dl-t{granule}", BLOCK, N)
        target.fill(0, 0xA5, N * BLOCK)
        assert hs.bdev_unpack_marked(target, bitmap, granule, want,
                                     length=n * granule,
                                     staging_bytes=3 * granule) == len(marked)
        assert target.read(0, N * BLOCK) == model_unpack(
            b"\xA5" * (N * BLOCK), granule, marked, want)

    def test_offset(self, volume):
        off = 7 * BLOCK
        n = N - 7
        marked = [0, 1, 56, 57, 200, n - 1]
        bitmap = model_bitmap(n, marked)
        want = model_pack(volume["data"], BLOCK, marked, offset=off)
        assert hs.bdev_pack_marked(volume["bdev"], bitmap, BLOCK,
                                   src_offset=off) == want
        target = hs.create_malloc_bdev("dl-off", BLOCK, N)
        target.fill(0, 0xA5, N * BLOCK)
        assert hs.bdev_unpack_marked(target, bitmap, BLOCK, want,
                                     dst_offset=off) == len(marked)
        assert target.read(0, N * BLOCK) == model_unpack(
            b"\xA5" * (N * BLOCK), BLOCK, marked, want, offset=off)

    def test_empty_all_and_stray_bits(self, volume):
        bdev, data = volume["bdev"], volume["data"]
        target = hs.create_malloc_bdev("dl-e", BLOCK, N)
        target.fill(0, 0xA5, N * BLOCK)
        empty = bytes((N + 7) // 8)
        assert hs.bdev_pack_marked(bdev, empty, BLOCK) == b""
        assert hs.bdev_unpack_marked(target, empty, BLOCK, b"") == 0
        everything = model_bitmap(N, range(N))
        for staging in (3 * BLOCK, 64 * BLOCK, 0):
            assert hs.bdev_pack_marked(bdev, everything, BLOCK,
                                       staging_bytes=staging) == data
        # bits at or past n_granules: ignored and not counted
        n = 70
        marked = [0, 64, 69]
        stray = model_bitmap(n, marked, stray=[70, 71]) + b"\xff" * 8
        want = model_pack(data, BLOCK, marked)
        assert hs.bdev_pack_marked(bdev, stray, BLOCK,
                                   length=n * BLOCK) == want
        assert hs.bdev_unpack_marked(target, stray, BLOCK, want,
                                     length=n * BLOCK) == 3
        assert target.read(0, N * BLOCK) == model_unpack(
            b"\xA5" * (N * BLOCK), BLOCK, marked, want)
        only_stray = model_bitmap(n, [], stray=[70, 71])
        assert hs.bdev_pack_marked(bdev, only_stray, BLOCK,
                                   length=n * BLOCK) == b""

    def test_rejections(self, volume):
        bdev = volume["bdev"]
        full = b"\xff" * ((N + 7) // 8)
        for granule, kwargs in (
                (768, {}),
                (BLOCK, {"src_offset": 100, "length": BLOCK}),
                (BLOCK, {"length": (N + 1) * BLOCK}),
                (BLOCK, {"src_offset": N * BLOCK, "length": BLOCK}),
                (BLOCK, {"src_offset": 2**64 - BLOCK}),
                (BLOCK, {"src_offset": 2**64 - BLOCK, "length": 2 * BLOCK}),
                (4096, {"staging_bytes": 4095})):
            with pytest.raises(RuntimeError):
                hs.bdev_pack_marked(bdev, full, granule, **kwargs)
        with pytest.raises(RuntimeError):  # short bitmap
            hs.bdev_pack_marked(bdev, b"\xff", BLOCK, length=9 * BLOCK)
        target = hs.create_malloc_bdev("dl-rej", BLOCK, 128)
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
                (BLOCK, one + b"x", {}),
                (BLOCK, b"", {})):
            with pytest.raises(RuntimeError):
                hs.bdev_unpack_marked(target, b"\x01" + bytes(15), granule,
                                      data, **kwargs)
        with pytest.raises(RuntimeError):  # short bitmap
            hs.bdev_unpack_marked(target, b"\x01", BLOCK, one,
                                  length=9 * BLOCK)
        assert target.read(0, 128 * BLOCK) == b"\xA5" * (128 * BLOCK)


PLANTED = [0, 63, 64, 200, N - 1]


def planted_pair(prefix):
    """A volume and the clone it diverged from in PLANTED."""
    data = indexed_bytes(N)
    base = hs.create_malloc_bdev(prefix + "-base", BLOCK, N)
    base.write(0, data)
    live = bytearray(data)
    for g in PLANTED:
        live[g * BLOCK:(g + 1) * BLOCK] = bytes([g % 251 + 1]) * BLOCK
    src = hs.create_malloc_bdev(prefix + "-src", BLOCK, N)
    src.write(0, bytes(live))
    return src, base, bytes(live)


class TestFileFormat:
    def test_full_and_delta_match_documented_layout(self, tmp_path):
        src, base, live = planted_pair("dl-ff")
        full_path = str(tmp_path / "v.full")
        delta_path = str(tmp_path / "v.delta")
        r = hs.bdev_export_delta(src, full_path)
        want = build_delta_file(live, BLOCK)
        assert open(full_path, "rb").read() == want
        assert r == {"version": 1, "block_size": BLOCK, "granule": BLOCK,
                     "full": True, "volume_bytes": N * BLOCK, "granules": N,
                     "marked": N, "file_bytes": len(want)}
        assert hs.delta_file_info(full_path) == r
        r = hs.bdev_export_delta(src, delta_path, base=base)
        want = build_delta_file(live, BLOCK, PLANTED)
        assert open(delta_path, "rb").read() == want
        assert r["marked"] == len(PLANTED) and not r["full"]
        assert r["file_bytes"] == len(want)
        assert hs.delta_file_info(delta_path) == r
        assert not os.path.exists(full_path + ".tmp")
        assert not os.path.exists(delta_path + ".tmp")

    def test_coarse_granule_cuts_several_records(self, tmp_path):
        """4 KiB granules, 300 marked: records of 256 and 44."""
        n = 300
        data = indexed_bytes(n * 8, salt=5)
        src = hs.create_malloc_bdev("dl-rec", BLOCK, n * 8)
        src.write(0, data)
        path = str(tmp_path / "rec.full")
        r = hs.bdev_export_delta(src, path, granule=4096)
        want = build_delta_file(data, 4096)
        assert open(path, "rb").read() == want
        assert r["file_bytes"] == HEADER + 40 + 2 * 8 + n * 4096 + TRAILER
        back = hs.create_malloc_bdev("dl-rec-back", BLOCK, n * 8)
        assert hs.bdev_import_delta(back, path)["marked"] == n
        assert back.read(0, len(data)) == data

    def test_identical_base_gives_empty_delta(self, tmp_path):
        src, _, live = planted_pair("dl-same")
        path = str(tmp_path / "same.delta")
        r = hs.bdev_export_delta(src, path, base=src)
        assert r["marked"] == 0
        assert open(path, "rb").read() == build_delta_file(live, BLOCK, [])
        target = hs.create_malloc_bdev("dl-same-t", BLOCK, N)
        assert hs.bdev_import_delta(target, path)["marked"] == 0
        assert target.read(0, N * BLOCK) == bytes(N * BLOCK)

    def test_export_refusals(self, tmp_path):
        src, base, _ = planted_pair("dl-ref")
        path = str(tmp_path / "x.delta")
        hs.bdev_export_delta(src, path)
        before = open(path, "rb").read()
        with pytest.raises(RuntimeError, match="exists"):
            hs.bdev_export_delta(src, path, base=base)
        assert open(path, "rb").read() == before
        hs.bdev_export_delta(src, path, base=base, overwrite=True)
        assert hs.delta_file_info(path)["marked"] == len(PLANTED)
        other = hs.create_malloc_bdev("dl-ref-o", BLOCK, N + 1)
        with pytest.raises(ValueError):
            hs.bdev_export_delta(src, str(tmp_path / "y"), base=other)
        with pytest.raises(ValueError):
            hs.bdev_export_delta(src, str(tmp_path / "y"), granule=768)
        with pytest.raises(RuntimeError):
            hs.bdev_export_delta(src, str(tmp_path / "no-dir" / "y"))
        assert sorted(os.listdir(tmp_path)) == ["x.delta"]


class TestRestore:
    def test_full_plus_two_deltas(self, tmp_path):
        """Checkpoint, write, checkpoint against the snapshot, twice;
        the chain applied in order onto a fresh volume reproduces the
        live one."""
        rng = random.Random(11)
        live = hs.create_malloc_bdev("dl-live", BLOCK, N)
        live.write(0, indexed_bytes(N))
        paths = [str(tmp_path / f"c{i}") for i in range(3)]
        assert hs.bdev_export_delta(live, paths[0])["marked"] == N
        for i in (1, 2):
            snap = hs.create_malloc_bdev(f"dl-snap{i}", BLOCK, N)
            snap.write(0, live.read(0, N * BLOCK))
            touched = sorted(rng.sample(range(N), 9))
            for g in touched:
                live.write(g * BLOCK, bytes([i * 16 + g % 13]) * BLOCK)
            r = hs.bdev_export_delta(live, paths[i], base=snap)
            assert r["marked"] == len(touched)
        fresh = hs.create_malloc_bdev("dl-fresh", BLOCK, N + 3)
        fresh.fill(0, 0xA5, (N + 3) * BLOCK)
        for path in paths:
            before = fresh.read(0, (N + 3) * BLOCK)
            hs.bdev_import_delta(fresh, path, dry_run=True)
            assert fresh.read(0, (N + 3) * BLOCK) == before
            hs.bdev_import_delta(fresh, path)
        assert hs.bdev_diff(live, fresh)["mismatched"] == 0
        # a larger target keeps what lies past the file's volume
        assert fresh.read(N * BLOCK, 3 * BLOCK) == b"\xA5" * (3 * BLOCK)


# --- hostile files, through the daemon ---------------------------------------

def hostile_variants(valid):
    """(name, blob, structural): structural failures must leave the
    target untouched; a bad payload is caught by dry_run."""
    n_words = (N + 63) // 64
    records = HEADER + n_words * 8

    def flip(blob, at):
        blob = bytearray(blob)
        blob[at] ^= 0x40
        return bytes(blob)

    def header_field(offset, fmt, value):
        blob = bytearray(valid)
        blob[offset:offset + struct.calcsize(fmt)] = struct.pack(fmt, value)
        return refresh_header_crc(blob)

    out = [
        ("payload byte", flip(valid, records + 8 + 3 * BLOCK + 17), False),
        ("record crc", flip(valid, records + 5), False),
        ("record count", flip(valid, records), False),
        ("bitmap byte", flip(valid, HEADER + 3), True),
        ("header byte", flip(valid, 30), True),
        ("header crc", flip(valid, 61), True),
        ("magic", b"HSDELTA2" + valid[8:], True),
        ("end magic", flip(valid, len(valid) - 12), True),
        ("trailer count", flip(valid, len(valid) - 8), True),
        ("trailing garbage", valid + b"\0", True),
        ("empty", b"", True),
        ("version 2", header_field(8, "<I", 2), True),
        ("unknown flag", header_field(20, "<I", 2), True),
        ("reserved", header_field(52, "<I", 1), True),
        ("n_marked + 1", header_field(40, "<Q", len(PLANTED) + 1), True),
        ("n_marked - 1", header_field(40, "<Q", len(PLANTED) - 1), True),
        ("n_granules huge", header_field(32, "<Q", 2**63), True),
        ("granule 0", header_field(16, "<I", 0), True),
        ("granule 24", header_field(16, "<I", 24), True),
        ("block size 4096", header_field(12, "<I", 4096), True),
    ]
    for cut in (0, 7, 63, 64, HEADER + 8, records, records + 8,
                len(valid) - TRAILER, len(valid) - 1):
        out.append((f"truncated at {cut}", valid[:cut], True))
    return out


def serve_volume(client, name, data, tmp_path, block_size=BLOCK):
    """A daemon volume with known content: a full file built here,
    imported."""
    hipstore.construct_malloc_bdev(client, num_blocks=len(data) // block_size,
                                   block_size=block_size, name=name)
    path = str(tmp_path / f"{name}.seed")
    with open(path, "wb") as f:
        f.write(build_delta_file(data, block_size, block_size=block_size))
    r = hipstore.bdev_import_delta(client, name, path)
    assert r["applied"] == len(data) // block_size
    os.unlink(path)


class TestHostileFiles:
    def test_each_is_refused_and_the_daemon_lives(self, hipstored, tmp_path):  # noqa: F811
        base = indexed_bytes(N)
        live = bytearray(base)
        for g in PLANTED:
            live[g * BLOCK:(g + 1) * BLOCK] = bytes([g % 251 + 1]) * BLOCK
        valid = build_delta_file(bytes(live), BLOCK, PLANTED)
        path = str(tmp_path / "hostile")
        with hipstore.Client(hipstored.socket_path) as client:
            serve_volume(client, "ht", base, tmp_path)
            hipstore.bdev_clone(client, "ht", "ht-pristine")
            for name, blob, structural in hostile_variants(valid):
                with open(path, "wb") as f:
                    f.write(blob)
                for dry_run in (True, False) if not structural else (False,):
                    if not dry_run and not structural:
                        # dry_run caught it and wrote nothing
                        assert hipstore.bdev_compare(
                            client, "ht", "ht-pristine")["mismatched"] == 0
                    with pytest.raises(hipstore.RpcError) as err:
                        hipstore.bdev_import_delta(client, "ht", path,
                                                   dry_run=dry_run)
                    assert err.value.code == hipstore.ERROR_INVALID_PARAMS, \
                        (name, str(err.value))
                if structural:
                    assert hipstore.bdev_compare(
                        client, "ht", "ht-pristine")["mismatched"] == 0, name
                else:
                    assert "partly" in str(err.value), name
                assert "bdev_import_delta" in client.invoke("get_rpc_methods")
            # the file is fine for a volume it fits
            with open(path, "wb") as f:
                f.write(valid)
            hipstore.construct_malloc_bdev(client, num_blocks=N - 1,
                                           block_size=BLOCK, name="ht-small")
            hipstore.construct_malloc_bdev(client, num_blocks=N // 8 + 1,
                                           block_size=4096, name="ht-4k")
            for target in ("ht-small", "ht-4k"):
                with pytest.raises(hipstore.RpcError) as err:
                    hipstore.bdev_import_delta(client, target, path)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS
            # restore "ht" to its base, then the valid delta applies
            r = hipstore.bdev_export_delta(client, "ht-pristine",
                                           str(tmp_path / "pristine.full"))
            hipstore.bdev_import_delta(client, "ht",
                                       str(tmp_path / "pristine.full"))
            assert r["saved"] == N
            r = hipstore.bdev_import_delta(client, "ht", path)
            assert r == {"granule": BLOCK, "granules": N,
                         "applied": len(PLANTED)}
            r = hipstore.bdev_compare(client, "ht", "ht-pristine",
                                      max_report=64)
            assert r["first_mismatches"] == PLANTED

    def test_random_mutations_are_all_answered(self, hipstored, tmp_path):  # noqa: F811
        rng = random.Random(2026)
        data = indexed_bytes(64 + 7, salt=3)
        marked = [0, 5, 63, 64, 70]
        valid = build_delta_file(data, BLOCK, marked)
        path = str(tmp_path / "mutant")
        outcomes = {"ok": 0, "refused": 0}
        with hipstore.Client(hipstored.socket_path) as client:
            hipstore.construct_malloc_bdev(client, num_blocks=64 + 7,
                                           block_size=BLOCK, name="mu")
            for i in range(200):
                blob = bytearray(valid)
                kind = rng.choice(("byte", "byte", "byte", "cut", "grow"))
                if kind == "byte":
                    blob[rng.randrange(len(blob))] ^= 1 << rng.randrange(8)
                elif kind == "cut":
                    del blob[rng.randrange(len(blob)):]
                else:
                    blob += bytes(rng.randrange(1, 600))
                with open(path, "wb") as f:
                    f.write(blob)
                try:
                    r = hipstore.bdev_import_delta(client, "mu", path,
                                                   dry_run=i % 2 == 0)
                    assert r["applied"] == len(marked)
                    outcomes["ok"] += 1
                except hipstore.RpcError as err:
                    assert err.code == hipstore.ERROR_INVALID_PARAMS, \
                        (i, kind, str(err))
                    outcomes["refused"] += 1
            assert "bdev_export_delta" in client.invoke("get_rpc_methods")
        # every bit of the file is covered by a CRC, a length or a magic
        assert outcomes == {"ok": 0, "refused": 200}


class TestDaemonFiles:
    def test_export_import_and_refusals(self, hipstored, tmp_path):  # noqa: F811
        data = indexed_bytes(N)
        with hipstore.Client(hipstored.socket_path) as client:
            methods = client.invoke("get_rpc_methods")
            assert "bdev_export_delta" in methods
            assert "bdev_import_delta" in methods
            serve_volume(client, "df", data, tmp_path)
            path = str(tmp_path / "df.full")
            r = hipstore.bdev_export_delta(client, "df", path)
            want = build_delta_file(data, BLOCK)
            assert r == {"granule": BLOCK, "granules": N, "saved": N,
                         "file_bytes": len(want), "full": True}
            assert open(path, "rb").read() == want
            # existing path: refused without overwrite, file untouched
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_export_delta(client, "df", path, granule=3584)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert open(path, "rb").read() == want
            r = hipstore.bdev_export_delta(client, "df", path, granule=3584,
                                           overwrite=True)
            assert r["granule"] == 3584 and r["granules"] == N // 7
            assert open(path, "rb").read() == build_delta_file(data, 3584)
            # a base of another size, a bad granule, bad parameters
            hipstore.construct_malloc_bdev(client, num_blocks=N + 1,
                                           block_size=BLOCK, name="df-big")
            out = str(tmp_path / "never")
            for params in ({"name": "df", "path": out, "base": "df-big"},
                           {"name": "df", "path": out, "granule": 768},
                           {"name": "df", "path": out, "granule": -512},
                           {"name": "df", "path": out, "granule": 2**33},
                           {"name": "df"},
                           {"name": "df", "path": ""},
                           {"name": "df", "path": 7},
                           {"name": "nope", "path": out},
                           {"name": "df", "path": out, "base": "nope"},
                           {"path": out}):
                with pytest.raises(hipstore.RpcError) as err:
                    client.invoke("bdev_export_delta", params)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS, params
            for params in ({"name": "df"}, {"name": "df", "path": ""},
                           {"name": "nope", "path": path}, {"path": path}):
                with pytest.raises(hipstore.RpcError) as err:
                    client.invoke("bdev_import_delta", params)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS, params
            # I/O failures are -32603 and leave no .tmp behind
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_export_delta(client, "df",
                                           str(tmp_path / "no-dir" / "f"))
            assert err.value.code == hipstore.ERROR_INTERNAL
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_import_delta(client, "df", out)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert sorted(os.listdir(tmp_path)) == [
                "df.full", "hipstored.sock", "hipstored.stderr"]
            # a claimed target is refused; export and dry_run are not
            hipstore.construct_vhost_scsi_controller(client, "df-ctrl")
            hipstore.add_vhost_scsi_lun(client, "df-ctrl", 0, "df")
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_import_delta(client, "df", path)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert "claimed" in str(err.value)
            assert hipstore.bdev_import_delta(
                client, "df", path, dry_run=True)["applied"] == N // 7
            assert hipstore.bdev_export_delta(
                client, "df", path, overwrite=True)["saved"] == N
            hipstore.remove_vhost_controller(client, "df-ctrl")
            assert hipstore.bdev_import_delta(client, "df",
                                              path)["applied"] == N


# --- oim.v0 and oimctl ------------------------------------------------------------

METADATA = ((spec.CONTROLLER_ID_KEY, "c0"),)
SIZE = 1 << 20


@pytest.fixture
def stack(hipstored, tmp_path):  # noqa: F811
    registry = Registry(db=MemRegistryDB())
    reg_server = RegistryServer(f"unix://{tmp_path}/reg.sock", registry)
    reg_server.start()
    controller = Controller(controller_id="c0",
                            hipstored_socket=hipstored.socket_path)
    ctrl_server = ControllerServer(f"unix://{tmp_path}/ctrl.sock", controller)
    ctrl_server.start()
    registry.db.store(["c0", "address"], f"unix://{tmp_path}/ctrl.sock")
    channel = grpc.insecure_channel(grpc_target(reg_server.addr()))
    stub = spec.ControllerStub(channel)
    stub.endpoint = reg_server.addr()
    stub.socket_path = hipstored.socket_path
    yield stub
    channel.close()
    ctrl_server.stop()
    reg_server.stop()


def provision(stack, name, size=SIZE):
    stack.ProvisionMallocBDev(
        spec.ProvisionMallocBDevRequest(bdev_name=name, size=size),
        metadata=METADATA, timeout=30)


class TestOimV0:
    def test_checkpoint_restore_chain(self, stack, tmp_path):
        base = indexed_bytes(N)
        live = bytearray(base)
        for g in PLANTED:
            live[g * BLOCK:(g + 1) * BLOCK] = bytes([g % 251 + 1]) * BLOCK
        for name, blob in (("seed", build_delta_file(base, BLOCK)),
                           ("edit", build_delta_file(bytes(live), BLOCK,
                                                     PLANTED))):
            with open(tmp_path / name, "wb") as f:
                f.write(blob)

        def checkpoint(**kwargs):
            return stack.CheckpointMallocBDev(
                spec.CheckpointMallocBDevRequest(**kwargs),
                metadata=METADATA, timeout=30)

        def restore(name, path, dry_run=False):
            return stack.RestoreMallocBDev(
                spec.RestoreMallocBDevRequest(
                    bdev_name=name, path=str(tmp_path / path),
                    dry_run=dry_run),
                metadata=METADATA, timeout=30)

        provision(stack, "cv", N * BLOCK)
        assert restore("cv", "seed").applied == N
        stack.CloneMallocBDev(
            spec.CloneMallocBDevRequest(source="cv", dest="cv-snap"),
            metadata=METADATA, timeout=30)
        full = checkpoint(bdev_name="cv", path=str(tmp_path / "cv.full"))
        assert (full.granules, full.saved) == (N, N)
        assert open(tmp_path / "cv.full", "rb").read() == \
            open(tmp_path / "seed", "rb").read()
        assert full.file_bytes == os.path.getsize(tmp_path / "cv.full")
        assert restore("cv", "edit").applied == len(PLANTED)
        delta = checkpoint(bdev_name="cv", base_name="cv-snap",
                           path=str(tmp_path / "cv.d1"))
        assert (delta.granules, delta.saved) == (N, len(PLANTED))
        assert open(tmp_path / "cv.d1", "rb").read() == \
            open(tmp_path / "edit", "rb").read()
        provision(stack, "cv-new", N * BLOCK)
        assert restore("cv-new", "cv.full").applied == N
        assert restore("cv-new", "cv.d1", dry_run=True).applied == \
            len(PLANTED)
        with hipstore.Client(stack.socket_path) as client:
            assert hipstore.bdev_compare(client, "cv-snap",
                                         "cv-new")["mismatched"] == 0
            assert restore("cv-new", "cv.d1").granules == N
            assert hipstore.bdev_compare(client, "cv",
                                         "cv-new")["mismatched"] == 0

    def test_error_mapping(self, stack, tmp_path):
        provision(stack, "em")
        provision(stack, "em-big", 2 * SIZE)
        path = str(tmp_path / "em.full")

        def checkpoint(**kwargs):
            return stack.CheckpointMallocBDev(
                spec.CheckpointMallocBDevRequest(**kwargs),
                metadata=METADATA, timeout=30)

        def restore(**kwargs):
            return stack.RestoreMallocBDev(
                spec.RestoreMallocBDevRequest(**kwargs),
                metadata=METADATA, timeout=30)

        checkpoint(bdev_name="em", path=path)
        with open(tmp_path / "junk", "wb") as f:
            f.write(b"HSDELTA1" + bytes(100))
        cases = (
            (checkpoint, {"bdev_name": "nope", "path": path},
             grpc.StatusCode.NOT_FOUND),
            (checkpoint, {"bdev_name": "em", "base_name": "nope",
                          "path": path}, grpc.StatusCode.NOT_FOUND),
            (checkpoint, {"bdev_name": "em"},
             grpc.StatusCode.INVALID_ARGUMENT),
            (checkpoint, {"path": path}, grpc.StatusCode.INVALID_ARGUMENT),
            (checkpoint, {"bdev_name": "em", "base_name": "em-big",
                          "path": str(tmp_path / "other")},
             grpc.StatusCode.INVALID_ARGUMENT),
            (checkpoint, {"bdev_name": "em", "path": path},
             grpc.StatusCode.ALREADY_EXISTS),
            (restore, {"bdev_name": "nope", "path": path},
             grpc.StatusCode.NOT_FOUND),
            (restore, {"bdev_name": "em"}, grpc.StatusCode.INVALID_ARGUMENT),
            (restore, {"bdev_name": "em", "path": str(tmp_path / "junk")},
             grpc.StatusCode.INVALID_ARGUMENT),
            (restore, {"bdev_name": "em", "path": str(tmp_path)},
             grpc.StatusCode.INVALID_ARGUMENT),
        )
        for call, kwargs, code in cases:
            with pytest.raises(grpc.RpcError) as err:
                call(**kwargs)
            assert err.value.code() == code, kwargs
        checkpoint(bdev_name="em", path=path, overwrite=True)
        # mapped = claimed: restore is refused, a dry run is not
        stack.MapVolume(
            spec.MapVolumeRequest(volume_id="em", malloc=spec.MallocParams()),
            metadata=METADATA, timeout=30)
        with pytest.raises(grpc.RpcError) as err:
            restore(bdev_name="em", path=path)
        assert err.value.code() == grpc.StatusCode.FAILED_PRECONDITION
        assert restore(bdev_name="em", path=path,
                       dry_run=True).applied == SIZE // BLOCK
        stack.UnmapVolume(spec.UnmapVolumeRequest(volume_id="em"),
                          metadata=METADATA, timeout=30)
        assert restore(bdev_name="em", path=path).applied == SIZE // BLOCK

    def test_oimctl_verbs(self, stack, tmp_path, capsys):
        provision(stack, "oc")
        base = ["--registry", stack.endpoint]
        full = str(tmp_path / "oc.full")
        assert oimctl.main(base + ["checkpoint", "--controller", "c0", "oc",
                                   full]) == 0
        assert f"{SIZE // BLOCK} of {SIZE // BLOCK} granules" in \
            capsys.readouterr().out
        assert oimctl.main(base + ["clone", "--controller", "c0", "oc",
                                   "oc-snap"]) == 0
        delta = str(tmp_path / "oc.d1")
        assert oimctl.main(base + ["checkpoint", "--controller", "c0", "oc",
                                   delta, "--base", "oc-snap"]) == 0
        assert "0 of" in capsys.readouterr().out
        with pytest.raises(grpc.RpcError) as err:
            oimctl.main(base + ["checkpoint", "--controller", "c0", "oc",
                                delta])
        assert err.value.code() == grpc.StatusCode.ALREADY_EXISTS
        assert oimctl.main(base + ["checkpoint", "--controller", "c0", "oc",
                                   delta, "--overwrite"]) == 0
        capsys.readouterr()
        assert oimctl.main(base + ["restore", "--controller", "c0", "oc-snap",
                                   delta, "--dry-run"]) == 0
        assert "verified oc-snap" in capsys.readouterr().out
        assert oimctl.main(base + ["restore", "--controller", "c0", "oc-snap",
                                   full]) == 0
        assert "restored oc-snap" in capsys.readouterr().out
