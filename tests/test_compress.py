"""HSLZ1 granule codec on the host and version-2 (compressed) delta
files on malloc bdevs.

The reference is the plain LZ4 block decoder below plus the original
bytes; every comparison is exact. lz4_decode and the content classes
are shared with test_compress_gpu.py."""

import random
import struct

import pytest

from oim_amd import _hipstore as hs

from test_delta import build_delta_file, model_bitmap, refresh_header_crc

GRANULES = [512, 4096, 16384]


def lz4_decode(block):
    """(decoded bytes, [(literals, offset, match length), ...]) of a legal
    LZ4 block; the last sequence has offset 0 and length 0."""
    out = bytearray()
    seqs = []
    ip = 0

    def length(nibble):
        nonlocal ip
        n = nibble
        while nibble == 15:
            n += block[ip]
            ip += 1
            if block[ip - 1] != 255:
                break
        return n

    while True:
        token = block[ip]
        ip += 1
        lit = length(token >> 4)
        out += block[ip:ip + lit]
        ip += lit
        if ip == len(block):
            seqs.append((lit, 0, 0))
            return bytes(out), seqs
        offset = block[ip] | block[ip + 1] << 8
        ip += 2
        mlen = length(token & 15) + 4
        assert 1 <= offset <= len(out)
        for _ in range(mlen):
            out.append(out[-offset])
        seqs.append((lit, offset, mlen))


def stored_decode(piece, granule):
    """A stored piece: raw when its size is the granule."""
    return piece if len(piece) == granule else lz4_decode(piece)[0]


def contents(granule):
    """name -> one granule of each content class of the codec's tests."""
    rng = random.Random(granule)
    rnd = rng.randbytes(granule)
    words = [bytes(rng.choices(b"etaoinshrdlu", k=rng.randint(2, 9)))
             for _ in range(200)]
    text = b" ".join(rng.choice(words) for _ in range(granule))[:granule]
    out = {
        "zeros": bytes(granule),
        "random": rnd,
        "period1": b"\xab" * granule,
        "period3": (b"abc" * granule)[:granule],
        "period7": (b"abcdefg" * granule)[:granule],
        # the only repeat: 32 bytes from position 10 again at 300
        "far": rnd[:300] + rnd[10:42] + bytes(granule - 332),
        # the only repeat starts at 112 and crosses position 128
        "straddle": rnd[:112] + rnd[8:40] + bytes(granule - 144),
        # the second half repeats the first: the match must stop at G - 5
        "to_end": rnd[:granule // 2] * 2,
        "text": text,
    }
    for lit in (14, 15, 270):
        # zeros (a match up to 128), exactly `lit` non-zero literals, zeros.
        # None of the literals' u32s may share the table slot of u32 0
        # (slot 0 of the documented hash), or the match after them would
        # be found late: draw until the input has that property.
        body = b""
        while not all((int.from_bytes(body[q:q + 4], "little") * 2654435761
                       & 0xFFFFFFFF) >> 21 for q in range(128, 128 + lit)):
            fresh = bytes(rng.choices(range(1, 255), k=lit))
            body = bytes(128) + fresh + bytes(granule - 128 - lit)
        out[f"lit{lit}"] = body
    assert all(len(v) == granule for v in out.values())
    return out


CASES = [(g, name) for g in GRANULES for name in contents(512)]


@pytest.mark.parametrize("granule,name", CASES)
def test_granule_round_trip(granule, name):
    data = contents(granule)[name]
    piece = hs.lz_compress_granule(data)
    assert 1 <= len(piece) <= granule
    assert hs.lz_validate_granule(piece, granule)
    assert hs.lz_decompress_granule(piece, granule) == data
    if name == "random":
        assert piece == data  # raw
        return
    assert len(piece) < granule
    decoded, seqs = lz4_decode(piece)
    assert decoded == data
    # end-of-block rules
    assert seqs[-1][0] >= 5
    starts = [sum(s[0] + s[2] for s in seqs[:i]) + seqs[i][0]
              for i in range(len(seqs) - 1)]
    assert all(q <= granule - 12 for q in starts)
    if name == "zeros":  # first window literal, then one maximal match
        assert seqs == [(64, 1, granule - 69), (5, 0, 0)]
    if name in ("period3", "period7"):
        assert seqs[0][1] % int(name[-1]) == 0 and seqs[0][2] > seqs[0][1]
    if name == "to_end":
        assert seqs[-2][1] == granule // 2 and seqs[-1] == (5, 0, 0)
    if name == "far":  # found at 300, or a little later after a collision
        assert seqs[0][1] == 290 and 300 <= seqs[0][0] < 328
    if name == "straddle":
        assert seqs[0][1] == 104 and 112 <= seqs[0][0] < 128 < sum(seqs[0][::2])
    if name.startswith("lit"):
        assert seqs[0] == (64, 1, 64) and seqs[1][0] == int(name[3:])


def ext(n):
    return bytes([255] * ((n - 15) // 255) + [(n - 15) % 255]) if n >= 15 else b""


def block_of(granule, offset=8, mlen=None, last_token=0x50, tail=b"ZZZZZ"):
    """8 literals, one long match, 5 final literals: legal as it stands."""
    mlen = granule - 13 if mlen is None else mlen
    return (bytes([0x8F]) + b"A" * 8 + struct.pack("<H", offset) +
            ext(mlen - 4) + bytes([last_token]) + tail)


@pytest.mark.parametrize("granule", GRANULES)
def test_malformed_pieces_are_refused(granule):
    """Host functions only: none of these streams is for a GPU call."""
    good = block_of(granule)
    assert hs.lz_validate_granule(good, granule)
    assert lz4_decode(good)[0] == hs.lz_decompress_granule(good, granule)
    bad = {
        "offset 0": block_of(granule, offset=0),
        "offset past the start": block_of(granule, offset=9),
        "match overruns G": block_of(granule, mlen=granule - 12),
        "match into the last 5": block_of(granule, mlen=granule - 10, tail=b"ZZ",
                                          last_token=0x20),
        "literals overrun the piece": block_of(granule, last_token=0x60),
        "truncated in the literals": good[:-3],
        "truncated in the length": good[:12],
        "truncated in the offset": good[:10],
        "output shorter than G": block_of(granule, mlen=granule - 14),
        "empty": b"",
        "longer than G": bytes(granule + 1),
    }
    for what, piece in bad.items():
        assert not hs.lz_validate_granule(piece, granule), what
        with pytest.raises(ValueError):
            hs.lz_decompress_granule(piece, granule)


def build_delta_file_v2(data, granule, marked, pieces, block_size=512,
                        full=False):
    """The documented version-2 layout around the given stored pieces."""
    n = len(data) // granule
    bitmap = model_bitmap(n, marked, pad_to_words=True)
    per_record = max(1, (1 << 20) // granule)
    records = []
    for i in range(0, len(marked), per_record):
        part = pieces[i:i + per_record]
        payload = b"".join(struct.pack("<I", len(p)) for p in part) + b"".join(part)
        records.append(struct.pack("<IIII", len(part), hs.crc32c(payload),
                                   len(payload), 0) + payload)
    area = b"".join(records)
    head = b"HSDELTA1" + struct.pack(
        "<IIIIQQQIQ", 2, block_size, granule, 2 | (1 if full else 0),
        len(data), n, len(marked), hs.crc32c(bitmap), len(area))
    return (head + struct.pack("<I", hs.crc32c(head)) + bitmap + area +
            b"HSDEND1\0" + struct.pack("<Q", len(marked)))


@pytest.fixture(scope="module")
def volume():
    """A malloc bdev of 4 KiB granules, one per content class and then
    some, and its content. Read-only."""
    granule = 4096
    data = b"".join(contents(granule).values()) * 6  # 72 granules
    bdev = hs.create_malloc_bdev("lz-vol", 512, len(data) // 512)
    bdev.write(0, data)
    return {"bdev": bdev, "data": data, "granule": granule,
            "n": len(data) // granule}


class TestCompressedFiles:
    def test_export_info_dry_run_import(self, volume, tmp_path):
        g, n, data = volume["granule"], volume["n"], volume["data"]
        path = str(tmp_path / "vol.lz")
        info = hs.bdev_export_delta(volume["bdev"], path, granule=g,
                                    compress=True)
        pieces = [hs.lz_compress_granule(data[i * g:(i + 1) * g])
                  for i in range(n)]
        blob = open(path, "rb").read()
        assert blob == build_delta_file_v2(data, g, list(range(n)), pieces,
                                           full=True)
        assert info["version"] == 2 and info["compressed"] and info["full"]
        assert info["stored_bytes"] == sum(map(len, pieces)) < len(data)
        assert info["file_bytes"] == len(blob)
        assert hs.delta_file_info(path) == info
        fresh = hs.create_malloc_bdev("lz-new", 512, len(data) // 512)
        assert hs.bdev_import_delta(fresh, path, dry_run=True)["marked"] == n
        assert fresh.read(0, len(data)) == bytes(len(data))
        assert hs.bdev_import_delta(fresh, path)["marked"] == n
        assert fresh.read(0, len(data)) == data

    def test_delta_against_base_and_small_windows(self, volume, tmp_path):
        """Sparse marks through bdev_compress_marked with windows of 3
        granules, then back onto a sentinel volume."""
        g, n, data = volume["granule"], volume["n"], volume["data"]
        marked = [0, 9, 10, 11, 63, 64, 65, n - 1]
        bitmap = model_bitmap(n, marked)
        sizes, blob = hs.bdev_compress_marked(volume["bdev"], bitmap, g,
                                              staging_bytes=6 * g)
        want = [hs.lz_compress_granule(data[i * g:(i + 1) * g]) for i in marked]
        assert sizes == list(map(len, want)) and blob == b"".join(want)
        target = hs.create_malloc_bdev("lz-tgt", 512, len(data) // 512)
        target.write(0, b"\xa5" * len(data))
        assert hs.bdev_decompress_marked(target, bitmap, g, sizes, blob,
                                         staging_bytes=6 * g) == len(marked)
        got = target.read(0, len(data))
        for i in range(n):
            assert got[i * g:(i + 1) * g] == (
                data[i * g:(i + 1) * g] if i in marked else b"\xa5" * g), i

    def test_uncompressed_export_is_version_1(self, volume, tmp_path):
        path = str(tmp_path / "vol.v1")
        info = hs.bdev_export_delta(volume["bdev"], path,
                                    granule=volume["granule"])
        assert open(path, "rb").read() == build_delta_file(
            volume["data"], volume["granule"])
        assert info["version"] == 1 and "compressed" not in info

    def test_unsupported_granule(self, volume, tmp_path):
        for granule in (32768, 256):
            bdev = hs.create_malloc_bdev(f"lz-g{granule}", 256, 512)
            with pytest.raises(ValueError, match="granule"):
                hs.bdev_export_delta(bdev, str(tmp_path / "x"), granule=granule,
                                     compress=True)
            with pytest.raises(ValueError, match="granule"):
                hs.bdev_compress_marked(bdev, b"\x01" + bytes(63), granule)

    def test_structural_failures(self, volume, tmp_path):
        g, data = volume["granule"], volume["data"][:8 * 4096]
        pieces = [hs.lz_compress_granule(data[i * g:(i + 1) * g])
                  for i in range(8)]
        marked = list(range(8))
        good = build_delta_file_v2(data, g, marked, pieces, full=True)
        payload_at = 64 + 8 + 16 + 8 * 4  # header, bitmap, record head, sizes

        def flipped(blob, at):
            return blob[:at] + bytes([blob[at] ^ 0x40]) + blob[at + 1:]

        area = struct.unpack_from("<Q", good, 52)[0]
        hostile = {
            "record_area_bytes": refresh_header_crc(
                good[:52] + struct.pack("<Q", area + 16) + good[60:]),
            "size 0": build_delta_file_v2(
                data, g, marked, [b""] + pieces[1:], full=True),
            "size above G": build_delta_file_v2(
                data, g, marked, [bytes(g + 16)] + pieces[1:], full=True),
            "flipped payload byte": flipped(good, payload_at + 3),
            "version 2 without the flag": refresh_header_crc(
                good[:20] + struct.pack("<I", 1) + good[24:]),
            # a CRC-clean record whose first piece has offset 0
            "bad piece": build_delta_file_v2(
                data, g, marked, [block_of(g, offset=0)] + pieces[1:],
                full=True),
        }
        target = hs.create_malloc_bdev("lz-hostile", 512, len(data) // 512)
        path = str(tmp_path / "hostile.lz")
        for what, blob in hostile.items():
            with open(path, "wb") as f:
                f.write(blob)
            for dry_run in (True, False):
                with pytest.raises(ValueError):
                    hs.bdev_import_delta(target, path, dry_run=dry_run)
        with open(path, "wb") as f:
            f.write(good)
        assert hs.bdev_import_delta(target, path)["marked"] == 8
        assert target.read(0, len(data)) == data
