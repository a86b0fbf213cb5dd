"""HSLZD1 (dictionary) granule codec on the host and version-4 delta files
on malloc bdevs. The reference is the prefix-aware LZ4 block decoder below
plus the original bytes; every comparison is exact. The decoder and the
volume are shared with test_dict_compress_gpu.py."""
import functools
import random
import struct

import pytest

from oim_amd import _hipstore as hs

N = 64 * 2 + 7  # granules: two bitmap words and a ragged third


def dict_decode(piece, d):
    """(X, [(literals, offset, match length), ...]) of a piece; d = D."""
    if len(piece) == len(d):
        return piece, []
    out, seqs, ip = bytearray(d), [], 0

    def length(nibble):
        nonlocal ip
        n = nibble
        while nibble == 15:
            n += piece[ip]
            ip += 1
            if piece[ip - 1] != 255:
                break
        return n

    while True:
        token = piece[ip]
        ip += 1
        lit = length(token >> 4)
        out += piece[ip:ip + lit]
        ip += lit
        if ip == len(piece):
            return bytes(out[len(d):]), seqs + [(lit, 0, 0)]
        offset = piece[ip] | piece[ip + 1] << 8
        ip += 2
        mlen = length(token & 15) + 4
        assert 1 <= offset <= len(out)
        for _ in range(mlen):
            out.append(out[-offset])
        seqs.append((lit, offset, mlen))


@functools.lru_cache(maxsize=None)
def volume(granule, n=N):
    """(D, X): n seeded random granules and their edits, kind i % 8."""
    rng = random.Random(granule)
    base = rng.randbytes(n * granule)
    out = []
    for i in range(n):
        d = base[i * granule:(i + 1) * granule]
        flip = lambda at: d[:at] + bytes([d[at] ^ 0x55]) + d[at + 1:]
        out.append([
            flip(granule // 2),         # 0: one byte mid-granule
            flip(2),                    # 1: no aligned winner at q = G
            rng.randbytes(3) + d[:-3],  # 2: shifted, table candidates only
            bytes(granule),             # 3: matches inside X, offset 1
            rng.randbytes(granule),     # 4: unrelated, raw
            d,                          # 5: equal, one maximal match
            d[-8:] + d[8:],             # 6: a match whose source ends D
            flip(19 + 255),             # 7: a length with a final 0 byte
        ][i % 8])
    return base, b"".join(out)


@pytest.mark.parametrize("granule", [512, 2048, 4096, 16384])
@pytest.mark.parametrize("kind", range(8))
def test_granule_round_trip(granule, kind):
    base, data = volume(granule)
    d = base[kind * granule:(kind + 1) * granule]
    x = data[kind * granule:(kind + 1) * granule]
    piece = hs.lz_compress_granule(x, dictionary=d)
    assert hs.lz_validate_granule(piece, granule, dictionary=True)
    assert hs.lz_decompress_granule(piece, granule, dictionary=d) == x
    decoded, seqs = dict_decode(piece, d)
    assert decoded == x
    if kind == 4:
        assert piece == x  # raw
        return
    assert seqs[-1][0] >= 5
    if kind in (0, 5) and granule == 4096:
        # two sequences (token, <= 4 literals, offset, <= 17 length bytes),
        # then token and 5 literals: <= 50 bytes
        assert len(piece) <= 64
    if kind == 5:
        assert seqs == [(0, granule, granule - 5), (5, 0, 0)]
    if kind == 2:  # the aligned candidate never hits
        assert all(s[1] != granule for s in seqs)
        assert any(s[1] == granule + 3 for s in seqs)
    if kind in (1, 3, 6):  # literals first / offset 1 / the end of D
        assert {1: seqs[0][0] > 0, 3: seqs[0][1] == 1,
                6: seqs[0][:2] == (0, 8)}[kind]
    if kind == 7:
        assert seqs[0] == (0, granule, 274) and piece[3:5] == b"\xff\x00"
    if kind != 3:  # a piece that reaches into D is no HSLZ1 piece
        assert not hs.lz_validate_granule(piece, granule)


def test_version_4_files(tmp_path):
    g = 4096
    d, x = volume(g)
    base, vol, fresh = (hs.create_malloc_bdev(f"lzd-{i}", 512, len(d) // 512)
                        for i in range(3))
    base.write(0, d), vol.write(0, x)
    path, full = str(tmp_path / "inc.v4"), str(tmp_path / "base.v1")
    # the four refusals, before anything is written
    hs.bdev_fingerprint_file(base, str(tmp_path / "map"), granule=g)
    for kwargs in ({"base": base}, {"compress": True},
                   {"compress": True, "base_map": str(tmp_path / "map")},
                   {"compress": True, "base": base, "key": bytes(range(64))}):
        with pytest.raises(ValueError, match="dictionary"):
            hs.bdev_export_delta(vol, path, granule=g, dictionary=True, **kwargs)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["map"]
    info = hs.bdev_export_delta(vol, path, base=base, granule=g,
                                compress=True, dictionary=True)
    marked = [i for i in range(N) if i % 8 != 5]
    pieces = [hs.lz_compress_granule(x[i * g:(i + 1) * g],
                                     dictionary=d[i * g:(i + 1) * g])
              for i in marked]
    blob = open(path, "rb").read()
    assert struct.unpack_from("<I", blob, 8)[0] == 4  # version; Lz and Dict:
    assert struct.unpack_from("<I", blob, 20)[0] == 2 | 8
    assert info["version"] == 4 and info["dictionary"] and info["compressed"]
    assert (info["marked"], info["stored_bytes"]) == (
        len(marked), sum(map(len, pieces)))
    assert b"".join(pieces) in blob  # one record: the pieces back to back
    assert hs.delta_file_info(path) == info
    # full file plus the version-4 delta restores the data
    hs.bdev_export_delta(base, full, granule=g)
    hs.bdev_import_delta(fresh, full)
    assert hs.bdev_import_delta(fresh, path, dry_run=True)["marked"] == len(marked)
    assert fresh.read(0, len(d)) == d
    assert hs.bdev_import_delta(fresh, path)["marked"] == len(marked)
    assert fresh.read(0, len(x)) == x
    # a CRC-clean file whose first piece has an offset past the dictionary
    at = blob.index(pieces[0])
    bad = bytearray(blob)
    bad[at + 1:at + 3] = struct.pack("<H", g + 1)
    head = 64 + 8 * 3  # header and bitmap, then the one record
    size = struct.unpack_from("<I", bad, head + 8)[0]
    struct.pack_into("<I", bad, head + 4,
                     hs.crc32c(bytes(bad[head + 16:head + 16 + size])))
    open(path, "wb").write(bad)
    fresh.write(0, d)
    for dry_run in (True, False):
        with pytest.raises(ValueError, match="granule 0: bad compressed piece"):
            hs.bdev_import_delta(fresh, path, dry_run=dry_run)
    assert fresh.read(0, len(d)) == d  # refused before anything was written
