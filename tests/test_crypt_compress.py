"""HSXTS2 (XTS with ciphertext stealing) on the host and version-5 delta
files on malloc bdevs, against the pure-Python XTS of xts_model.py plus
the stealing below; plaintext pieces come from the hs.lz_* host codec."""
import random
import struct

import pytest

import xts_model as xm
from oim_amd import _hipstore as hs

KEY = bytes(range(1, 65))


def _block(key, unit, j, data):
    """E(data, T_j): one block under the tweak of block j."""
    t = int.from_bytes(xm.encrypt_block(
        xm.expand(key[32:]), unit.to_bytes(8, "little") + bytes(8)), "little")
    for _ in range(j):
        t = (t << 1) ^ (0x87 if t >> 127 else 0)
        t &= (1 << 128) - 1
    mask = t.to_bytes(16, "little")
    return xm._xor(xm.encrypt_block(xm.expand(key[:32]), xm._xor(data, mask)),
                   mask)


def xts_var(key, unit, data):
    """IEEE 1619 encryption of a unit of any length >= 16."""
    m, b = divmod(len(data), 16)
    if b == 0:
        return xm.xts_encrypt(key, unit, data)
    cc = _block(key, unit, m - 1, data[16 * (m - 1):16 * m])
    return (xm.xts_encrypt(key, unit, data[:16 * (m - 1)]) +
            _block(key, unit, m, data[16 * m:] + cc[b:]) + cc[:b])


def stored(key, unit, piece):
    """A piece as a keyed stream and a version-5 record hold it."""
    return xts_var(key, unit, piece.ljust(16, b"\0"))


def periodic(granule, period):
    """Random bytes repeated: compresses to about `period` bytes."""
    return (random.Random(period).randbytes(period) * granule)[:granule]


@pytest.mark.parametrize("n", [16, 17, 31, 32, 33, 1023, 1024, 1025, 1039, 1040])
def test_codec_against_the_model(n):
    data = random.Random(n).randbytes(n)
    cipher = hs.xts_encrypt_var(data, KEY, unit=n)
    assert cipher == xts_var(KEY, n, data)
    assert hs.xts_decrypt_var(cipher, KEY, unit=n) == data
    if n % 16 == 0:
        assert cipher == hs.xts_encrypt_units(data, n, KEY, first_unit=n)


def parse_v5(raw):
    """(flags, kcv, bitmap words, [(size, stored bytes)]) of a v5 file."""
    version, _, _, flags, _, n = struct.unpack_from("<IIIIQQ", raw, 8)
    marked, _, area = struct.unpack_from("<QIQ", raw, 40)
    assert raw[:8] == b"HSDELTA1" and version == 5
    at = 64 + (n + 63) // 64 * 8
    words = struct.unpack_from(f"<{(n + 63) // 64}Q", raw, 64)
    magic, kcv, zero, crc = struct.unpack_from("<4sIII", raw, at)
    assert (magic, zero, crc) == (b"HSKC", 0, hs.crc32c(raw[at:at + 12]))
    at += 16
    end, pieces = at + area, []
    while at < end:
        count, crc, payload, zero = struct.unpack_from("<IIII", raw, at)
        assert zero == 0 and crc == hs.crc32c(raw[at + 16:at + 16 + payload])
        sizes = struct.unpack_from(f"<{count}I", raw, at + 16)
        at += 16 + 4 * count
        for size in sizes:
            pieces.append((size, raw[at:at + max(size, 16)]))
            at += max(size, 16)
    assert at == end == len(raw) - 16 and len(pieces) == marked
    return flags, kcv, words, pieces


def twins(name, granule, n):
    """(base, vol) contents and bdevs; vol differs in three granules."""
    rng = random.Random(granule)
    base = rng.randbytes(n * granule)
    edits = {3: base[3 * granule:4 * granule - 1] + b"\xff",  # 11 bytes at 512
             7: periodic(granule, 69), n - 1: rng.randbytes(granule)}
    vol = bytearray(base)
    for g, x in edits.items():
        vol[g * granule:(g + 1) * granule] = x
    bdevs = [hs.create_malloc_bdev(f"{name}-{i}", granule, n) for i in (0, 1)]
    bdevs[0].write(0, base)
    bdevs[1].write(0, bytes(vol))
    return base, bytes(vol), bdevs[0], bdevs[1], sorted(edits)


@pytest.mark.parametrize("dictionary", [False, True])
def test_version_5_file(tmp_path, dictionary):
    granule, n = 512, 70
    base, vol, b_base, b_vol, changed = twins(f"v5{dictionary}", granule, n)
    path = str(tmp_path / "d.v5")
    info = hs.bdev_export_delta(b_vol, path, base=b_base, compress=True,
                                key=KEY, dictionary=dictionary, cts=True)
    raw = open(path, "rb").read()
    flags, kcv, words, pieces = parse_v5(raw)
    assert flags == (2 | 4 | (8 if dictionary else 0)) and kcv == xm.kcv(KEY)
    assert changed == [g for g in range(n) if words[g // 64] >> (g % 64) & 1]
    for g, (size, cipher) in zip(changed, pieces):
        d = base[g * granule:(g + 1) * granule] if dictionary else None
        assert len(cipher) == max(size, 16)
        plain = hs.xts_decrypt_var(cipher, KEY, unit=g)
        assert cipher == stored(KEY, g, plain[:size])  # the model agrees
        assert plain[size:] == bytes(len(plain) - size)
        assert hs.lz_decompress_granule(plain[:size], granule, dictionary=d) == \
            vol[g * granule:(g + 1) * granule]
    if dictionary:
        assert [size for size, _ in pieces][:2] == [11, 81]
    target = hs.create_malloc_bdev(f"v5t{dictionary}", granule, n)
    target.write(0, base)
    with pytest.raises(ValueError, match="wrong key"):
        hs.bdev_import_delta(target, path, key=KEY[::-1])
    assert hs.bdev_import_delta(target, path, dry_run=True)["marked"] == 3
    assert hs.bdev_import_delta(target, path, dry_run=True, key=KEY)
    assert target.read(0, len(base)) == base  # kcv and dry runs wrote nothing
    hs.bdev_import_delta(target, path, key=KEY)
    assert target.read(0, len(vol)) == vol
    # one flipped ciphertext byte: the record CRC, over the file as stored
    bad = bytearray(raw)
    bad[len(raw) - 16 - 100] ^= 1
    open(path, "wb").write(bad)
    with pytest.raises(ValueError, match="CRC mismatch"):
        hs.bdev_import_delta(target, path, dry_run=True)


@pytest.mark.parametrize("args", [dict(compress=True, cts=True),
                                  dict(key=KEY, cts=True)])
def test_cts_needs_key_and_compress(tmp_path, args):
    bdev = hs.create_malloc_bdev(f"cts-{len(args)}-{'key' in args}", 512, 8)
    with pytest.raises(ValueError, match="cts needs key and compress"):
        hs.bdev_export_delta(bdev, str(tmp_path / "x"), **args)
