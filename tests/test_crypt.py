"""HSXTS1 (AES-256-XTS) on the host: the codec against known answers and
the pure-Python model of xts_model.py, and encrypted (version-3) delta
files on malloc bdevs. The GPU kernels are in test_crypt_gpu.py."""

import struct

import pytest

from oim_amd import _hipstore as hs

import xts_model
from test_delta import (build_delta_file, indexed_bytes, model_bitmap,
                        refresh_header_crc)

KEY = bytes(range(64))
OTHER_KEY = bytes(range(1, 65))

# Produced with OpenSSL 3.0.2, EVP_aes_256_xts, key KEY, IV = the unit
# number as a little-endian u64 followed by eight zero bytes.
XTS_48 = (5, bytes(range(48)), bytes.fromhex(
    "f87ca2f29b117c1b024a6ec8e8c5994e76f7d16b43eed21e6936126969e00dab"
    "9d57dfb999d8d20535e3b2b7a51fab52"))
XTS_512 = (2 ** 32 + 7, bytes((7 * i + 3) & 0xFF for i in range(512)),
           bytes.fromhex(
    "b348269158ee5a4acda0bfb5005a3b8e60032e2fd0abe371e5a52e8cf6a8cf70"
    "7faf3a830ede7cc26193b1bb59020038082110e5de12eb67dd6142783c10a59b"
    "c75b6d93e188f685192dd4b710e586710d84d279868f1d0034999b701ae21ffa"
    "7035ecbd2f0504dd3d8457cba4d76144065fc6ad3a7a39e40392fcb8cfa49d9b"
    "23298550699ddc0fd145722b438a655e4d445a6b808c9071a06d41d3bd4abadb"
    "e436ce7149e244a7782d3f1a5b49167b699a27e617b7c2dc8eeba68daefea8e2"
    "6830c5b93a8aabf2a784cd5f52f2d1add49f5d33ee6c30784f044eb775d934bd"
    "17badf94de86e28345b071281779c2f8c2a895054e90042e960719df9862036b"
    "ba1d691ab4e863bc2c3d152e509a264ba43bbdd54f55b47bd672140dbe47802a"
    "5bc8cd675083a7bd962a700fbc4272de4877e1da1f65044e43470fda2d7f45fa"
    "4d30354b2aaae0da51d0b8952d3fb4cff6d894f1347a94ab58e146a99efcbfee"
    "4721363ee026be9376b817e268ffb4ca257a42f250ff40facabfb15a640a7cc0"
    "58d424bef5eb22492002290c139346505e81368fcb1dd559d8cba0b24b85d8bd"
    "619085d372f1b84f6aca8052e0af48d23171b649f4e80684bc72c2ad0d1f0c1b"
    "3181b957cf6122d54b9516ddd01a0a3676595ed06bf641a72b4e1488a85ee9b0"
    "24cd2c424dcfbdfa02146c6606fb1229fd138aae57a55448701f58144921bcb7"))


def test_model_block_is_fips_197_c3():
    block = xts_model.encrypt_block(
        xts_model.expand(bytes(range(32))),
        bytes.fromhex("00112233445566778899aabbccddeeff"))
    assert block.hex() == "8ea2b7ca516745bfeafc49904b496089"


@pytest.mark.parametrize("vector", [XTS_48, XTS_512], ids=["48", "512"])
def test_known_answers(vector):
    unit, plain, cipher = vector
    assert xts_model.xts_encrypt(KEY, unit, plain) == cipher
    assert hs.xts_encrypt_units(plain, len(plain), KEY, unit) == cipher
    assert hs.xts_decrypt_units(cipher, len(plain), KEY, unit) == plain


@pytest.mark.parametrize("first_unit", [0, 2 ** 32 - 2])
@pytest.mark.parametrize("granule", [16, 512, 1536])
def test_host_codec_equals_model(granule, first_unit):
    data = indexed_bytes(9, salt=granule)[:3 * granule]
    cipher = hs.xts_encrypt_units(data, granule, KEY, first_unit)
    assert cipher == xts_model.xts_encrypt_units(KEY, granule, data, first_unit)
    assert hs.xts_decrypt_units(cipher, granule, KEY, first_unit) == data
    assert hs.xts_kcv(KEY) == xts_model.kcv(KEY) != hs.xts_kcv(OTHER_KEY)


# --- version-3 files on a malloc bdev ---------------------------------------

BLOCK = 512
N = 64 + 9  # a ragged second bitmap word
CHANGED = [0, 1, 63, 64, N - 1]


def as_version_3(blob, key):
    """A version-1 file of ciphertext with the three header differences."""
    blob = bytearray(blob)
    flags, = struct.unpack_from("<I", blob, 20)
    struct.pack_into("<I", blob, 8, 3)
    struct.pack_into("<I", blob, 20, flags | 4)
    struct.pack_into("<I", blob, 52, xts_model.kcv(key))
    return refresh_header_crc(bytes(blob))


@pytest.fixture(scope="module")
def volumes():
    """(bdev, its bytes, their ciphertext, base bdev): the base differs
    from the volume in the granules CHANGED."""
    data = indexed_bytes(N)
    old = bytearray(data)
    for g in CHANGED:
        old[g * BLOCK] ^= 0xFF
    src = hs.create_malloc_bdev("xts-src", BLOCK, N)
    base = hs.create_malloc_bdev("xts-base", BLOCK, N)
    src.write(0, data)
    base.write(0, bytes(old))
    return src, data, xts_model.xts_encrypt_units(KEY, BLOCK, data), base


@pytest.mark.parametrize("marked", [None, CHANGED], ids=["full", "delta"])
def test_export_is_the_model_file_and_import_restores(volumes, tmp_path,
                                                      marked):
    src, data, cipher, base = volumes
    path = str(tmp_path / "v3")
    info = hs.bdev_export_delta(src, path, key=KEY,
                                base=None if marked is None else base)
    assert (info["version"], info["encrypted"]) == (3, True)
    assert open(path, "rb").read() == as_version_3(
        build_delta_file(cipher, BLOCK, marked), KEY)
    assert hs.delta_file_info(path)["encrypted"] is True
    # A keyless dry run vets the file; the import needs the key.
    dst = hs.create_malloc_bdev(f"xts-dst{marked is None}", BLOCK, N)
    dst.write(0, base.read(0, len(data)))
    assert hs.bdev_import_delta(dst, path, dry_run=True)["marked"] == \
        info["marked"]
    assert hs.bdev_import_delta(dst, path, dry_run=True, key=KEY)
    assert dst.read(0, len(data)) == base.read(0, len(data))
    hs.bdev_import_delta(dst, path, key=KEY)
    assert dst.read(0, len(data)) == data


def test_version_1_export_is_unchanged(volumes, tmp_path):
    src, data, _, _ = volumes
    path = str(tmp_path / "v1")
    info = hs.bdev_export_delta(src, path)
    assert open(path, "rb").read() == build_delta_file(data, BLOCK)
    assert "encrypted" not in info
    assert "encrypted" not in hs.delta_file_info(path)


@pytest.mark.parametrize("kwargs", [
    {"key": bytes(32) * 2}, {"key": KEY[:63]}, {"key": KEY, "compress": True},
], ids=["equal-halves", "63-bytes", "with-compress"])
def test_export_refusals(volumes, tmp_path, kwargs):
    with pytest.raises(ValueError):
        hs.bdev_export_delta(volumes[0], str(tmp_path / "no"), **kwargs)
    assert not (tmp_path / "no").exists()


def test_import_refusals_leave_the_target_alone(volumes, tmp_path):
    src, data, _, _ = volumes
    v1, v3 = str(tmp_path / "v1"), str(tmp_path / "v3")
    hs.bdev_export_delta(src, v1)
    hs.bdev_export_delta(src, v3, key=KEY)
    before = bytes([0x5A]) * len(data)
    dst = hs.create_malloc_bdev("xts-refuse", BLOCK, N)
    dst.write(0, before)
    for path, key in [(v3, None), (v1, KEY), (v3, OTHER_KEY), (v3, KEY[:63])]:
        with pytest.raises(ValueError):
            hs.bdev_import_delta(dst, path, key=key)
        assert dst.read(0, len(data)) == before
    with pytest.raises(ValueError):
        hs.bdev_import_delta(dst, v3, dry_run=True, key=OTHER_KEY)


def test_marked_calls_on_a_malloc_bdev(volumes):
    src, data, cipher, _ = volumes
    bitmap = model_bitmap(N, CHANGED)
    first = 2 ** 32 - 2
    want = b"".join(
        xts_model.xts_encrypt(KEY, first + g, data[g * BLOCK:(g + 1) * BLOCK])
        for g in CHANGED)
    assert hs.bdev_xts_pack_marked(src, bitmap, BLOCK, KEY, first) == want
    dst = hs.create_malloc_bdev("xts-marked", BLOCK, N)
    assert hs.bdev_xts_unpack_marked(dst, bitmap, BLOCK, want, KEY,
                                     first) == len(CHANGED)
    for g in range(N):
        got = dst.read(g * BLOCK, BLOCK)
        assert got == (data[g * BLOCK:(g + 1) * BLOCK] if g in CHANGED
                       else bytes(BLOCK)), g
    with pytest.raises(ValueError):  # a granule would carry the kcv's number
        hs.bdev_xts_pack_marked(src, bitmap, BLOCK, KEY, 2 ** 64 - N)
