"""hipstore::k_xts_var and the strict LZ decode on HBM bdevs: the keyed
marked calls against the Python model of test_crypt_compress.py and the
generic path on malloc twins, and version-5 files through the daemon."""
import functools
import random

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore
from fixtures import launch_hipstored
from test_crypt_compress import KEY, periodic, stored
from test_delta import model_bitmap

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")]

N = 70  # granules: one bitmap word and a ragged second
FIRST_UNIT = 1 << 33
# Period of the content -> stored size (asserted below): a multiple of 16;
# 1024 + b and 2048 + b, whose last pair of blocks straddles two rows of
# the wave; 1023; the largest compressed size; raw. Dictionary mode adds
# the unchanged granule, below 16 bytes at G = 512.
SIZES = {512: {68: 80, 69: 81, 244: 255, 500: 511, 512: 512},
         4096: {998: 1024, 1003: 1029, 997: 1023, 2027: 2053, 4066: 4094,
                4096: 4096},
         16384: {965: 1040, 954: 1029, 949: 1023, 14616: 16383, 16384: 16384}}
UNCHANGED = {512: 11, 4096: 25, 16384: 74}
MARKED = [1, 3, 4, 9, 63, 64, 69]  # gaps: the unit number is not the rank


@functools.lru_cache(maxsize=None)
def case(granule, dictionary):
    """(base, vol, sizes, the keyed stream the model expects)."""
    base = random.Random(granule).randbytes(N * granule)
    vol, sizes, stream = bytearray(base), [], b""
    periods = list(SIZES[granule]) + [None] * dictionary
    for g, period in zip(MARKED, periods):
        span = slice(g * granule, (g + 1) * granule)
        if period is not None:
            vol[span] = periodic(granule, period)
        piece = hs.lz_compress_granule(
            bytes(vol[span]), dictionary=base[span] if dictionary else None)
        assert len(piece) == (SIZES[granule][period] if period is not None
                              else UNCHANGED[granule])
        sizes.append(len(piece))
        cipher = stored(KEY, FIRST_UNIT + g, piece)
        stream += cipher + bytes(-len(cipher) % 16)
    return base, bytes(vol), sizes, stream


@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("granule", [512, 4096, 16384])
def test_keyed_stream_against_the_model(granule, dictionary):
    base, vol, sizes, stream = case(granule, dictionary)
    bitmap = model_bitmap(N, MARKED[:len(sizes)])
    staging = 2 * 3 * granule  # three pieces per window
    for kind, create in (("h", lambda *a: hs.create_hbm_bdev(*a, device=0)),
                         ("m", hs.create_malloc_bdev)):
        bdevs = {}
        for what, content in (("base", base), ("vol", vol), ("out", base)):
            bdevs[what] = create(f"cts{granule}{dictionary}-{what}-{kind}", 512,
                                 len(vol) // 512)
            bdevs[what].write(0, content)
        got = hs.bdev_compress_marked(
            bdevs["vol"], bitmap, granule, staging_bytes=staging, key=KEY,
            first_unit=FIRST_UNIT, base=bdevs["base"] if dictionary else None)
        assert got == (sizes, stream), kind  # pad bytes included
        assert hs.bdev_decompress_marked(
            bdevs["out"], bitmap, granule, sizes, stream, staging_bytes=staging,
            dictionary=dictionary, key=KEY,
            first_unit=FIRST_UNIT) == len(sizes)
        assert bdevs["out"].read(0, len(vol)) == vol, kind


# Legal LZ4 blocks of 512 bytes that break one end-of-block rule each: 4
# final literals after a match up to G - 4; a match that starts at G - 11.
CRAFTED = {
    "final": bytes([0x1F, 65, 1, 0, 255, 233, 0x40]) + b"BBBB",
    "start": bytes([0x1F, 65, 1, 0, 255, 225, 0x10, 66, 1, 0, 0x70]) + b"CCCCCCC",
}


@pytest.mark.parametrize("rule", sorted(CRAFTED))
def test_strict_decode_refuses_what_the_validator_refuses(rule):
    piece = CRAFTED[rule]
    assert not hs.lz_validate_granule(piece, 512)
    cipher = stored(KEY, 5, piece).ljust(32 if len(piece) > 16 else 16, b"\0")
    old = random.Random(5).randbytes(8 * 512)
    for kind, create in (("h", lambda *a: hs.create_hbm_bdev(*a, device=0)),
                         ("m", hs.create_malloc_bdev)):
        out = create(f"strict-{rule}-{kind}", 512, 8)
        out.write(0, old)
        with pytest.raises(ValueError, match="granule 5: bad compressed piece"):
            hs.bdev_decompress_marked(out, model_bitmap(8, [5]), 512,
                                      [len(piece)], cipher, key=KEY)
        assert out.read(0, len(old)) == old, kind


def test_version_5_files_through_the_daemon(tmp_path):
    granule = 4096
    base, vol, sizes, _ = case(granule, True)
    files = {}
    for what, content in (("base", base), ("vol", vol)):
        twin = hs.create_malloc_bdev(f"ctsd-{what}", granule, N)
        twin.write(0, content)
        files[what] = str(tmp_path / f"{what}.v1")
        hs.bdev_export_delta(twin, files[what])
    key_file = str(tmp_path / "key")
    open(key_file, "wb").write(KEY)
    full, inc, map0, map1 = (str(tmp_path / f) for f in
                             ("full.v5", "inc.v5", "map0", "map1"))
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            for name in ("vol", "new"):
                hipstore.construct_malloc_bdev(client, num_blocks=N,
                                               block_size=granule, name=name)
            assert "hbm" in hipstore.get_bdevs(client, "vol")[0].driver_specific
            hipstore.bdev_import_delta(client, "vol", files["base"])
            r = hipstore.bdev_export_delta(
                client, "vol", full, compress=True, key_file=key_file, cts=True,
                map_out=map0)
            assert r["encrypted"] and r["saved"] == N
            hipstore.bdev_clone(client, "vol", "base")
            hipstore.bdev_import_delta(client, "vol", files["vol"])
            r = hipstore.bdev_export_delta(
                client, "vol", inc, base="base", compress=True, dictionary=True,
                key_file=key_file, cts=True, map_out=map1)
            # the unchanged marked granule of case() is not in a diff
            assert r["dictionary"] and r["saved"] == len(sizes) - 1
            assert r["stored_bytes"] == sum(sizes[:-1])
            for path, map_path in ((full, map0), (inc, map1)):
                hipstore.bdev_import_delta(client, "new", path,
                                           key_file=key_file)
                assert hipstore.bdev_verify_fingerprints(
                    client, "new", map_path)["mismatched"] == 0
            assert hipstore.bdev_compare(client, "vol", "new")["mismatched"] == 0
    finally:
        fixture.stop()
