"""hipstore::k_xts_pack_marked / k_xts_unpack_marked on HBM bdevs, and
encrypted delta files of HBM volumes through the daemon.

The yardsticks are the pure-Python AES-256-XTS of xts_model.py and the
host codec on a malloc twin with the same content (the byte model)."""

import functools
import random

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

import xts_model
from fixtures import launch_hipstored
from test_delta import model_bitmap

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

BLOCK = 512
N = 64 * 2 + 7  # granules: two bitmap words and a ragged third
SENTINEL = 0xA5
KEY = bytes(range(64))


@functools.lru_cache(maxsize=None)
def content(n_bytes):
    return random.Random(n_bytes).randbytes(n_bytes)


@functools.lru_cache(maxsize=None)
def model_cipher(granule, first_unit):
    """Every granule of content(N * granule), encrypted by the model."""
    return xts_model.xts_encrypt_units(KEY, granule, content(N * granule),
                                       first_unit)


def twins(name, data):
    hbm = hs.create_hbm_bdev(f"{name}-h", BLOCK, len(data) // BLOCK, device=0)
    twin = hs.create_malloc_bdev(f"{name}-m", BLOCK, len(data) // BLOCK)
    for bdev in (hbm, twin):
        bdev.write(0, data)
    return hbm, twin


def check_round_trip(name, data, granule, marked, first_unit=0, staging=0,
                     model=None):
    """Pack on both paths, compare (with the model when given), then
    unpack on the GPU onto a sentinel volume."""
    n = len(data) // granule
    hbm, twin = twins(name, data)
    bitmap = model_bitmap(n, marked)
    dense = hs.bdev_xts_pack_marked(hbm, bitmap, granule, KEY, first_unit,
                                    staging_bytes=staging)
    assert dense == hs.bdev_xts_pack_marked(twin, bitmap, granule, KEY,
                                            first_unit, staging_bytes=staging)
    assert len(dense) == len(marked) * granule
    if model is not None:
        assert dense == b"".join(model[g * granule:(g + 1) * granule]
                                 for g in marked)
    hbm.write(0, bytes([SENTINEL]) * len(data))
    assert hs.bdev_xts_unpack_marked(hbm, bitmap, granule, dense, KEY,
                                     first_unit,
                                     staging_bytes=staging) == len(marked)
    want = bytearray([SENTINEL]) * len(data)
    for g in marked:
        want[g * granule:(g + 1) * granule] = data[g * granule:(g + 1) * granule]
    assert hbm.read(0, len(data)) == bytes(want)


@needs_gpu
@pytest.mark.parametrize("first_unit", [0, 2 ** 32 - 3])
@pytest.mark.parametrize("marks", ["all", "sparse", "none"])
@pytest.mark.parametrize("granule", [512, 1536, 4096])
def test_model_and_path_equality(granule, marks, first_unit):
    """Half a row of lanes, a row and a half, four rows."""
    marked = {"all": list(range(N)), "sparse": [0, 63, 64, 65, N - 1],
              "none": []}[marks]
    check_round_trip(f"xts{granule}{marks}{first_unit}", content(N * granule),
                     granule, marked, first_unit,
                     model=model_cipher(granule, first_unit))


@needs_gpu
@pytest.mark.parametrize("staging, marked", [
    (2 * 40 * 512, list(range(N))),   # boundaries at 40, 80 and 120
    (2 * 3 * 512, list(range(1, N, 2))),
], ids=["40", "3-odd"])
def test_windows_cut_inside_bitmap_words(staging, marked):
    check_round_trip(f"xtswin{staging}", content(N * 512), 512, marked,
                     staging=staging, model=model_cipher(512, 0))


@needs_gpu
def test_more_bitmap_words_than_workgroups():
    n = 2 * 2048 * 64 + 65
    marked = sorted(set(range(0, n, 97)) | {0, n - 1})
    check_round_trip("xtsgrid", content(n * 512), 512, marked)


@needs_gpu
def test_encrypted_export_import_through_the_daemon(tmp_path):
    granule, n = 4096, 300
    data = content(n * granule)
    twin = hs.create_malloc_bdev("xtsd-m", granule, n)
    twin.write(0, data)
    seed, want, got = (str(tmp_path / f) for f in ("seed.v1", "twin.v3",
                                                   "hbm.v3"))
    key_file, wrong_file = str(tmp_path / "key"), str(tmp_path / "wrong")
    open(key_file, "wb").write(KEY)
    open(wrong_file, "wb").write(KEY[::-1])
    hs.bdev_export_delta(twin, seed)
    hs.bdev_export_delta(twin, want, key=KEY)
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            for name in ("xtsd", "xtsd-new"):
                hipstore.construct_malloc_bdev(client, num_blocks=n,
                                               block_size=granule, name=name)
            assert "hbm" in hipstore.get_bdevs(client, "xtsd")[0].driver_specific
            hipstore.bdev_import_delta(client, "xtsd", seed)
            r = hipstore.bdev_export_delta(client, "xtsd", got,
                                           key_file=key_file)
            assert r["saved"] == n and r["full"] and r["encrypted"]
            assert open(got, "rb").read() == open(want, "rb").read()
            with pytest.raises(hipstore.RpcError):
                hipstore.bdev_import_delta(client, "xtsd-new", got,
                                           key_file=wrong_file)
            assert hipstore.bdev_import_delta(
                client, "xtsd-new", got, key_file=key_file)["applied"] == n
            assert hipstore.bdev_compare(
                client, "xtsd", "xtsd-new")["mismatched"] == 0
    finally:
        fixture.stop()
