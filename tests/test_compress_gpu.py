"""hipstore::k_lz_compress_marked / k_gather_var / k_lz_decompress_marked
on HBM bdevs, and compressed delta files of HBM volumes through the
daemon.

The yardsticks are the host codec on a malloc twin with the same content
(the byte model: sizes and bytes must be equal) and the plain LZ4 decoder
of test_compress.py against the source granules. Only streams that a
compress call produced reach a GPU call."""

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored
from test_compress import contents, stored_decode
from test_delta import model_bitmap

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

BLOCK = 512
N = 64 * 2 + 7  # granules: two bitmap words and a ragged third
SENTINEL = 0xA5


def class_bytes(granule, n):
    """n granules: the content classes of test_compress.py in turn."""
    classes = list(contents(granule).values())
    return b"".join(classes[i % len(classes)] for i in range(n))


def twins(name, granule, n):
    data = class_bytes(granule, n)
    hbm = hs.create_hbm_bdev(f"{name}-h", BLOCK, len(data) // BLOCK, device=0)
    twin = hs.create_malloc_bdev(f"{name}-m", BLOCK, len(data) // BLOCK)
    for bdev in (hbm, twin):
        bdev.write(0, data)
    return hbm, twin, data


def split(sizes, blob):
    out, at = [], 0
    for size in sizes:
        out.append(blob[at:at + size])
        at += size
    assert at == len(blob)
    return out


def check_round_trip(hbm, twin, data, granule, marked, staging=0):
    """Compress on both paths, compare, decode in Python, then decompress
    on the GPU onto a sentinel volume."""
    n = len(data) // granule
    bitmap = model_bitmap(n, marked)
    sizes, blob = hs.bdev_compress_marked(hbm, bitmap, granule,
                                          staging_bytes=staging)
    assert (sizes, blob) == hs.bdev_compress_marked(twin, bitmap, granule,
                                                    staging_bytes=staging)
    assert len(sizes) == len(marked)
    for g, piece in zip(marked, split(sizes, blob)):
        assert stored_decode(piece, granule) == \
            data[g * granule:(g + 1) * granule], g
    hbm_out = hs.create_hbm_bdev(f"lz-out{len(data)}-{len(marked)}-{staging}", BLOCK, len(data) // BLOCK, device=0)
    hbm_out.write(0, bytes([SENTINEL]) * len(data))
    assert hs.bdev_decompress_marked(hbm_out, bitmap, granule, sizes, blob,
                                     staging_bytes=staging) == len(marked)
    got = hbm_out.read(0, len(data))
    want = bytearray([SENTINEL]) * len(data)
    for g in marked:
        want[g * granule:(g + 1) * granule] = data[g * granule:(g + 1) * granule]
    assert got == bytes(want)


@needs_gpu
@pytest.mark.parametrize("granule", [512, 4096, 16384])
@pytest.mark.parametrize("marks", ["all", "sparse", "none"])
def test_model_and_path_equality(granule, marks):
    hbm, twin, data = twins(f"lz{granule}{marks}", granule, N)
    marked = {"all": list(range(N)), "sparse": [0, 63, 64, 65, N - 1],
              "none": []}[marks]
    check_round_trip(hbm, twin, data, granule, marked)


@needs_gpu
def test_windows_cut_inside_bitmap_words():
    """40 granules per window: boundaries at 40, 80 and 120."""
    hbm, twin, data = twins("lzwin", 512, N)
    check_round_trip(hbm, twin, data, 512, list(range(N)), staging=2 * 40 * 512)
    check_round_trip(hbm, twin, data, 512, list(range(1, N, 2)),
                     staging=2 * 3 * 512)


@needs_gpu
def test_more_bitmap_words_than_workgroups():
    n = 2 * 2048 * 64 + 65
    hbm, twin, data = twins("lzgrid", 512, n)
    marked = sorted(set(range(0, n, 97)) | {0, n - 1})
    check_round_trip(hbm, twin, data, 512, marked)


@needs_gpu
def test_compressed_export_import_through_the_daemon(tmp_path):
    granule, n = 4096, 300
    twin = hs.create_malloc_bdev("lzd-m", 4096, n)
    data = class_bytes(granule, n)
    twin.write(0, data)
    seed = str(tmp_path / "seed.v1")
    want = str(tmp_path / "twin.lz")
    got = str(tmp_path / "hbm.lz")
    hs.bdev_export_delta(twin, seed)
    model = hs.bdev_export_delta(twin, want, compress=True)
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            for name in ("lzd", "lzd-new"):
                hipstore.construct_malloc_bdev(client, num_blocks=n,
                                               block_size=4096, name=name)
            assert "hbm" in hipstore.get_bdevs(client, "lzd")[0].driver_specific
            hipstore.bdev_import_delta(client, "lzd", seed)
            r = hipstore.bdev_export_delta(client, "lzd", got, compress=True)
            assert r["saved"] == n and r["full"]
            assert r["stored_bytes"] == model["stored_bytes"] < n * granule
            assert open(got, "rb").read() == open(want, "rb").read()
            assert hipstore.bdev_import_delta(
                client, "lzd-new", got, dry_run=True)["applied"] == n
            assert hipstore.bdev_import_delta(
                client, "lzd-new", got)["applied"] == n
            assert hipstore.bdev_compare(
                client, "lzd", "lzd-new")["mismatched"] == 0
            # and the restored volume, uncompressed, is the seed again
            back = str(tmp_path / "back.v1")
            hipstore.bdev_export_delta(client, "lzd-new", back)
            assert open(back, "rb").read() == open(seed, "rb").read()
    finally:
        fixture.stop()
