"""hipstore::k_lzd_compress_marked / k_lzd_decompress_marked on HBM bdevs,
and version-4 delta files of HBM volumes through the daemon. The
yardsticks are the host codec on malloc twins (sizes and bytes must be
equal) and the decoder of test_dict_compress.py against the source. Only
streams that a compress call produced reach a GPU kernel."""
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore
from fixtures import launch_hipstored
from test_delta import model_bitmap
from test_dict_compress import N, dict_decode, volume

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")]

SPARSE = [0, 63, 64, 65, N - 1]
BIG = 2048 * 4 + 135  # more 512-byte granules than waves in the grid, 4 MiB
CASES = [(g, m, N, 0) for g in (512, 2048, 4096, 16384)
         for m in (list(range(N)), SPARSE, [])] + [
    (512, list(range(N)), N, 2 * 40 * 512),  # windows cut inside bitmap words
    (512, list(range(1, N, 2)), N, 2 * 3 * 512),
    (512, list(range(BIG)), BIG, 0)]


def round_trip(name, granule, marked, n=N, staging=0):
    """Both paths against each other, the decoder, and back onto D."""
    base, data = volume(granule, n)
    bdevs = {}
    for kind, create in (("h", lambda *a: hs.create_hbm_bdev(*a, device=0)),
                         ("m", hs.create_malloc_bdev)):
        for what, content in (("base", base), ("vol", data), ("out", base)):
            bdevs[what + kind] = create(f"{name}-{what}-{kind}", 512,
                                        len(data) // 512)
            bdevs[what + kind].write(0, content)
    bitmap = model_bitmap(n, marked)
    sizes, blob = hs.bdev_compress_marked(
        bdevs["volh"], bitmap, granule, staging_bytes=staging, base=bdevs["baseh"])
    assert (sizes, blob) == hs.bdev_compress_marked(
        bdevs["volm"], bitmap, granule, staging_bytes=staging, base=bdevs["basem"])
    want, at = bytearray(base), 0
    for g, size in zip(marked, sizes):
        span = slice(g * granule, (g + 1) * granule)
        assert dict_decode(blob[at:at + size], base[span])[0] == data[span], g
        want[span] = data[span]
        at += size
    assert at == len(blob) and len(sizes) == len(marked)
    for out in (bdevs["outh"], bdevs["outm"]):
        assert hs.bdev_decompress_marked(out, bitmap, granule, sizes, blob,
                                         staging_bytes=staging,
                                         dictionary=True) == len(marked)
        assert out.read(0, len(data)) == bytes(want)  # unmarked: still D
    return bdevs["outh"], bitmap, sizes, blob


@pytest.mark.parametrize("case", range(len(CASES)))
def test_model_and_path_equality(case):
    granule, marked, n, staging = CASES[case]
    round_trip(f"lzd{case}", granule, marked, n, staging)


def test_corrupt_piece_is_refused_on_the_host():
    """Granule 0 with an offset one past the dictionary: refused by the
    window's validation before a kernel runs, so nothing is written."""
    out, bitmap, sizes, blob = round_trip("lzdbad", 4096, SPARSE)
    base = volume(4096)[0]
    out.write(0, base)
    bad = blob[:1] + (4096 + 1).to_bytes(2, "little") + blob[3:]
    with pytest.raises(ValueError, match="granule 0: bad compressed piece"):
        hs.bdev_decompress_marked(out, bitmap, 4096, sizes, bad, dictionary=True)
    assert out.read(0, len(base)) == base


def test_version_4_export_import_through_the_daemon(tmp_path):
    granule = 4096
    twins, files = {}, {}
    for what, content in zip(("base", "vol"), volume(granule)):
        twins[what] = hs.create_malloc_bdev(f"lzdd-{what}", granule, N)
        twins[what].write(0, content)
        files[what] = str(tmp_path / f"{what}.v1")
        hs.bdev_export_delta(twins[what], files[what])
    want, got = str(tmp_path / "twin.v4"), str(tmp_path / "hbm.v4")
    model = hs.bdev_export_delta(twins["vol"], want, base=twins["base"],
                                 compress=True, dictionary=True)
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            for name in ("base", "vol", "new"):
                hipstore.construct_malloc_bdev(client, num_blocks=N,
                                               block_size=granule, name=name)
            assert "hbm" in hipstore.get_bdevs(client, "vol")[0].driver_specific
            for name in ("base", "vol"):
                hipstore.bdev_import_delta(client, name, files[name])
            r = hipstore.bdev_export_delta(client, "vol", got, base="base",
                                           compress=True, dictionary=True)
            assert r["dictionary"] and r["saved"] == model["marked"]
            assert open(got, "rb").read() == open(want, "rb").read()
            hipstore.bdev_import_delta(client, "new", files["base"])
            for dry_run, same in ((True, "base"), (False, "vol")):
                assert hipstore.bdev_import_delta(
                    client, "new", got, dry_run=dry_run)["applied"] == model["marked"]
                assert hipstore.bdev_compare(client, same, "new")["mismatched"] == 0
    finally:
        fixture.stop()
