"""hipstore::k_diff_granules / k_copy_marked on HBM bdevs.

Expected bitmaps come from a Python byte model (the set of granules the
test made different) and, for the same writes carried by two malloc
bdevs, from the generic host path. All ranges are validated on the host
before any launch."""

import random

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

BLOCK = 512
MAX_WGS = 2048
# More bitmap words than workgroups, twice over, plus a ragged tail:
# the grid-stride loop wraps and the last word is partial.
N = 2 * MAX_WGS * 64 + 65
FILL = 0x3C
POSITIONS = [0, 15, 16, BLOCK - 1]


def model_bitmap(n_granules, mismatching):
    """Little-endian bitmap bytes: granule g is byte g//8, bit g%8."""
    out = bytearray((n_granules + 7) // 8)
    for g in mismatching:
        assert 0 <= g < n_granules
        out[g // 8] |= 1 << (g % 8)
    return bytes(out)


def flipped_block(pos, fill=FILL):
    block = bytearray([fill]) * BLOCK
    block[pos] ^= 0xFF
    return bytes(block)


def plant(bdevs, granule, pos, fill=FILL):
    """One differing byte at `pos` of 512 B granule `granule`, in every
    bdev of `bdevs` (the HBM bdev and its malloc twin)."""
    for bdev in bdevs:
        bdev.write(granule * BLOCK, flipped_block(pos, fill))


@pytest.fixture(scope="module")
def planted():
    """HBM pair (a, b), malloc twins (ma, mb) carrying the same writes,
    and the model: the sorted granules where b differs from a. Shared
    and read-only: tests that write work on their own bdevs."""
    a = hs.create_hbm_bdev("dg-a", BLOCK, N, device=0)
    b = hs.create_hbm_bdev("dg-b", BLOCK, N, device=0)
    ma = hs.create_malloc_bdev("dg-ma", BLOCK, N)
    mb = hs.create_malloc_bdev("dg-mb", BLOCK, N)
    for bdev in (a, b, ma, mb):
        bdev.fill(0, FILL, N * BLOCK)
    rng = random.Random(20261)
    fixed = [0, 63, 64, 65, MAX_WGS * 64 - 1, MAX_WGS * 64, N - 1]
    granules = sorted(set(fixed) | set(rng.sample(range(N), 50)))
    pos = {g: POSITIONS[i % 4] for i, g in enumerate(granules)}
    for g in granules:
        plant((b, mb), g, pos[g])
    return {"a": a, "b": b, "ma": ma, "mb": mb, "granules": granules,
            "pos": pos}


@needs_gpu
class TestDiffKernel:
    def test_matches_model_and_generic_path(self, planted):
        want = planted["granules"]
        r = hs.bdev_diff(planted["a"], planted["b"], max_report=1024)
        assert r["granules"] == N
        assert r["mismatched"] == len(want)
        assert r["first_mismatches"] == want
        assert r["bitmap"] == model_bitmap(N, want)
        host = hs.bdev_diff(planted["ma"], planted["mb"], max_report=1024)
        assert r == host
        # a mixed pair (HBM vs malloc) takes the generic path
        mixed = hs.bdev_diff(planted["a"], planted["mb"], max_report=1024)
        assert mixed == host

    def test_coarse_granule(self, planted):
        n8 = N // 8
        want = sorted({g // 8 for g in planted["granules"] if g // 8 < n8})
        r = hs.bdev_diff(planted["a"], planted["b"], granule=4096,
                         max_report=1024)
        assert r["granules"] == n8
        assert r["first_mismatches"] == want
        assert r["bitmap"] == model_bitmap(n8, want)
        host = hs.bdev_diff(planted["ma"], planted["mb"], granule=4096,
                            max_report=1024)
        assert r == host

    @pytest.mark.parametrize("granule", [1024, 1536])
    def test_other_granules(self, planted, granule):
        """1 KiB is the first size that uses every lane once; 1536 B is
        no multiple of the 1 KiB a wave moves per step."""
        per = granule // BLOCK
        n = N // per
        want = sorted({g // per for g in planted["granules"] if g // per < n})
        r = hs.bdev_diff(planted["a"], planted["b"], granule=granule,
                         length=n * granule, max_report=1024)
        assert r["first_mismatches"] == want
        assert r["bitmap"] == model_bitmap(n, want)

    def test_shifted_offsets(self, planted):
        """a is uniform, so shifting a's window changes nothing; b's
        window starts 7 blocks in."""
        a_off, b_off = 3 * BLOCK, 7 * BLOCK
        n = N - 7
        want = [g - 7 for g in planted["granules"] if g >= 7]
        r = hs.bdev_diff(planted["a"], planted["b"], a_offset=a_off,
                         b_offset=b_off, length=n * BLOCK, max_report=1024)
        assert r["granules"] == n
        assert r["first_mismatches"] == want
        assert r["bitmap"] == model_bitmap(n, want)
        host = hs.bdev_diff(planted["ma"], planted["mb"], a_offset=a_off,
                            b_offset=b_off, length=n * BLOCK, max_report=1024)
        assert r == host

    def test_result_independent_of_scratch(self):
        """Every bit set, then a compare of identical ranges of the same
        size: the second bitmap is all zero, so no word is inherited."""
        n = 3 * 64 * 8 + 5
        x = hs.create_hbm_bdev("dg-x", BLOCK, n, device=0)
        y = hs.create_hbm_bdev("dg-y", BLOCK, n, device=0)
        y.fill(0, 0xFF, n * BLOCK)
        full = hs.bdev_diff(x, y, max_report=4)
        assert full["mismatched"] == n
        assert full["first_mismatches"] == [0, 1, 2, 3]
        assert full["bitmap"] == model_bitmap(n, range(n))  # tail bits 0
        y.fill(0, 0, n * BLOCK)
        same = hs.bdev_diff(x, y)
        assert same["mismatched"] == 0
        assert same["bitmap"] == bytes((n + 7) // 8)

    def test_tail_and_out_of_range(self):
        u = hs.create_hbm_bdev("dg-u", BLOCK, 128, device=0)
        v = hs.create_hbm_bdev("dg-v", BLOCK, 128, device=0)
        plant((v,), 65, 0, fill=0)
        plant((v,), 66, BLOCK - 1, fill=0)
        r = hs.bdev_diff(u, v, length=65 * BLOCK)
        assert r["granules"] == 65
        assert r["mismatched"] == 0
        assert r["first_mismatches"] == []
        assert r["bitmap"] == bytes(9)
        r = hs.bdev_diff(u, v, length=67 * BLOCK)
        assert r["first_mismatches"] == [65, 66]
        assert r["bitmap"] == model_bitmap(67, [65, 66])

    def test_rejected_before_launch(self, planted):
        a, b = planted["a"], planted["b"]
        for kwargs in ({"granule": 768}, {"a_offset": 100, "length": BLOCK},
                       {"length": (N + 1) * BLOCK},
                       {"a_offset": 2**64 - BLOCK, "length": 2 * BLOCK},
                       {"a_offset": N * BLOCK}):
            with pytest.raises(RuntimeError):
                hs.bdev_diff(a, b, **kwargs)


@needs_gpu
class TestCopyMarkedKernel:
    def test_subset_bitmap(self, planted):
        a, b = planted["a"], planted["b"]
        differing = planted["granules"]
        c = hs.create_hbm_bdev("dg-c", BLOCK, N, device=0)
        hs.hbm_copy(b, 0, c, 0, N * BLOCK)
        assert hs.bdev_diff(b, c)["mismatched"] == 0
        middle = differing[1:-1]
        marked = [0] + middle[::2] + [N - 1]
        left = middle[1::2]
        assert differing[0] == 0 and differing[-1] == N - 1
        # also mark two granules that do not differ: copied all the same
        extra = [g for g in (1000, MAX_WGS * 64 + 7) if g not in differing]
        bitmap = model_bitmap(N, marked + extra)
        assert hs.bdev_copy_marked(a, c, bitmap, BLOCK) == len(marked + extra)
        # marked granules now equal the source, unmarked differing ones
        # still differ
        r = hs.bdev_diff(a, c, max_report=1024)
        assert r["first_mismatches"] == left
        assert r["bitmap"] == model_bitmap(N, left)
        # nothing but the marked granules moved: against its old content
        # (b) the copy differs exactly where a differing granule was fixed
        r = hs.bdev_diff(b, c, max_report=1024)
        assert r["first_mismatches"] == marked
        # a still-differing granule and its neighbours, byte for byte
        g = left[len(left) // 2]
        want = b"".join(
            flipped_block(planted["pos"][h]) if h in left
            else bytes([FILL]) * BLOCK for h in (g - 1, g, g + 1))
        assert c.read((g - 1) * BLOCK, 3 * BLOCK) == want
        assert c.read(marked[1] * BLOCK, BLOCK) == bytes([FILL]) * BLOCK

    def test_stray_bits_past_the_range(self):
        """Bits at or past the last granule are neither copied nor
        counted: inside the last word (70, 71) and in a whole extra word
        of ones, with marks on both sides of the word boundary."""
        blocks, n = 192, 70
        src = hs.create_hbm_bdev("dg-stray-s", BLOCK, blocks, device=0)
        dst = hs.create_hbm_bdev("dg-stray-d", BLOCK, blocks, device=0)
        src.fill(0, 0x5A, src.size_bytes)
        dst.fill(0, 0xC3, dst.size_bytes)
        marked = [0, 63, 64, 69]
        bitmap = bytearray(model_bitmap(192, marked + [70, 71]))
        bitmap[16:24] = b"\xff" * 8
        copied = hs.bdev_copy_marked(src, dst, bytes(bitmap), BLOCK,
                                     length=n * BLOCK)
        assert copied == 4
        after = dst.read(0, blocks * BLOCK)
        for g in range(blocks):
            value = 0x5A if g in marked else 0xC3
            assert after[g * BLOCK:(g + 1) * BLOCK] == bytes([value]) * BLOCK, \
                f"granule {g}"

    def test_coarse_granule_with_offsets(self):
        granule = 4096
        src = hs.create_hbm_bdev("dg-s", BLOCK, 8 * 70, device=0)
        dst = hs.create_hbm_bdev("dg-d", BLOCK, 8 * 70, device=0)
        rng = random.Random(5)
        data = bytes(rng.getrandbits(8) for _ in range(66 * granule))
        src.write(2 * granule, data)
        marked = [0, 1, 63, 64, 65]
        hs.bdev_copy_marked(src, dst, model_bitmap(66, marked), granule,
                            src_offset=2 * granule, dst_offset=4 * granule,
                            length=66 * granule)
        got = dst.read(0, 70 * granule)
        want = bytearray(70 * granule)
        for g in marked:
            want[(4 + g) * granule:(5 + g) * granule] = \
                data[g * granule:(g + 1) * granule]
        assert got == bytes(want)
        with pytest.raises(RuntimeError):  # overlap within one store
            hs.bdev_copy_marked(src, src, b"\xff", granule, src_offset=0,
                                dst_offset=granule, length=2 * granule)


def diverge_and_scrub(children, name):
    blocks = 32768 + 65
    bdev = hs.create_replicated_bdev(name, children)
    rng = random.Random(23)
    payload = bytes(rng.getrandbits(8) for _ in range(64 * BLOCK))
    for off in (0, (blocks - 64) * BLOCK, 12345 * BLOCK):
        bdev.write(off, payload)
    clean = hs.replica_scrub(bdev)
    assert [r["child"] for r in clean["replicas"]] == [1]
    assert clean["replicas"][0]["granules"] == blocks
    assert clean["replicas"][0]["mismatched"] == 0
    stale = [0, 63, 64, 12345, blocks - 1]
    for blk in stale:
        children[1].write(blk * BLOCK, b"\xEE" * BLOCK)
    found = hs.replica_scrub(bdev)["replicas"][0]
    assert found["first_mismatches"] == stale and found["repaired"] == 0
    fixed = hs.replica_scrub(bdev, repair=True)["replicas"][0]
    assert fixed["mismatched"] == len(stale)
    assert fixed["repaired"] == len(stale)
    assert hs.replica_scrub(bdev)["replicas"][0]["mismatched"] == 0
    for off in (0, (blocks - 64) * BLOCK, 12345 * BLOCK):
        assert children[1].read(off, len(payload)) == payload
    assert children[1].read(64 * BLOCK, BLOCK) == bytes(BLOCK)


@needs_gpu
class TestReplicaScrubGpu:
    def test_same_device_children(self):
        children = [hs.create_hbm_bdev(f"dg-r{i}", BLOCK, 32768 + 65,
                                       device=0) for i in range(2)]
        diverge_and_scrub(children, "dg-r")

    @pytest.mark.skipif(hs.gpu_device_count() < 2,
                        reason="needs >=2 GPUs for the peer-access path")
    def test_cross_device_children(self):
        children = [hs.create_hbm_bdev(f"dg-p{i}", BLOCK, 32768 + 65,
                                       device=i) for i in range(2)]
        diverge_and_scrub(children, "dg-p")


@needs_gpu
class TestDiffDaemonHbm:
    def test_compare_clone(self, tmp_path):
        fixture = launch_hipstored(tmp_path, cpu=False)
        try:
            with hipstore.Client(fixture.socket_path) as client:
                hipstore.construct_malloc_bdev(
                    client, num_blocks=16384, block_size=4096, name="dgh")
                hipstore.bdev_clone(client, "dgh", "dgh-clone")
                info = hipstore.get_bdevs(client, "dgh-clone")[0]
                assert "hbm" in info.driver_specific
                r = hipstore.bdev_compare(client, "dgh", "dgh-clone")
                assert r["granules"] == 16384 and r["mismatched"] == 0
                perf = hipstore.perf_run(client, "dgh-clone",
                                         workload="randwrite", io_size=4096,
                                         queue_depth=4, num_queues=1,
                                         seconds=5.0, max_ios=32)
                assert perf["io_count"] >= 1
                r = hipstore.bdev_compare(client, "dgh", "dgh-clone",
                                          granule=4096, max_report=1024)
                assert 1 <= r["mismatched"] <= perf["io_count"]
                assert len(r["first_mismatches"]) == r["mismatched"]
        finally:
            fixture.stop()
