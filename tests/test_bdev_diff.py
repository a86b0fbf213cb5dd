"""Granule compare, marked copy and replica scrub on the generic
(host) path and through the daemon's RPC plane.

The expected bitmap always comes from a byte model the test keeps
itself: the set of granules it made different. The GPU kernels are
checked against the same model (and against this path) in
test_bdev_diff_gpu.py."""

import itertools

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import hipstored  # noqa: F401

BLOCK = 512
_seq = itertools.count()


def model_bitmap(n_granules, mismatching):
    """Little-endian bitmap bytes: granule g is byte g//8, bit g%8."""
    out = bytearray((n_granules + 7) // 8)
    for g in mismatching:
        assert 0 <= g < n_granules
        out[g // 8] |= 1 << (g % 8)
    return bytes(out)


def make_pair(blocks, fill=0xA5):
    """Two malloc bdevs with identical content."""
    tag = next(_seq)
    a = hs.create_malloc_bdev(f"diff-a-{tag}", BLOCK, blocks)
    b = hs.create_malloc_bdev(f"diff-b-{tag}", BLOCK, blocks)
    a.fill(0, fill, a.size_bytes)
    b.fill(0, fill, b.size_bytes)
    return a, b


def flip_byte(bdev, byte_offset):
    """Changes exactly one byte of a bdev (read-modify-write a block)."""
    base = byte_offset // BLOCK * BLOCK
    block = bytearray(bdev.read(base, BLOCK))
    block[byte_offset - base] ^= 0xFF
    bdev.write(base, bytes(block))


class TestDiffGeneric:
    @pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
    def test_granule_counts_and_word_boundaries(self, n):
        """Differences at granule 0, the last granule and on both sides
        of each word boundary, the differing byte at 0, 15, 16 and
        granule-1 of its granule."""
        a, b = make_pair(n + 4)
        wanted = {0, n - 1, 63, 64, 127, 128}
        planted = sorted(g for g in wanted if g < n)
        positions = [0, 15, 16, BLOCK - 1]
        for i, g in enumerate(planted):
            flip_byte(b, g * BLOCK + positions[i % 4])
        # just outside the compared range: no report, no tail bit
        flip_byte(b, n * BLOCK)
        r = hs.bdev_diff(a, b, length=n * BLOCK, max_report=1024)
        assert r["granules"] == n
        assert r["mismatched"] == len(planted)
        assert r["first_mismatches"] == planted
        assert r["bitmap"] == model_bitmap(n, planted)

    @pytest.mark.parametrize("pos", [0, 15, 16, BLOCK - 1])
    def test_every_byte_position_counts(self, pos):
        a, b = make_pair(8)
        flip_byte(a, 5 * BLOCK + pos)
        r = hs.bdev_diff(a, b)
        assert r["granules"] == 8
        assert r["first_mismatches"] == [5]
        assert r["bitmap"] == model_bitmap(8, [5])

    def test_identical_ranges(self):
        a, b = make_pair(130)
        r = hs.bdev_diff(a, b)
        assert r["granules"] == 130
        assert r["mismatched"] == 0
        assert r["first_mismatches"] == []
        assert r["bitmap"] == bytes((130 + 7) // 8)

    def test_unequal_offsets(self):
        a, b = make_pair(96)
        a_off, b_off, n = 3 * BLOCK, 7 * BLOCK, 70
        # make the two windows equal first: b's window is a's, shifted
        for bdev in (a, b):
            bdev.fill(0, 0, bdev.size_bytes)
        payload = bytes((i * 7 + i // BLOCK) & 0xFF for i in range(n * BLOCK))
        a.write(a_off, payload)
        b.write(b_off, payload)
        assert hs.bdev_diff(a, b, a_offset=a_off, b_offset=b_off,
                            length=n * BLOCK)["mismatched"] == 0
        planted = [0, 1, 63, 64, 69]
        for g in planted:
            flip_byte(b, b_off + g * BLOCK + 16)
        # one block before and one after b's window
        flip_byte(b, b_off - 1)
        flip_byte(b, b_off + n * BLOCK)
        r = hs.bdev_diff(a, b, a_offset=a_off, b_offset=b_off,
                         length=n * BLOCK, max_report=64)
        assert r["first_mismatches"] == planted
        assert r["bitmap"] == model_bitmap(n, planted)

    def test_coarse_granule_on_small_blocks(self):
        granule = 4096
        a, b = make_pair(8 * 66)  # 66 granules of 8 blocks
        flips = [0, 4095, 4096 + 15, 63 * 4096 + 16, 64 * 4096, 65 * 4096 + 4095]
        for off in flips:
            flip_byte(b, off)
        flip_byte(b, 64 * 4096 + 700)  # second hit in granule 64
        planted = sorted({off // granule for off in flips})
        r = hs.bdev_diff(a, b, granule=granule, max_report=64)
        assert r["granules"] == 66
        assert r["mismatched"] == len(planted)
        assert r["first_mismatches"] == planted
        assert r["bitmap"] == model_bitmap(66, planted)

    def test_report_is_ascending_and_truncated(self):
        a, b = make_pair(200)
        planted = list(range(3, 200, 5))
        for g in reversed(planted):
            flip_byte(a, g * BLOCK + g % BLOCK)
        r = hs.bdev_diff(a, b, max_report=7)
        assert r["first_mismatches"] == planted[:7]
        assert r["mismatched"] == len(planted)
        assert r["bitmap"] == model_bitmap(200, planted)
        assert hs.bdev_diff(a, b, max_report=0)["first_mismatches"] == []

    def test_range_longer_than_one_host_chunk(self):
        """The host path reads at most 1 MiB per side at a time; a
        3 MiB + 1 block range crosses chunk boundaries."""
        blocks = 3 * 2048 + 1
        a, b = make_pair(blocks, fill=0)
        planted = [0, 2047, 2048, 4096, blocks - 1]
        for g in planted:
            flip_byte(b, g * BLOCK + BLOCK - 1)
        r = hs.bdev_diff(a, b)
        assert r["granules"] == blocks
        assert r["first_mismatches"] == planted
        assert r["bitmap"] == model_bitmap(blocks, planted)


class TestDiffValidation:
    def rejects(self, *args, **kwargs):
        with pytest.raises(RuntimeError):
            hs.bdev_diff(*args, **kwargs)

    def test_bad_granule(self):
        a, b = make_pair(64)
        self.rejects(a, b, granule=768)    # not a block multiple
        self.rejects(a, b, granule=16)     # multiple of 16, not of the block
        odd_a = hs.create_malloc_bdev(f"diff-odd-{next(_seq)}", 520, 64)
        odd_b = hs.create_malloc_bdev(f"diff-odd-{next(_seq)}", 520, 64)
        self.rejects(odd_a, odd_b, granule=520)  # block multiple, not of 16
        assert hs.bdev_diff(odd_a, odd_b, granule=1040)["granules"] == 32

    def test_misaligned_offset_and_length(self):
        a, b = make_pair(64)
        self.rejects(a, b, a_offset=BLOCK, granule=4096, length=4096)
        self.rejects(a, b, b_offset=BLOCK, granule=4096, length=4096)
        self.rejects(a, b, a_offset=100, length=BLOCK)
        self.rejects(a, b, granule=4096, length=4096 + BLOCK)

    def test_zero_length(self):
        """An offset at the very end leaves nothing to compare: the
        derived length is 0, which the engine rejects."""
        a, b = make_pair(64)
        self.rejects(a, b, a_offset=a.size_bytes)
        self.rejects(a, b, granule=a.size_bytes * 2)

    def test_out_of_bounds(self):
        a, b = make_pair(64)
        small = hs.create_malloc_bdev(f"diff-small-{next(_seq)}", BLOCK, 32)
        self.rejects(a, b, length=65 * BLOCK)
        self.rejects(a, b, a_offset=BLOCK, length=64 * BLOCK)
        self.rejects(a, b, b_offset=63 * BLOCK, length=2 * BLOCK)
        self.rejects(a, small, length=33 * BLOCK)
        self.rejects(a, b, a_offset=65 * BLOCK)

    def test_wrapping_offsets(self):
        """offset + length wraps to a small number: still out of bounds."""
        a, b = make_pair(64)
        near_top = 2**64 - BLOCK
        self.rejects(a, b, a_offset=near_top, length=2 * BLOCK)
        self.rejects(a, b, b_offset=near_top, length=2 * BLOCK)
        self.rejects(a, b, a_offset=near_top, b_offset=near_top, length=BLOCK)
        with pytest.raises(RuntimeError):
            hs.bdev_copy_marked(a, b, b"\x01", BLOCK, src_offset=near_top,
                                length=2 * BLOCK)

    def test_mismatched_block_sizes(self):
        a = hs.create_malloc_bdev(f"diff-bs-{next(_seq)}", 512, 64)
        b = hs.create_malloc_bdev(f"diff-bs-{next(_seq)}", 4096, 8)
        self.rejects(a, b, granule=4096)
        with pytest.raises(RuntimeError):
            hs.bdev_copy_marked(a, b, b"\xff", 4096)


class TestCopyMarked:
    def test_subset_bitmap(self):
        n = 130
        src, dst = make_pair(n, fill=0x11)
        differing = [0, 1, 5, 63, 64, 65, 100, 129]
        for g in differing:
            flip_byte(dst, g * BLOCK + (g % 4) * 5)
        marked = [0, 5, 64, 129]
        before = dst.read(0, n * BLOCK)
        copied = hs.bdev_copy_marked(src, dst, model_bitmap(n, marked), BLOCK)
        assert copied == len(marked)
        after = dst.read(0, n * BLOCK)
        want = src.read(0, n * BLOCK)
        for g in range(n):
            sl = slice(g * BLOCK, (g + 1) * BLOCK)
            if g in marked:
                assert after[sl] == want[sl], f"marked granule {g}"
            else:
                # unmarked: untouched, so differing ones still differ
                assert after[sl] == before[sl], f"unmarked granule {g}"
        left = sorted(set(differing) - set(marked))
        r = hs.bdev_diff(src, dst, max_report=64)
        assert r["first_mismatches"] == left

    def test_marked_but_equal_and_offsets(self):
        """Marking is the caller's business: a marked granule is copied
        whether it differs or not; offsets shift both windows."""
        src, dst = make_pair(64, fill=0)
        src.write(8 * BLOCK, bytes(range(256)) * 8)  # granules 2 (4 blocks)
        copied = hs.bdev_copy_marked(src, dst, b"\x06", 4 * BLOCK,
                                     src_offset=0, dst_offset=16 * BLOCK,
                                     length=12 * BLOCK)
        assert copied == 2
        assert dst.read(24 * BLOCK, 4 * BLOCK) == src.read(8 * BLOCK, 4 * BLOCK)
        assert dst.read(0, 24 * BLOCK) == bytes(24 * BLOCK)
        assert dst.read(28 * BLOCK, 36 * BLOCK) == bytes(36 * BLOCK)

    def test_diff_bitmap_round_trip(self):
        src, dst = make_pair(200)
        for g in (0, 7, 8, 64, 199):
            flip_byte(dst, g * BLOCK + 3)
        r = hs.bdev_diff(src, dst)
        assert hs.bdev_copy_marked(src, dst, r["bitmap"], BLOCK) == 5
        assert hs.bdev_diff(src, dst)["mismatched"] == 0

    def test_stray_bits_past_the_range(self):
        """Bits at or past the last granule are neither copied nor
        counted: inside the last word (70, 71) and in a whole extra word
        of ones, with marks on both sides of the word boundary."""
        blocks, n = 192, 70
        tag = next(_seq)
        src = hs.create_malloc_bdev(f"stray-s-{tag}", BLOCK, blocks)
        dst = hs.create_malloc_bdev(f"stray-d-{tag}", BLOCK, blocks)
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

    def test_validation(self):
        src, dst = make_pair(64)
        with pytest.raises(RuntimeError):  # bitmap shorter than the range
            hs.bdev_copy_marked(src, dst, b"\xff" * 7, BLOCK)
        with pytest.raises(RuntimeError):  # overlapping ranges, one store
            hs.bdev_copy_marked(src, src, b"\xff", BLOCK, src_offset=0,
                                dst_offset=4 * BLOCK, length=8 * BLOCK)
        with pytest.raises(RuntimeError):
            hs.bdev_copy_marked(src, dst, b"\xff", 100)
        # disjoint ranges of one bdev are fine
        flip_byte(src, 0)
        assert hs.bdev_copy_marked(src, src, b"\x01", BLOCK, src_offset=0,
                                   dst_offset=8 * BLOCK, length=8 * BLOCK) == 1
        assert src.read(8 * BLOCK, BLOCK) == src.read(0, BLOCK)


class TestReplicaScrub:
    def make_replicated(self, n=3, blocks=256):
        tag = next(_seq)
        children = [hs.create_malloc_bdev(f"scrub-{tag}-{i}", BLOCK, blocks)
                    for i in range(n)]
        return hs.create_replicated_bdev(f"scrub-{tag}", children), children

    def test_detect_repair_rescrub(self):
        bdev, children = self.make_replicated()
        payload = bytes((i * 13 + i // BLOCK) & 0xFF for i in range(256 * BLOCK))
        bdev.write(0, payload)
        clean = hs.replica_scrub(bdev)
        assert clean["granule"] == BLOCK
        assert [r["child"] for r in clean["replicas"]] == [1, 2]
        assert all(r["granules"] == 256 and r["mismatched"] == 0
                   for r in clean["replicas"])
        # diverge the replicas behind the parent's back
        stale = {1: [0, 63, 64, 255], 2: [17]}
        for child, blocks in stale.items():
            for blk in blocks:
                children[child].write(blk * BLOCK, b"\xEE" * BLOCK)
        found = hs.replica_scrub(bdev, max_report=64)
        for rep in found["replicas"]:
            assert rep["first_mismatches"] == stale[rep["child"]]
            assert rep["mismatched"] == len(stale[rep["child"]])
            assert rep["repaired"] == 0
        fixed = hs.replica_scrub(bdev, repair=True)
        assert [r["repaired"] for r in fixed["replicas"]] == [4, 1]
        again = hs.replica_scrub(bdev)
        assert all(r["mismatched"] == 0 for r in again["replicas"])
        for child in children:
            assert child.read(0, 256 * BLOCK) == payload

    def test_coarse_granule(self):
        bdev, children = self.make_replicated(n=2)
        children[1].write(9 * BLOCK, b"\x01" * BLOCK)
        r = hs.replica_scrub(bdev, granule=4096)
        assert r["granule"] == 4096
        assert r["replicas"][0]["granules"] == 32
        assert r["replicas"][0]["first_mismatches"] == [1]
        with pytest.raises(RuntimeError):
            hs.replica_scrub(bdev, granule=100)

    def test_not_replicated(self):
        children = [hs.create_malloc_bdev(f"scrub-s-{next(_seq)}", BLOCK, 64)
                    for _ in range(2)]
        striped = hs.create_striped_bdev(f"scrub-st-{next(_seq)}", children,
                                         4096)
        with pytest.raises(RuntimeError):
            hs.replica_scrub(striped)
        with pytest.raises(RuntimeError):
            hs.replica_scrub(children[0])


class TestDiffRpc:
    def test_compare_clone_then_diverge(self, hipstored):  # noqa: F811
        with hipstore.Client(hipstored.socket_path) as client:
            hipstore.construct_malloc_bdev(client, 2048, 512, name="cmp-src")
            hipstore.bdev_clone(client, "cmp-src", "cmp-clone")
            r = hipstore.bdev_compare(client, "cmp-src", "cmp-clone")
            assert r == {"granule": 512, "granules": 2048, "mismatched": 0,
                         "first_mismatches": []}
            # perf writes carry 0x5A over the zero-initialised clone
            perf = hipstore.perf_run(client, "cmp-clone",
                                     workload="randwrite", io_size=4096,
                                     queue_depth=4, num_queues=1,
                                     seconds=5.0, max_ios=16)
            assert perf["io_count"] >= 1
            r = hipstore.bdev_compare(client, "cmp-src", "cmp-clone",
                                      granule=4096, max_report=1024)
            assert r["granule"] == 4096 and r["granules"] == 256
            assert 1 <= r["mismatched"] <= perf["io_count"]
            assert len(r["first_mismatches"]) == r["mismatched"]
            assert r["first_mismatches"] == sorted(set(r["first_mismatches"]))
            capped = hipstore.bdev_compare(client, "cmp-src", "cmp-clone",
                                           granule=4096, max_report=1)
            assert capped["first_mismatches"] == r["first_mismatches"][:1]
            assert capped["mismatched"] == r["mismatched"]
            # explicit window with offsets: the same data, shifted
            w = hipstore.bdev_compare(client, "cmp-src", "cmp-src",
                                      a_offset=4096, b_offset=8192,
                                      length=8192, granule=4096)
            assert w["granules"] == 2 and w["mismatched"] == 0

    def test_compare_errors(self, hipstored):  # noqa: F811
        with hipstore.Client(hipstored.socket_path) as client:
            hipstore.construct_malloc_bdev(client, 64, 512, name="e-a")
            hipstore.construct_malloc_bdev(client, 8, 4096, name="e-b")
            hipstore.construct_malloc_bdev(client, 64, 512, name="e-c")
            bad = [
                {"a": "nope", "b": "e-a"},
                {"a": "e-a", "b": "nope"},
                {"a": "e-a"},
                {"a": "e-a", "b": "e-b"},                    # block sizes
                {"a": "e-a", "b": "e-c", "granule": 100},
                {"a": "e-a", "b": "e-c", "granule": -512},
                {"a": "e-a", "b": "e-c", "a_offset": 100},
                {"a": "e-a", "b": "e-c", "a_offset": -512},
                {"a": "e-a", "b": "e-c", "length": 0},
                {"a": "e-a", "b": "e-c", "length": 65 * 512},
                {"a": "e-a", "b": "e-c", "a_offset": 64 * 512},
                {"a": "e-a", "b": "e-c", "b_offset": 2**63 - 512,
                 "length": 1024},
                {"a": "e-a", "b": "e-c", "max_report": -1},
            ]
            for params in bad:
                with pytest.raises(hipstore.RpcError) as err:
                    client.invoke("bdev_compare", params)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS, params
            big = client.invoke("bdev_compare", {"a": "e-a", "b": "e-c",
                                                 "max_report": 10**6})
            assert big["granules"] == 64
            methods = client.invoke("get_rpc_methods")
            assert "bdev_compare" in methods
            assert "bdev_replica_scrub" in methods

    def test_replica_scrub_rpc(self, hipstored):  # noqa: F811
        with hipstore.Client(hipstored.socket_path) as client:
            hipstore.construct_replicated_malloc_bdev(
                client, "rs0", num_blocks=2048, block_size=512, count=3)
            r = hipstore.bdev_replica_scrub(client, "rs0")
            assert r["granule"] == 512
            assert [rep["child"] for rep in r["replicas"]] == [1, 2]
            for rep in r["replicas"]:
                assert rep["granules"] == 2048
                assert rep["mismatched"] == 0 and rep["repaired"] == 0
                assert rep["first_mismatches"] == []
            coarse = hipstore.bdev_replica_scrub(client, "rs0", granule=4096)
            assert coarse["granule"] == 4096
            assert all(rep["granules"] == 256 for rep in coarse["replicas"])

            # repair is offline-only: refused while a vhost controller
            # holds the bdev, compare-only still allowed
            hipstore.construct_vhost_scsi_controller(client, "rs-ctrl")
            hipstore.add_vhost_scsi_lun(client, "rs-ctrl", 0, "rs0")
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_replica_scrub(client, "rs0", repair=True)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert "claimed" in str(err.value)
            assert len(hipstore.bdev_replica_scrub(
                client, "rs0")["replicas"]) == 2
            hipstore.remove_vhost_controller(client, "rs-ctrl")
            r = hipstore.bdev_replica_scrub(client, "rs0", repair=True)
            assert all(rep["repaired"] == 0 for rep in r["replicas"])

    def test_replica_scrub_errors(self, hipstored):  # noqa: F811
        with hipstore.Client(hipstored.socket_path) as client:
            hipstore.construct_malloc_bdev(client, 64, 512, name="plain")
            hipstore.construct_striped_malloc_bdev(
                client, "st0", num_blocks=1024, block_size=512,
                stripe_size_kb=64, count=2)
            hipstore.construct_replicated_malloc_bdev(
                client, "rs1", num_blocks=64, block_size=512, count=2)
            bad = [
                {"name": "nope"},
                {},
                {"name": "plain"},
                {"name": "st0"},
                {"name": "rs1", "granule": 100},
                {"name": "rs1", "granule": -1},
                {"name": "rs1", "max_report": -1},
            ]
            for params in bad:
                with pytest.raises(hipstore.RpcError) as err:
                    client.invoke("bdev_replica_scrub", params)
                assert err.value.code == hipstore.ERROR_INVALID_PARAMS, params
