"""hipstore::k_parity_encode / k_parity_check / k_parity_rebuild on HBM
bdevs against the numpy reference of parity_model.py (exact integer
arithmetic: byte equality throughout) and against the generic host path.
All ranges are validated on the host before any launch."""

import itertools

import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import launch_hipstored
from parity_model import BLOCK, EXP, SENTINEL, ParitySet, gf_mul, model_bitmap

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device")

MAX_WGS = 2048
# One grid pass of the column kernels is 2048 x 256 x 16 B = 8 MiB: this
# wraps the grid-stride loop twice and ends ragged.
LONG = 16 * 2**20 + BLOCK
ENCODE_SHAPES = [(k, n) for k in (1, 2, 5, 32) for n in (BLOCK, 3 * BLOCK)]
ENCODE_SHAPES.append((2, LONG))
PAIRS = [c for n in (1, 2) for c in itertools.combinations(range(6), n)]


def hbm(name, block, blocks):
    return hs.create_hbm_bdev(name, block, blocks, device=0)


def lost_names(loss, k):
    return [i if i < k else "pq"[i - k] for i in loss]


@needs_gpu
@pytest.mark.parametrize("which", ["p", "q", "pq"])
@pytest.mark.parametrize("k,length", ENCODE_SHAPES)
def test_encode(k, length, which):
    s = ParitySet(hbm, k, length)
    r = hs.parity_encode(**s.kwargs(p="p" in which, q="q" in which))
    assert r == {"length": length, "on_gpu": True}
    sentinel = bytes([SENTINEL]) * s.bdevs[k].size_bytes
    for name, i in (("p", k), ("q", k + 1)):
        # written: the reference and the sentinel on both sides of it;
        # not asked for: sentinel throughout
        assert s.content(i) == (s.expected(i) if name in which else sentinel), name


@needs_gpu
@pytest.mark.parametrize("k,loss", [(4, c) for c in PAIRS] +
                         [(32, (0, 31)), (32, (30, 31)), (32, (31, 33))], ids=str)
def test_rebuild(k, loss):
    s = ParitySet(hbm, k, 3 * BLOCK)
    s.store_parity()
    for i in loss:
        s.bdevs[i].fill(s.offsets[i], SENTINEL, s.length)
    r = hs.parity_rebuild(lost=lost_names(loss, k), **s.kwargs())
    assert r["on_gpu"]
    for i in range(k + 2):  # survivors too: they were not written
        assert s.content(i) == s.expected(i), i


@needs_gpu
@pytest.mark.parametrize("granule,n", [(512, 2 * MAX_WGS * 64 + 65),
                                       (1024, 130), (1536, 130)])
def test_check_planted(granule, n):
    """Uniform members have uniform parity. Single-byte flips in three
    disjoint granule sets: in P, in Q and in data member 1."""
    fills = [0x3C, 0xA5]
    members = [hbm(f"pc-{granule}-{i}", BLOCK, n * granule // BLOCK)
               for i in range(4)]
    p_fill = fills[0] ^ fills[1]
    q_fill = fills[0] ^ int(gf_mul(EXP[1], np.array([fills[1]], np.uint8))[0])
    for bdev, fill in zip(members, fills + [p_fill, q_fill]):
        bdev.fill(0, fill, bdev.size_bytes)
    fixed = [0, 63, 64, 65, MAX_WGS * 64 - 1, MAX_WGS * 64, n - 1]
    rng = np.random.default_rng(granule)
    planted = sorted({g for g in fixed if g < n} |
                     set(rng.choice(n, 30, replace=False).tolist()))
    sets = {2: planted[0::3], 3: planted[1::3], 1: planted[2::3]}
    positions = itertools.cycle([0, 15, 16, granule - 1])
    for member, granules in sets.items():
        for g in granules:
            pos = next(positions)
            at = g * granule + pos // BLOCK * BLOCK
            block = bytearray(members[member].read(at, BLOCK))
            block[pos % BLOCK] ^= 0xFF
            members[member].write(at, bytes(block))
    r = hs.parity_check(members[:2], members[2], members[3], granule=granule,
                        max_report=1024)
    assert r["on_gpu"]
    for name, member in (("p", 2), ("q", 3)):
        want = sorted(sets[member] + sets[1])
        assert r[name] == {"granules": n, "mismatched": len(want),
                           "first_mismatches": want,
                           "bitmap": model_bitmap(n, want)}, name


@needs_gpu
@pytest.mark.parametrize("mixed", [False, True])
def test_two_paths_agree(mixed):
    """The same bytes on malloc twins, and a set with one malloc member
    (generic path), give what the HBM set gives."""
    k, length = 3, 3 * BLOCK
    kinds = {1: hs.create_malloc_bdev} if mixed else None
    gpu = ParitySet(hbm, k, length)
    host = ParitySet(hs.create_malloc_bdev if not mixed else hbm, k, length,
                     kinds=kinds)
    assert hs.parity_encode(**gpu.kwargs())["on_gpu"]
    assert not hs.parity_encode(**host.kwargs())["on_gpu"]
    for s in (gpu, host):  # one stale parity granule each, then two losses
        s.bdevs[k].fill(s.offsets[k] + BLOCK, SENTINEL, BLOCK)
    checks = [hs.parity_check(max_report=8, **s.kwargs()) for s in (gpu, host)]
    assert checks[0].pop("on_gpu") and not checks[1].pop("on_gpu")
    assert checks[0] == checks[1]
    assert checks[0]["p"]["first_mismatches"] == [1]
    for s in (gpu, host):
        s.store_parity()
        for i in (0, 2):
            s.bdevs[i].fill(s.offsets[i], SENTINEL, length)
        hs.parity_rebuild(lost=[0, 2], **s.kwargs())
    for i in range(k + 2):
        assert gpu.content(i) == host.content(i) == gpu.expected(i), i


@needs_gpu
def test_daemon_round_trip(tmp_path):
    fixture = launch_hipstored(tmp_path, cpu=False)
    try:
        with hipstore.Client(fixture.socket_path) as client:
            names = [f"pd{i}" for i in range(5)]
            rng = np.random.default_rng(11)
            for i, name in enumerate(names):
                hipstore.construct_malloc_bdev(client, 2048, BLOCK, name=name)
                if i < 3:  # random content arrives as a full delta file
                    local = hs.create_malloc_bdev(f"pd-local-{i}", BLOCK, 2048)
                    local.write(0, rng.integers(0, 256, 2048 * BLOCK,
                                                np.uint8).tobytes())
                    path = str(tmp_path / f"{name}.delta")
                    hs.bdev_export_delta(local, path)
                    hipstore.bdev_import_delta(client, name, path)
            data, p, q = names[:3], names[3], names[4]
            assert hipstore.bdev_parity_encode(client, data, p=p, q=q)["on_gpu"]
            r = hipstore.bdev_parity_scrub(client, data, p=p, q=q, granule=4096)
            assert r["p"]["granules"] == 256
            assert r["p"]["mismatched"] == r["q"]["mismatched"] == 0
            for name in (names[0], names[2]):
                hipstore.bdev_clone(client, name, name + "-was")
                client.invoke("bdev_copy", {"src": p, "dst": name})  # overwrite
                assert hipstore.bdev_compare(
                    client, name, name + "-was")["mismatched"] > 0
            r = hipstore.bdev_parity_scrub(client, data, p=p, q=q)
            assert r["p"]["mismatched"] > 0 and r["q"]["mismatched"] > 0
            assert hipstore.bdev_parity_rebuild(
                client, data, [0, 2], p=p, q=q)["on_gpu"]
            for name in (names[0], names[2]):
                assert hipstore.bdev_compare(
                    client, name, name + "-was")["mismatched"] == 0
    finally:
        fixture.stop()
