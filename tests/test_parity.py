"""P+Q parity on the generic (host) path and through the daemon's RPC
plane, against the numpy reference of parity_model.py: exact integer
arithmetic, so every comparison is byte equality. The kernels are checked
against the same reference in test_parity_gpu.py."""

import itertools

import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import hipstored  # noqa: F401
from parity_model import BLOCK, SENTINEL, ParitySet, model_bitmap

LENGTH = 3 * BLOCK
LOSSES = [c for n in (1, 2) for c in itertools.combinations(range(6), n)]


def lost_names(loss, k):
    return [i if i < k else "pq"[i - k] for i in loss]


@pytest.mark.parametrize("k", [1, 3])
def test_encode(k):
    s = ParitySet(hs.create_malloc_bdev, k, LENGTH)
    assert hs.parity_encode(**s.kwargs()) == {"length": LENGTH, "on_gpu": False}
    for i in range(k + 2):  # parity right, sentinels and data untouched
        assert s.content(i) == s.expected(i), i


@pytest.mark.parametrize("loss", LOSSES, ids=str)
def test_rebuild(loss):
    s = ParitySet(hs.create_malloc_bdev, 4, LENGTH)
    s.store_parity()
    for i in loss:
        s.bdevs[i].fill(s.offsets[i], SENTINEL, LENGTH)
    hs.parity_rebuild(lost=lost_names(loss, 4), **s.kwargs())
    for i in range(6):
        assert s.content(i) == s.expected(i), i


def test_rebuild_with_one_parity():
    """P alone and Q alone each bring back one data member."""
    for keep in ("p", "q"):
        s = ParitySet(hs.create_malloc_bdev, 4, LENGTH)
        s.store_parity()
        s.bdevs[2].fill(s.offsets[2], SENTINEL, LENGTH)
        hs.parity_rebuild(lost=[2], **s.kwargs(p=keep == "p", q=keep == "q"))
        assert s.content(2) == s.expected(2), keep


def test_check_planted():
    n, k = 130, 3
    s = ParitySet(hs.create_malloc_bdev, k, n * BLOCK)
    s.store_parity()
    assert hs.parity_check(**s.kwargs())["p"]["mismatched"] == 0
    sets = {k: [0, 64], k + 1: [63, 129], 1: [1, 65]}  # P, Q, data member 1
    positions = itertools.cycle([0, 15, 16, BLOCK - 1])
    for member, granules in sets.items():
        for g in granules:
            at = s.offsets[member] + g * BLOCK
            block = bytearray(s.bdevs[member].read(at, BLOCK))
            block[next(positions)] ^= 0xFF
            s.bdevs[member].write(at, bytes(block))
    r = hs.parity_check(max_report=64, **s.kwargs())
    for name, member in (("p", k), ("q", k + 1)):
        want = sorted(sets[member] + sets[1])
        assert r[name] == {"granules": n, "mismatched": len(want),
                           "first_mismatches": want,
                           "bitmap": model_bitmap(n, want)}, name


# name -> (call, changes to the valid k = 3 set's arguments, error)
INVALID = {
    "k = 0": ("encode", lambda s, a: a.update(data=[], data_offsets=[]), ValueError),
    "k = 33": ("encode", lambda s, a: a.update(
        data=[hs.create_malloc_bdev(f"par-wide-{i}", BLOCK, 16) for i in range(33)],
        data_offsets=[]), ValueError),
    "block sizes": ("encode", lambda s, a: a.update(
        q=hs.create_malloc_bdev("par-4k", 4096, 16), q_offset=0), ValueError),
    "zero length": ("encode", lambda s, a: a.update(
        length=0, p_offset=s.bdevs[3].size_bytes), ValueError),
    "length not a block multiple": ("encode", lambda s, a: a.update(length=528),
                                    ValueError),
    "offset not a block multiple": ("encode", lambda s, a: a.update(p_offset=16),
                                    ValueError),
    "out of bounds": ("encode", lambda s, a: a.update(
        q_offset=s.bdevs[4].size_bytes - BLOCK), ValueError),
    "wrapping offset": ("encode", lambda s, a: a.update(q_offset=2**64 - BLOCK),
                        ValueError),
    "bdev twice": ("encode", lambda s, a: a.update(
        data=[a["data"][0], a["data"][1], a["data"][0]]), ValueError),
    "input is output": ("encode", lambda s, a: a.update(p=a["data"][2]), ValueError),
    "no parity": ("encode", lambda s, a: a.update(p=None, q=None), ValueError),
    "three lost": ("rebuild", lambda s, a: a.update(lost=[0, 1, "p"]), ValueError),
    "nothing lost": ("rebuild", lambda s, a: a.update(lost=[]), ValueError),
    "lost index = k": ("rebuild", lambda s, a: a.update(lost=[3]), ValueError),
    "duplicate lost": ("rebuild", lambda s, a: a.update(lost=[1, 1]), ValueError),
    "two data lost, P only": ("rebuild", lambda s, a: a.update(lost=[0, 1], q=None),
                              ValueError),
    "data and P lost, P only": ("rebuild", lambda s, a: a.update(lost=[0, "p"], q=None),
                                ValueError),
    "lost parity not given": ("rebuild", lambda s, a: a.update(lost=["q"], q=None),
                              ValueError),
    "granule not a block multiple": ("check", lambda s, a: a.update(granule=16),
                                     ValueError),
    "length not a granule multiple": ("check", lambda s, a: a.update(granule=1024),
                                      ValueError),
}


@pytest.mark.parametrize("case", INVALID)
def test_rejected(case):
    call, change, error = INVALID[case]
    s = ParitySet(hs.create_malloc_bdev, 3, LENGTH)
    args = s.kwargs()
    change(s, args)
    before = [s.content(i) for i in range(5)]
    with pytest.raises(error):
        getattr(hs, "parity_" + call)(**args)
    assert [s.content(i) for i in range(5)] == before


def test_rpc(hipstored):  # noqa: F811
    with hipstore.Client(hipstored.socket_path) as client:
        names = [f"pr{i}" for i in range(5)]
        for name in names:
            hipstore.construct_malloc_bdev(client, 64, BLOCK, name=name)
        methods = client.invoke("get_rpc_methods")
        for method in ("bdev_parity_encode", "bdev_parity_scrub",
                       "bdev_parity_rebuild"):
            assert method in methods
        r = hipstore.bdev_parity_encode(client, names[:3], p="pr3", q="pr4")
        assert r["length"] == 64 * BLOCK
        r = hipstore.bdev_parity_scrub(client, names[:3], p="pr3", q="pr4")
        assert r["p"] == r["q"] == {"granules": 64, "mismatched": 0,
                                    "first_mismatches": []}
        with pytest.raises(hipstore.RpcError) as err:
            hipstore.bdev_parity_rebuild(client, names[:3], [0, 1], p="pr3")
        assert err.value.code == hipstore.ERROR_INVALID_PARAMS
        assert "cannot cover" in str(err.value)
        # A claimed target (kIoFailed) is refused and keeps its bytes; a
        # scrub only reads and is still allowed. Member 0 changes first,
        # so a call that did write would change P and member 1.
        hipstore.perf_run(client, "pr0", workload="randwrite", io_size=4096,
                          queue_depth=4, num_queues=1, seconds=5.0, max_ios=4)
        hipstore.construct_vhost_scsi_controller(client, "pr-ctrl")
        for lun, name in enumerate(("pr1", "pr3")):
            hipstore.bdev_clone(client, name, name + "-was")
            hipstore.add_vhost_scsi_lun(client, "pr-ctrl", lun, name)
        for call in (
                lambda: hipstore.bdev_parity_encode(client, names[:3], p="pr3"),
                lambda: hipstore.bdev_parity_rebuild(client, names[:3], ["p"],
                                                     p="pr3", q="pr4"),
                lambda: hipstore.bdev_parity_rebuild(client, names[:3], [1],
                                                     p="pr3", q="pr4")):
            with pytest.raises(hipstore.RpcError) as err:
                call()
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert "claimed" in str(err.value)
        for name in ("pr1", "pr3"):
            assert hipstore.bdev_compare(
                client, name, name + "-was")["mismatched"] == 0
        assert hipstore.bdev_parity_scrub(
            client, names[:3], p="pr3", q="pr4")["p"]["mismatched"] > 0
