"""P+Q update from base clones on the generic (host) path and through the
daemon against parity_model.py: exact, so whole bdevs are compared bytewise."""

import numpy as np
import pytest

from oim_amd import _hipstore as hs
from oim_amd import hipstore

from fixtures import hipstored  # noqa: F401
from parity_model import (BLOCK, EXP, LOG, SENTINEL, ParitySet, gf_mul,
                          model_bitmap, parity)

LENGTH = 3 * BLOCK


def whole(bdev, offset, payload):
    tail = bdev.size_bytes - offset - len(payload)
    return bytes([SENTINEL]) * offset + bytes(payload) + bytes([SENTINEL]) * tail


class Tracked:
    """A ParitySet with its parity stored and, per tracked member, a base
    bdev holding a clone of the member's range between sentinel margins."""

    def __init__(self, create, k, length, tracked, base_kinds=None):
        self.s = ParitySet(create, k, length)
        self.s.store_parity()
        self.tracked, self.now = tracked, [bytearray(d) for d in self.s.data]
        self.bases, self.base_offsets = [None] * k, [0] * k
        for i in self.tracked:
            make = (base_kinds or {}).get(i, create)
            base = make(self.s.bdevs[i].name + "-base", BLOCK, length // BLOCK + 3)
            base.fill(0, SENTINEL, base.size_bytes)
            base.write((i % 2 + 1) * BLOCK, self.s.data[i])
            self.bases[i], self.base_offsets[i] = base, (i % 2 + 1) * BLOCK

    def change(self, i, pos, delta=b"\xff"):
        """XORs `delta` into member i (tracked or not) at byte `pos`."""
        for n, x in enumerate(delta):
            self.now[i][pos + n] ^= x
        lo, hi = pos // BLOCK * BLOCK, -(-(pos + len(delta)) // BLOCK) * BLOCK
        self.s.bdevs[i].write(self.s.offsets[i] + lo, bytes(self.now[i][lo:hi]))

    def update(self, which="pq", **extra):
        return hs.parity_update(bases=self.bases, base_offsets=self.base_offsets,
                                **self.s.kwargs("p" in which, "q" in which), **extra)

    def contents(self):
        return [b.read(0, b.size_bytes) for b in self.s.bdevs + self.bases if b]

    def check(self, which="pq", refreshed=False):
        s = self.s  # parity: tracked members' new bytes, all others' old
        p, q = parity([bytes(self.now[i]) if i in self.tracked else s.data[i]
                       for i in range(s.k)])
        want = self.now + [p if "p" in which else s.p, q if "q" in which else s.q]
        for i in range(s.k + 2):
            assert s.content(i) == whole(s.bdevs[i], s.offsets[i], want[i]), i
        for i in self.tracked:
            held, base = self.now[i] if refreshed else s.data[i], self.bases[i]
            assert base.read(0, base.size_bytes) == whole(
                base, self.base_offsets[i], held), i


def changed(n, granules, limit=16):
    want = sorted(granules)
    return {"granules": n, "mismatched": len(want),
            "first_mismatches": want[:limit], "bitmap": model_bitmap(n, want)}


def cancelling_and_refresh(create, refresh):
    """k = 6, tracked [0, 1, 2]. Granule 0: d_0 = d_1, P's delta cancels.
    Granule 2: d_1 = 5 * 3^-1 * d_2 and d_0 = d_1 ^ d_2, both cancel. Both
    granules are reported, and refreshed when asked."""
    t = Tracked(create, 6, LENGTH, [0, 1, 2])
    d = np.random.default_rng(3).integers(1, 256, 16, np.uint8)
    t.change(0, 32, d.tobytes())
    t.change(1, 32, d.tobytes())
    d1 = gf_mul(int(gf_mul(5, EXP[255 - LOG[3]:][:1])[0]), d)
    for i, delta in enumerate((d1 ^ d, d1, d)):
        t.change(i, 2 * BLOCK + 496, delta.tobytes())
    p, q = parity([bytes(m) for m in t.now])
    assert p == t.s.p and q != t.s.q and q[2 * BLOCK:] == t.s.q[2 * BLOCK:]
    r = t.update(refresh=refresh)
    assert r["changed"] == changed(3, [0, 2])
    t.check(refreshed=refresh)
    if refresh:  # the bases are current: a second call has nothing to do
        assert t.update(refresh=True)["changed"] == changed(3, [])
        t.check(refreshed=True)
    return r["on_gpu"]


def tracked_set(create, k, tracked, which, on_gpu):
    t = Tracked(create, k, LENGTH, tracked)
    for n, i in enumerate(tracked):
        t.change(i, n % 3 * BLOCK + [0, 15, 16, BLOCK - 1][n % 4])
    for i in [i for i in range(k) if i not in tracked][:1]:  # is not read
        t.change(i, 2 * BLOCK + 100)
    assert t.update(which, granule=BLOCK) == {
        "length": LENGTH, "on_gpu": on_gpu, "granule": BLOCK,
        "changed": changed(3, {n % 3 for n in range(len(tracked))})}
    t.check(which)


@pytest.mark.parametrize("which", ["p", "q", "pq"])
def test_update(which):
    tracked_set(hs.create_malloc_bdev, 5, [1, 3], which, False)


@pytest.mark.parametrize("refresh", [False, True])
def test_cancelling_and_refresh(refresh):
    assert not cancelling_and_refresh(hs.create_malloc_bdev, refresh)


# name -> changes to the valid k = 3, tracked [0, 1] arguments
INVALID = {
    "wrong bases length": lambda a: a.update(bases=a["bases"][:2]),
    "all None": lambda a: a.update(bases=[None] * 3),
    "base too short": lambda a: a["bases"].__setitem__(
        0, hs.create_malloc_bdev("parbase-short", BLOCK, 2)),
    "base is a member": lambda a: a["bases"].__setitem__(1, a["data"][2]),
    "two slots, one base": lambda a: a["bases"].__setitem__(2, a["bases"][0]),
    "other block size": lambda a: a["bases"].__setitem__(
        0, hs.create_malloc_bdev("parbase-4k", 4096, 16)),
    "granule not a block multiple": lambda a: a.update(granule=16),
    "length not a granule multiple": lambda a: a.update(granule=1024),
}


@pytest.mark.parametrize("case", INVALID)
def test_rejected(case):
    t = Tracked(hs.create_malloc_bdev, 3, LENGTH, [0, 1])
    t.change(0, 5)
    args = dict(t.s.kwargs(), bases=list(t.bases), base_offsets=t.base_offsets,
                refresh=True)
    INVALID[case](args)
    before = t.contents()
    with pytest.raises(ValueError):
        hs.parity_update(**args)
    assert t.contents() == before


def test_rpc(hipstored):  # noqa: F811
    with hipstore.Client(hipstored.socket_path) as client:
        names = [f"pu{i}" for i in range(5)]
        for name in names:
            hipstore.construct_malloc_bdev(client, 64, BLOCK, name=name)
        assert "bdev_parity_update" in client.invoke("get_rpc_methods")
        data, pq = names[:3], dict(p="pu3", q="pu4")
        hipstore.bdev_parity_encode(client, data, **pq)
        hipstore.bdev_clone(client, "pu1", "pu1-base")
        hipstore.perf_run(client, "pu1", workload="randwrite", io_size=4096,
                          queue_depth=4, num_queues=1, seconds=5.0, max_ios=4)
        stale = hipstore.bdev_parity_scrub(client, data, **pq)["p"]["mismatched"]
        bases = [None, "pu1-base", None]
        r = hipstore.bdev_parity_update(client, data, bases, refresh=True, **pq)
        assert r["changed"]["mismatched"] == stale > 0 and not r["on_gpu"]
        # A claimed base is refused only with refresh, a claimed parity always.
        hipstore.construct_vhost_scsi_controller(client, "pu-ctrl")
        hipstore.add_vhost_scsi_lun(client, "pu-ctrl", 0, "pu1-base")
        r = hipstore.bdev_parity_update(client, data, bases, **pq)
        assert r["changed"]["mismatched"] == 0
        for refresh, claim_next in ((True, "pu3"), (False, "pu4")):
            with pytest.raises(hipstore.RpcError) as err:
                hipstore.bdev_parity_update(client, data, bases,
                                            refresh=refresh, **pq)
            assert err.value.code == hipstore.ERROR_INTERNAL
            assert "claimed" in str(err.value)
            hipstore.add_vhost_scsi_lun(client, "pu-ctrl", 1 + refresh, claim_next)
        r = hipstore.bdev_parity_scrub(client, data, **pq)
        assert r["p"]["mismatched"] == r["q"]["mismatched"] == 0
