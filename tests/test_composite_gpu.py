"""Striped and replicated bdevs over HBM children against a byte model.

native/src/composite.cpp feeds the HBM engines with sub-requests whose
shapes it chooses itself: pieces cut at stripe boundaries (a 512- or
1536-byte stripe is no multiple of the engines' 4 KiB tile), several
pieces of one parent request on one child channel in one burst, and
every write and fill of a same-device replicated bdev mirrored through
each child's engine from one shared pinned buffer. These tests drive
composites with hs.IoQueue (a whole list of requests submitted before
the first poll) and compare every byte with tests/io_model.py.

A round trip through a striped bdev cannot see a consistently wrong
placement, and a read through a replicated bdev sees one replica only,
so every test also reads each child directly: striped children must
hold io_model.stripe_layout(), replicas the whole model. No tolerances
anywhere: a byte is right or wrong.

IoQueue.kind says "cpu" for a composite, so each child's engine is
asserted with a probe channel before the composite is built. Every test
prints one `composite-matrix` line (geometry, children's engine, ops
and tiles verified); run with -s to see them. tests/test_composite.py
runs the same scenarios on host-RAM children.
"""

import pytest

from oim_amd import _hipstore as hs

import io_model
from io_model import ByteModel, RecordingQueue

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device"),
    pytest.mark.timeout(120),
]

ENGINES = ("batched", "persistent", "shared")

KIB = 1 << 10
MIB = 1 << 20

# Seeds with which each scenario alone reads from every replica of 2, 3
# and 4 replicas of 4 MiB (a condition on the inputs, asserted below).
SEED_EDGES = 11
SEED_MIXED = 12

DEVICES = hs.gpu_device_count() if hs.gpu_available() else 0


def make_child(engine, monkeypatch, name, size_bytes, device=0):
    """512-byte-block HBM bdev whose channels land on `engine`."""
    if engine == "shared":
        # Read by the bdev constructor on every call.
        monkeypatch.setenv("HIPSTORE_SHARED", "1")
    else:
        monkeypatch.delenv("HIPSTORE_SHARED", raising=False)
    child = hs.create_hbm_bdev(name, 512, size_bytes // 512, device=device,
                               persistent=engine != "batched")
    probe = hs.IoQueue(child)
    assert probe.kind == engine
    del probe
    return child


def make_children(engine, monkeypatch, tag, count, size_bytes, devices=None):
    devices = [0] * count if devices is None else devices
    return [make_child(engine, monkeypatch, f"cg-{tag}-{engine}-{i}",
                       size_bytes, device=devices[i]) for i in range(count)]


def read_all(bdevs):
    """Every bdev of the list in full, one after the other, each through
    a throw-away channel of its own. Nearly all of a resident-engine
    test's seconds go into closing channels (0.8 s per shared-engine
    channel, 1.4 s for a composite channel over per-queue kernels);
    holding one channel per child open side by side made it slower."""
    return [bdev.read(0, bdev.size_bytes) for bdev in bdevs]


def report(test, geometry, engine, model):
    print(f"composite-matrix {test} geometry={geometry} children={engine} "
          f"ops={model.ops_checked} tiles={model.tiles_checked}", flush=True)


def check_striped(bdev, children, model, stripe):
    """Whole bdev through fresh channels, then each child directly."""
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)
    want = io_model.stripe_layout(model.data, len(children), stripe)
    for index, held in enumerate(read_all(children)):
        assert held == want[index], (
            f"child {index} does not hold its stripe units")


def check_replicas(bdev, children, model):
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)
    for index, held in enumerate(read_all(children)):
        assert held == bytes(model.data), (
            f"replica {index} differs from the model")


class Replicated:
    """A replicated bdev with its children at hand; run() drives both
    generator scenarios through one queue."""

    def __init__(self, name, children):
        self.children = children
        self.bdev = hs.create_replicated_bdev(name, children)
        self.model = ByteModel(self.bdev.size_bytes)

    def run(self):
        n = len(self.children)
        queue = RecordingQueue(hs.IoQueue(self.bdev))
        assert queue.kind == "cpu"
        io_model.scenario_tile_edges(queue, self.model, seed=SEED_EDGES)
        io_model.scenario_mixed_batch(queue, self.model, seed=SEED_MIXED)
        # Reads are routed to replica (offset // 1 MiB) % n: the reads
        # of this test must have reached every replica.
        served = io_model.replicas_read(queue.runs, self.model, n)
        assert served == set(range(n)), served
        del queue
        check_replicas(self.bdev, self.children, self.model)

    def scrub_clean(self):
        """Every replica against child 0, granule by granule."""
        result = hs.replica_scrub(self.bdev)
        assert len(result["replicas"]) == len(self.children) - 1
        for replica in result["replicas"]:
            assert replica["granules"] == self.bdev.size_bytes // 512
            assert replica["mismatched"] == 0, replica


# (engine, children, stripe): every multi-child geometry on the batched
# engine; the stripe that is no tile multiple and the largest one on
# each resident engine.
BOUNDARY_CASES = (
    [("batched", n, stripe) for n, stripe in
     ((2, 512), (3, 1536), (3, 4096), (2, 65536), (2, 131072))]
    + [(engine, n, stripe) for engine in ("persistent", "shared")
       for n, stripe in ((3, 1536), (2, 131072))])


@pytest.mark.parametrize("engine,n,stripe", BOUNDARY_CASES)
def test_striped_boundaries(engine, n, stripe, monkeypatch):
    child_bytes = 1536 * KIB if n == 3 else 2 * MIB
    children = make_children(engine, monkeypatch, f"sb{stripe}", n,
                             child_bytes)
    bdev = hs.create_striped_bdev(f"cg-sb-{engine}-{n}-{stripe}", children,
                                  stripe)
    queue = hs.IoQueue(bdev)
    assert queue.kind == "cpu"
    model = ByteModel(bdev.size_bytes)
    io_model.scenario_stripe_boundaries(queue, model, 41, stripe, n)
    report("striped_boundaries",
           f"striped(n={n},stripe={stripe},child={child_bytes // KIB}KiB)",
           engine, model)
    del queue
    check_striped(bdev, children, model, stripe)


@pytest.mark.parametrize("engine", ENGINES)
def test_striped_tile_edges(engine, monkeypatch):
    children = make_children(engine, monkeypatch, "se", 3, 1536 * KIB)
    bdev = hs.create_striped_bdev(f"cg-se-{engine}", children, 1536)
    queue = hs.IoQueue(bdev)
    assert queue.kind == "cpu"
    model = ByteModel(bdev.size_bytes)
    assert len(io_model.OpGenerator(model.size, 0).free) == 60
    assert io_model.scenario_tile_edges(queue, model, seed=42) == 82
    report("striped_tile_edges", "striped(n=3,stripe=1536,child=1536KiB)",
           engine, model)
    del queue
    check_striped(bdev, children, model, 1536)


@pytest.mark.parametrize("engine", ENGINES)
def test_striped_mixed_batch(engine, monkeypatch):
    """The three invalid ops of the scenario must come back as -22 from
    the parent and change nothing (the scenario asserts both)."""
    children = make_children(engine, monkeypatch, "sm", 2, 2 * MIB)
    bdev = hs.create_striped_bdev(f"cg-sm-{engine}", children, 65536)
    queue = hs.IoQueue(bdev)
    assert queue.kind == "cpu"
    model = ByteModel(bdev.size_bytes)
    io_model.scenario_mixed_batch(queue, model, seed=43)
    report("striped_mixed_batch", "striped(n=2,stripe=65536,child=2048KiB)",
           engine, model)
    del queue
    check_striped(bdev, children, model, 65536)


@pytest.mark.parametrize("engine", ENGINES)
def test_replicated_same_device(engine, monkeypatch):
    """Two replicas on one device: no peer copies, every write and fill
    goes through both children's engines from one pinned buffer."""
    children = make_children(engine, monkeypatch, "rs", 2, 4 * MIB)
    rig = Replicated(f"cg-rs-{engine}", children)
    rig.run()
    rig.scrub_clean()   # cross-check on the device: k_diff_granules
    report("replicated_same_device", "replicated(n=2,child=4096KiB)",
           engine, rig.model)


def test_replicated_mixed_children(monkeypatch):
    """One HBM and one host-RAM replica (scrub takes its host path)."""
    children = [make_child("batched", monkeypatch, "cg-rm-hbm", 4 * MIB),
                hs.create_malloc_bdev("cg-rm-ram", 512, 4 * MIB // 512)]
    rig = Replicated("cg-rm", children)
    rig.run()
    rig.scrub_clean()
    report("replicated_mixed_children", "replicated(hbm+malloc,child=4096KiB)",
           "batched+cpu", rig.model)


def run_nested(engine, monkeypatch, tag, devices):
    """A 4 KiB stripe over two replicated pairs; pair p's leaves sit on
    devices[p]."""
    leaves = [make_children(engine, monkeypatch, f"{tag}{pair}", 2, 2 * MIB,
                            devices=devices[pair]) for pair in range(2)]
    pairs = [hs.create_replicated_bdev(f"cg-{tag}-pair{pair}", leaves[pair])
             for pair in range(2)]
    bdev = hs.create_striped_bdev(f"cg-{tag}", pairs, 4096)
    queue = hs.IoQueue(bdev)
    assert queue.kind == "cpu"
    model = ByteModel(bdev.size_bytes)
    assert io_model.scenario_tile_edges(queue, model, seed=44) == 82
    del queue
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)
    want = io_model.stripe_layout(model.data, 2, 4096)
    held = read_all(leaves[0] + leaves[1])
    for leaf in range(4):
        assert held[leaf] == want[leaf // 2], (
            f"pair {leaf // 2} replica {leaf % 2}")
    return model


@pytest.mark.parametrize("engine", ["persistent"])
def test_nested(engine, monkeypatch):
    model = run_nested(engine, monkeypatch, "n", [[0, 0], [0, 0]])
    report("nested", "striped(n=2,stripe=4096) over replicated(n=2,"
           "child=2048KiB)", engine, model)


# ---------------------------------------------------------------------------
# More than one device: the same scenarios and end checks.
# ---------------------------------------------------------------------------

@pytest.mark.skipif(DEVICES < 2, reason="needs >=2 GPUs for xGMI peer copies")
@pytest.mark.parametrize("engine", ["batched", "persistent"])
def test_replicated_two_devices(engine, monkeypatch):
    """Writes go to the primary and from there to the replica as a peer
    copy; fills and reads go through each child's own engine."""
    children = make_children(engine, monkeypatch, "r2", 2, 4 * MIB,
                             devices=[0, 1])
    rig = Replicated(f"cg-r2-{engine}", children)
    rig.run()
    rig.scrub_clean()
    report("replicated_two_devices", "replicated(devices=0+1,child=4096KiB)",
           engine, rig.model)


@pytest.mark.skipif(DEVICES < 3,
                    reason="needs >=3 GPUs for RCCL broadcast fan-out")
@pytest.mark.parametrize("rccl", ["rccl", "peer-copies"])
def test_replicated_three_or_more_devices(rccl, monkeypatch):
    """>= 3 replicas: ncclBroadcast fan-out, and with HIPSTORE_RCCL=0
    (read by the bdev constructor) a chain of peer copies."""
    if rccl == "rccl":
        monkeypatch.delenv("HIPSTORE_RCCL", raising=False)
    else:
        monkeypatch.setenv("HIPSTORE_RCCL", "0")
    n = min(DEVICES, 4)
    children = make_children("batched", monkeypatch, f"r{n}{rccl}", n,
                             4 * MIB, devices=list(range(n)))
    rig = Replicated(f"cg-r{n}-{rccl}", children)
    rig.run()
    rig.scrub_clean()
    report(f"replicated_{n}_devices[{rccl}]",
           f"replicated(devices=0..{n - 1},child=4096KiB)", "batched",
           rig.model)


@pytest.mark.skipif(DEVICES < 2, reason="needs >=2 GPUs")
@pytest.mark.parametrize("engine", ["batched", "persistent"])
def test_striped_two_devices(engine, monkeypatch):
    children = make_children(engine, monkeypatch, "s2", 2, 2 * MIB,
                             devices=[0, 1])
    bdev = hs.create_striped_bdev(f"cg-s2-{engine}", children, 65536)
    queue = hs.IoQueue(bdev)
    assert queue.kind == "cpu"
    model = ByteModel(bdev.size_bytes)
    io_model.scenario_stripe_boundaries(queue, model, 45, 65536, 2)
    io_model.scenario_tile_edges(queue, model, seed=46)
    io_model.scenario_mixed_batch(queue, model, seed=47)
    report("striped_two_devices",
           "striped(devices=0+1,stripe=65536,child=2048KiB)", engine, model)
    del queue
    check_striped(bdev, children, model, 65536)
