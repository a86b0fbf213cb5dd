"""Runs of ring descriptors on the two resident engines.

A worker wave of k_persistent_copy / k_shared_service claims up to
HIPSTORE_BATCH_TILES consecutive ring indices at once, fetches their
descriptors with one load, moves the tiles with write-through stores and
publishes all completion words after one drain of its own stores. Every
test here drives an hs.IoQueue and compares each byte with
io_model.ByteModel; nothing is measured and nothing has a tolerance.

test_single_tile_roundtrip is first on purpose: it is the narrowest run
of the kernels (one descriptor at a time, nothing ever queued behind
anything) and the one to run alone after a change to them.
"""

import json
import os
import random
import subprocess
import sys
import time

import pytest

from oim_amd import _hipstore as hs

import io_model
from io_model import ByteModel, OpGenerator, run_checked

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device"),
]

RESIDENT = ("persistent", "shared")
MIB = 1 << 20
TILE = io_model.TILE
RING = 32768            # descriptors per resident-engine channel


def make_queue(engine, monkeypatch, name, block_size=512, workers=None,
               batch=None):
    """A 64 MiB HBM bdev and one queue on `engine`. The per-queue engine
    reads its worker count and run length when the channel is created;
    the shared service reads them when its kernel is (re)launched, so in
    this process they take effect there only if it is not resident."""
    if engine == "shared":
        monkeypatch.setenv("HIPSTORE_SHARED", "1")
    else:
        monkeypatch.delenv("HIPSTORE_SHARED", raising=False)
    if workers is not None:
        monkeypatch.setenv("HIPSTORE_PERSISTENT_WORKERS", str(workers))
        monkeypatch.setenv("HIPSTORE_SHARED_WORKERS", str(workers))
    if batch is not None:
        monkeypatch.setenv("HIPSTORE_BATCH_TILES", str(batch))
    bdev = hs.create_hbm_bdev(name, block_size, 64 * MIB // block_size,
                              device=0, persistent=True)
    queue = hs.IoQueue(bdev)
    assert queue.kind == engine
    return bdev, queue


def report(test, queue, model, **extra):
    fields = dict(kind=queue.kind, ops=model.ops_checked,
                  tiles=model.tiles_checked, **extra)
    print("resident-batching " + test + " "
          + " ".join(f"{k}={v}" for k, v in fields.items()), flush=True)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("engine", RESIDENT)
def test_single_tile_roundtrip(engine, monkeypatch):
    """QD=1: sixteen times one 4 KiB write in a run() of its own and its
    read-back in the next. Every claim is a run of one."""
    bdev, queue = make_queue(engine, monkeypatch, f"rb-single-{engine}")
    model = ByteModel(bdev.size_bytes)
    gen = OpGenerator(bdev.size_bytes, seed=11, lengths=(TILE,))
    for _ in range(16):
        write = gen.make("write", TILE)
        run_checked(queue, model, [write])
        run_checked(queue, model, io_model.readback([write]))
    report("single_tile", queue, model)
    assert model.ops_checked == 32


@pytest.mark.timeout(120)
@pytest.mark.parametrize("batch", (1, 2, 4, 8))
@pytest.mark.parametrize("engine", RESIDENT)
def test_batch_sizes(engine, batch):
    """Run lengths 1, 2, 4 and 8 with two worker waves: lists of 1, 3,
    5, 17 and 64 single-tile writes at random offsets, each submitted in
    one run() and read back through the same queue (a child process per
    case: tests/resident_batch_child.py says why)."""
    script = os.path.join(os.path.dirname(__file__),
                          "resident_batch_child.py")
    env = dict(os.environ, HIPSTORE_BATCH_TILES=str(batch),
               HIPSTORE_PERSISTENT_WORKERS="2", HIPSTORE_SHARED_WORKERS="2")
    if engine == "shared":
        env["HIPSTORE_SHARED"] = "1"
    else:
        env.pop("HIPSTORE_SHARED", None)
    proc = subprocess.run([sys.executable, script, engine], env=env,
                          capture_output=True, text=True, timeout=100)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    print("resident-batching batch_sizes " + json.dumps(result), flush=True)
    assert result["ok"] is True, result
    assert result["kind"] == engine
    assert result["batch"] == str(batch)
    assert result["tiles"] == 2 * (1 + 3 + 5 + 17 + 64)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("engine", RESIDENT)
def test_mixed_run(engine, monkeypatch):
    """One request list whose neighbouring descriptors differ in kind
    and size: writes, fills and reads of 16, 512, 4080 and 4096 bytes
    and the block-unaligned multi-tile lengths of io_model.EDGE_LENGTHS,
    on a bdev of 16-byte blocks. With two workers and runs of up to
    eight they share runs."""
    bdev, queue = make_queue(engine, monkeypatch, f"rb-mixed-{engine}",
                             block_size=16, workers=2, batch=8)
    model = ByteModel(bdev.size_bytes, block_size=16)
    lengths = (16, 512, 4080, 4096) + io_model.EDGE_LENGTHS
    gen = OpGenerator(bdev.size_bytes, seed=22, lengths=lengths)
    n = len(lengths)
    seeded = gen.batch(n, kinds=("write",))
    under = gen.batch(n, kinds=("write",))     # non-zero under the fills
    run_checked(queue, model, seeded + under)
    writes = gen.batch(n, kinds=("write",))
    fills = [gen.make("fill", io_model.op_length(op), at=op[1])
             for op in under]
    reads = [("read", op[1], io_model.op_length(op)) for op in seeded]
    mixed = [op for trio in zip(writes, fills, reads) for op in trio]
    kinds = [op[0] for op in mixed]
    assert all(a != b for a, b in zip(kinds, kinds[1:]))
    run_checked(queue, model, mixed)
    run_checked(queue, model,
                io_model.readback(mixed) + io_model.guard_reads(mixed, 16))
    report("mixed_run", queue, model,
           run_tiles=sum(io_model.op_tiles(op) for op in mixed))
    del queue
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)


def advance_tail(queue, model, tail, target):
    """Fills over the lower 32 MiB until the ring tail is `target`."""
    value = 1
    while tail < target:
        tiles = min(8192, target - tail)
        run_checked(queue, model, [("fill", 0, tiles * TILE, value)])
        tail += tiles
        value += 1
    return tail


@pytest.mark.timeout(60)
@pytest.mark.parametrize("engine", RESIDENT)
def test_run_straddles_ring_end(engine, monkeypatch):
    """With the tail three short of the ring end, one run() holds an
    8-tile write and an 8-tile read: the write's descriptors straddle
    the end (with two workers and runs of eight they are one run). The
    same around the second wrap, where the straddling request is the
    read of what the first one wrote. Ops of one run() are unordered, so
    the read paired with each write is of the previous write."""
    bdev, queue = make_queue(engine, monkeypatch, f"rb-wrap-{engine}",
                             workers=2, batch=8)
    model = ByteModel(bdev.size_bytes)
    rng = random.Random(33)
    span = 8 * TILE
    at = [40 * MIB + 512, 44 * MIB + 512, 48 * MIB + 512]
    run_checked(queue, model, [("write", at[0], rng.randbytes(span))])
    tail = advance_tail(queue, model, 8, RING - 3)
    run_checked(queue, model, [("write", at[1], rng.randbytes(span)),
                               ("read", at[0], span)])
    tail += 16
    run_checked(queue, model, [("read", at[1], span)])
    tail += 8
    tail = advance_tail(queue, model, tail, 2 * RING - 3)
    run_checked(queue, model, [("read", at[1], span),
                               ("write", at[2], rng.randbytes(span))])
    tail += 16
    run_checked(queue, model, [("read", at[2], span), ("read", at[2] - 512, 512),
                               ("read", at[2] + span, 512)])
    report("ring_end", queue, model, tail=tail + 10)
    assert tail > 2 * RING


@pytest.mark.timeout(60)
def test_two_queues_cross_visibility(monkeypatch):
    """Two queues on one persistent bdev are two service kernels. 64
    tiles written through one must be what the other, and bdev.read's
    own channel, read once run() has returned: a payload store left
    dirty in one XCD's L2 would show here. Eight rounds over the same
    lines, a fresh pattern each. About 20 s: bdev.read frees a pinned
    buffer, which waits for both service kernels' idle exit (~1 s), in
    every round."""
    bdev, qa = make_queue("persistent", monkeypatch, "rb-cross")
    qb = hs.IoQueue(bdev)
    assert qb.kind == "persistent"
    model = ByteModel(bdev.size_bytes)
    base = 8 * MIB
    for round_no in range(8):
        rng = random.Random(4400 + round_no)
        writes = [("write", base + i * TILE, rng.randbytes(TILE))
                  for i in range(64)]
        run_checked(qa, model, writes)
        run_checked(qb, model, io_model.readback(writes))
        want = bytes(model.data[base:base + 64 * TILE])
        assert bdev.read(base, 64 * TILE) == want, round_no
    report("cross_visibility", qb, model)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("engine", RESIDENT)
def test_relaunch_replays_runs(engine, monkeypatch):
    """The service kernel idle-exits while the channel lives; the next
    run(), whose first request is multi-tile, restarts it from the
    completed prefix and the runs claimed from there carry the right
    bytes."""
    bdev, queue = make_queue(engine, monkeypatch, f"rb-relaunch-{engine}",
                             workers=2, batch=8)
    model = ByteModel(bdev.size_bytes)
    gen = OpGenerator(bdev.size_bytes, seed=55)
    first = gen.batch(17)
    run_checked(queue, model, first)
    before = hs.persistent_stats()
    time.sleep(2.5)  # beyond the idle exit
    second = [gen.make("write", 65536 + 1536)] + gen.batch(16)
    second += [("read", op[1], io_model.op_length(op)) for op in first[:8]]
    run_checked(queue, model, second)
    after = hs.persistent_stats()
    run_checked(queue, model, io_model.readback(first + second)
                + io_model.guard_reads(first + second))
    counter = "relaunches" if engine == "persistent" else "launches"
    report("relaunch", queue, model, counter=counter,
           before=before[counter], after=after[counter])
    assert after[counter] > before[counter], (before, after)
