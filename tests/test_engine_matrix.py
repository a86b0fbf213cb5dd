"""Queued I/O on every HBM engine against a byte model.

The benchmark drives the three engines (batched k_copy_blocks,
per-queue k_persistent_copy, shared k_shared_service) with many
requests in flight on long-lived channels; bdev.read/write/fill keep
one request in flight on a throw-away channel. These tests use
hs.IoQueue — one held channel, a whole list of requests submitted
before the first poll — and compare every byte with tests/io_model.py.
No tolerances anywhere: a byte is right or wrong.

Each test first asserts `queue.kind`, so a change in the fallback rules
cannot silently move a test onto another engine. Every test prints one
`engine-matrix` line (kind, ops and tiles verified, launch counters)
for the record; run with -s to see them.
"""

import json
import os
import subprocess
import sys
import threading
import time

import pytest

from oim_amd import _hipstore as hs

import io_model
from io_model import ByteModel, OpGenerator, run_checked

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device"),
]

ENGINES = ("batched", "persistent", "shared")
RESIDENT = ("persistent", "shared")

MIB = 1 << 20
RESIDENT_RING = 32768   # descriptors per resident-engine channel
BATCHED_RING = 65536    # descriptor slots per batched channel


def make_bdev(engine, monkeypatch, name, size_bytes):
    """512-byte-block HBM bdev whose channels land on `engine`."""
    if engine == "shared":
        # Read by the bdev constructor on every call.
        monkeypatch.setenv("HIPSTORE_SHARED", "1")
    else:
        monkeypatch.delenv("HIPSTORE_SHARED", raising=False)
    return hs.create_hbm_bdev(name, 512, size_bytes // 512, device=0,
                              persistent=engine != "batched")


def make_queue(engine, bdev):
    queue = hs.IoQueue(bdev)
    assert queue.kind == engine
    return queue


def report(test, queue, model, **extra):
    fields = dict(kind=queue.kind, ops=model.ops_checked,
                  tiles=model.tiles_checked, **extra)
    print("engine-matrix " + test + " "
          + " ".join(f"{k}={v}" for k, v in fields.items()), flush=True)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", ENGINES)
def test_perf_session_step_counts(engine, monkeypatch):
    """The benchmark's per-queue driver on each engine. Every count
    follows from per_queue_ios = ceil(total / num_queues) in
    PerfSession::step with two queues of depth 4; nothing is measured.

    First in the file on purpose: the two per-queue service kernels of
    the persistent case come up in 1.5 s here, but took 5.3 s (before
    and after the driver was shared) when they started right after the
    shared-engine cases of the tests below."""
    bdev = make_bdev(engine, monkeypatch, f"em-perf-{engine}", 8 * MIB)
    queue = make_queue(engine, bdev)
    del queue
    session = hs.PerfSession(bdev, "randrw", 4096, 4, 2)
    # 2 x 5: one more than the queue depth, so each queue resubmits
    # from a completion callback.
    assert session.step(10)["io_count"] == 10
    # 2 x 2: a target below the queue depth fills only part of the queue.
    assert session.step(3)["io_count"] == 4
    assert session.step(10)["io_count"] == 10
    print(f"engine-matrix perf_session kind={engine} steps=10,3,10",
          flush=True)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", ENGINES)
def test_tile_edges(engine, monkeypatch):
    bdev = make_bdev(engine, monkeypatch, f"em-edge-{engine}", 64 * MIB)
    queue = make_queue(engine, bdev)
    model = ByteModel(bdev.size_bytes)
    io_model.scenario_tile_edges(queue, model, seed=101)
    report("tile_edges", queue, model)
    del queue
    # Whole bdev through fresh channels: nothing outside the ops moved.
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", ENGINES)
def test_mixed_batch(engine, monkeypatch):
    bdev = make_bdev(engine, monkeypatch, f"em-mixed-{engine}", 64 * MIB)
    queue = make_queue(engine, bdev)
    model = ByteModel(bdev.size_bytes)
    io_model.scenario_mixed_batch(queue, model, seed=202)
    report("mixed_batch", queue, model)
    del queue
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", RESIDENT)
def test_ring_wrap(engine, monkeypatch):
    """More than 32768 tiles through ONE live channel, and more than
    32768 in a single run(): has_capacity() refuses, requests wait in
    pending_ and drain from poll(), and ring indices wrap (twice, with
    the read-back on the same queue)."""
    bdev = make_bdev(engine, monkeypatch, f"em-wrap-{engine}", 256 * MIB)
    queue = make_queue(engine, bdev)
    model = ByteModel(bdev.size_bytes)
    # Start from a tail that is not a multiple of anything convenient.
    io_model.scenario_tile_edges(queue, model, seed=303)

    fills = 40
    gen = OpGenerator(bdev.size_bytes, seed=304, lo=176 * MIB)
    big = []
    for i in range(fills):
        # 4 MiB = 1024 tiles each, contiguous, block- but not
        # tile-aligned, every fill its own value (1..40).
        big.append(("fill", 160 * MIB - 512 - (i + 1) * 4 * MIB + 1024,
                    4 * MIB, i + 1))
        big.append(gen.make("write", io_model.EDGE_LENGTHS[i % 8]))
    big_tiles = sum(io_model.op_tiles(op) for op in big)
    assert big_tiles > RESIDENT_RING
    run_checked(queue, model, big)
    # Read everything back on the SAME queue: another > 32768 tiles.
    run_checked(queue, model,
                io_model.readback(big) + io_model.guard_reads(big))
    assert model.tiles_checked > 2 * RESIDENT_RING
    report("ring_wrap", queue, model, single_run_tiles=big_tiles,
           wrapped=model.tiles_checked // RESIDENT_RING)


@pytest.mark.timeout(120)
def test_ring_pressure_batched(monkeypatch):
    """One run() of more than 65536 tiles on the batched engine with a
    ring head that is not aligned to the request sizes: kick() hits
    both `n + tiles > cap` (a batch never wraps, and is capped at a
    quarter ring) and `take == 0` (head at 61445 after four fills: the
    fifth 15360-tile fill does not fit before the end of the ring, so
    it waits until the ring empties and the head snaps back to 0)."""
    bdev = make_bdev("batched", monkeypatch, "em-press", 320 * MIB)
    queue = make_queue("batched", bdev)
    kind = queue.kind
    model = ByteModel(bdev.size_bytes)
    gen = OpGenerator(bdev.size_bytes, seed=404, lo=301 * MIB,
                      lengths=(4096, 12288))
    ops = [gen.make("write", 4096), gen.make("write", 12288),
           gen.make("fill", 4096, value=0xFF)]          # head = 5
    fill_len = 60 * MIB                                   # 15360 tiles
    fills = [("fill", i * fill_len, fill_len, 0x10 + i) for i in range(5)]
    ops += fills
    ops += [gen.make("write", 12288), ("flush",)]
    total = sum(io_model.op_tiles(op) for op in ops)
    assert total > BATCHED_RING
    run_checked(queue, model, ops)

    # Exact: first and last block of every op, neighbours of the small
    # ones, and the small ops whole.
    small = [op for op in ops if op[0] != "flush" and op not in fills]
    probes = io_model.readback(small) + io_model.guard_reads(small)
    for op in fills:
        probes.append(("read", op[1], 512))
        probes.append(("read", op[1] + fill_len - 512, 512))
    probes.append(("read", 5 * fill_len, 512))            # just past fill 4
    run_checked(queue, model, probes)
    del queue
    # Bulk of the large fills: GPU per-4 KiB CRCs against the table CRC
    # of the expected block (every block of one fill is identical).
    for op in fills:
        want = hs.crc32c_table(bytes([op[3]]) * 4096)
        crcs = hs.crc32c_gpu_blocks(bdev, op[1], 4096, fill_len // 4096)
        assert len(crcs) == fill_len // 4096
        bad = [i for i, crc in enumerate(crcs) if crc != want]
        assert not bad, (op[3], bad[:8], len(bad))
    print(f"engine-matrix ring_pressure kind={kind} "
          f"ops={model.ops_checked} tiles={model.tiles_checked} "
          f"single_run_tiles={total} crc_blocks={5 * (fill_len // 4096)}",
          flush=True)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", RESIDENT)
def test_relaunch_on_live_channel(engine, monkeypatch):
    """The service kernel idle-exits (~1 s) while the channel stays
    alive; the next run() on the SAME queue must restart it from
    poll() with a non-zero completed prefix (per-queue: launch() with
    claim = known_tail = completed_; shared: ensure_running_locked
    re-seeding every slot from prefix_[])."""
    bdev = make_bdev(engine, monkeypatch, f"em-relaunch-{engine}", 64 * MIB)
    queue = make_queue(engine, bdev)
    model = ByteModel(bdev.size_bytes)
    gen = OpGenerator(bdev.size_bytes, seed=505)
    first = gen.batch(17)
    run_checked(queue, model, first)
    before = hs.persistent_stats()
    time.sleep(2.5)  # beyond the idle exit
    second = gen.batch(17, kinds=("fill", "write"))
    second += [("read", op[1], io_model.op_length(op)) for op in first[:8]]
    run_checked(queue, model, second)
    after = hs.persistent_stats()
    run_checked(queue, model, io_model.readback(first + second)
                + io_model.guard_reads(first + second))
    counter = "relaunches" if engine == "persistent" else "launches"
    report("relaunch", queue, model, counter=counter,
           before=before[counter], after=after[counter])
    assert after[counter] > before[counter], (before, after)


@pytest.mark.timeout(120)
def test_two_queues_two_threads(monkeypatch):
    """Two live per-queue channels on one bdev, driven from two Python
    threads (run() releases the GIL), each on its own half."""
    bdev = make_bdev("persistent", monkeypatch, "em-two", 128 * MIB)
    half = bdev.size_bytes // 2
    queues = [make_queue("persistent", bdev) for _ in range(2)]
    models = [ByteModel(bdev.size_bytes) for _ in range(2)]
    errors = []

    def worker(index):
        try:
            gen = OpGenerator(bdev.size_bytes, seed=600 + index,
                              lo=index * half, hi=(index + 1) * half)
            written = []
            for _ in range(3):
                ops = gen.batch(80, kinds=("write", "fill"))
                ops += [("read", op[1], io_model.op_length(op))
                        for op in written[-40:]]
                run_checked(queues[index], models[index], ops)
                written += ops[:80]
            run_checked(queues[index], models[index],
                        io_model.readback(written)
                        + io_model.guard_reads(written))
        except BaseException as exc:  # surfaced in the main thread
            errors.append((index, exc))

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join(90)
        assert not thread.is_alive(), "queue thread did not finish"
    if errors:
        raise errors[0][1]
    for index in range(2):
        report(f"two_queues[{index}]", queues[index], models[index])
    del queues
    for index in range(2):
        lo = index * half
        assert bdev.read(lo, half) == bytes(models[index].data[lo:lo + half])


@pytest.mark.timeout(150)
@pytest.mark.parametrize("fallback", ["shared", "batched"])
def test_cross_engine_read_after_write(fallback):
    """A per-queue channel and a fallback channel on one bdev, each
    reading what the other wrote (HIPSTORE_PERQ_CAP is cached in a
    static, hence the child process)."""
    script = os.path.join(os.path.dirname(__file__), "engine_cross_child.py")
    env = dict(os.environ, HIPSTORE_PERQ_CAP="1")
    env.pop("HIPSTORE_SHARED", None)
    if fallback == "batched":
        env["HIPSTORE_FALLBACK"] = "batched"
    else:
        env.pop("HIPSTORE_FALLBACK", None)
    proc = subprocess.run([sys.executable, script, fallback], env=env,
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    print("engine-matrix cross_engine " + json.dumps(result), flush=True)
    assert result["ok"] is True, result
    assert result["kinds"] == ["persistent", fallback]
    assert result["fresh_channel_kind"] == fallback
    assert result["ops"] > 0 and result["tiles"] > 0
