"""The host side of the HBM submit path on the GPU.

I/O statistics are kept in per-thread shards, and I/O buffers inside a
range the process pinned itself are translated from a registry instead
of by a runtime call per tile. The first must stay exact; a stale entry
of the second is a wrong address handed to the GPU, so its logic is
proven without a GPU first (tests/test_submit_path.py and the
stand-alone program) and only its use is exercised here. Bytes and
counts are right or wrong: nothing has a tolerance.

The bindings offer no way to submit from memory pinned outside
alloc_pinned, so the fallback to the runtime's translation has no case
of its own here; the vhost GPU tests run on registered guest memory.
"""

import json
import os
import random
import subprocess
import sys

import pytest

from oim_amd import _hipstore as hs

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not hs.gpu_available(), reason="no HIP device"),
]

MIB = 1 << 20
SIZES = (4096, 12 * 1024 + 16, 64 * 1024, MIB)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", ("persistent", "shared"))
def test_iostat_exact(engine):
    """4 queues x QD 8 x 2000 reads of 4 KiB on each resident engine:
    the statistics equal the I/O count the session returned, and the
    bytes are ops x 4096 (a child process per engine:
    tests/submit_path_child.py says why)."""
    script = os.path.join(os.path.dirname(__file__), "submit_path_child.py")
    env = dict(os.environ)
    env["GPU_MAX_HW_QUEUES"] = "24"   # one per service kernel, and spare
    if engine == "shared":
        env["HIPSTORE_SHARED"] = "1"
    else:
        env.pop("HIPSTORE_SHARED", None)
    proc = subprocess.run([sys.executable, script, engine], env=env,
                          capture_output=True, text=True, timeout=100)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    result = json.loads(proc.stdout.strip().splitlines()[-1])
    print("submit-path iostat " + json.dumps(result), flush=True)
    assert result["ok"] is True, result
    assert result["kind"] == engine
    assert result["after"]["num_read_ops"] == result["io_count"] == 8000
    assert result["after"]["bytes_read"] == 8000 * 4096


@pytest.mark.timeout(120)
@pytest.mark.parametrize("engine", ("batched", "persistent"))
def test_roundtrip_through_changing_buffers(engine, monkeypatch):
    """32 times: a seeded pattern of 4 KiB, 12 KiB + 16 B (three whole
    tiles and a 16-byte one), 64 KiB or 1 MiB written at a seeded offset
    of a 64 MiB bdev from a freshly pinned buffer and read back into
    another, both freed afterwards. The allocator hands addresses back,
    so ranges leave the registry and return at the same host address.

    On the batched engine a queue is held open all the while and moves
    a tile of its own after every round: one channel whose remembered
    range has to survive, and be checked against, every change of the
    registry. (A held queue of a resident engine would make each free
    wait for its service kernel's idle exit.)"""
    monkeypatch.delenv("HIPSTORE_SHARED", raising=False)
    bdev = hs.create_hbm_bdev(f"sp-buffers-{engine}", 16, 64 * MIB // 16,
                              device=0, persistent=engine != "batched")
    held = hs.IoQueue(bdev) if engine == "batched" else None
    if held is None:
        probe = hs.IoQueue(bdev)
        assert probe.kind == engine
        del probe
    else:
        assert held.kind == engine
    rng = random.Random(20260)
    low = 32 * MIB          # the rounds write below, the held queue above
    for round_no in range(32):
        size = SIZES[round_no % len(SIZES)]
        offset = rng.randrange(0, (low - size) // 16) * 16
        pattern = rng.randbytes(size)
        bdev.write(offset, pattern)
        assert bdev.read(offset, size) == pattern, (round_no, size, offset)
        if held is not None:
            at = low + rng.randrange(0, (low - 4096) // 16) * 16
            tile = rng.randbytes(4096)
            assert held.run([("write", at, tile)]) == [(0, None)]
            assert held.run([("read", at, 4096)]) == [(0, tile)], round_no
    print(f"submit-path buffers kind={engine} rounds=32", flush=True)
