"""Child process of test_engine_matrix.py::test_cross_engine_read_after_write.

Run with HIPSTORE_PERQ_CAP=1 (and optionally HIPSTORE_FALLBACK=batched):
the first channel of a persistent bdev is served by the per-queue
resident kernel, every further one by the fallback engine named in
argv[1]. Each side then reads what the other wrote — plain stores of a
resident kernel followed by another engine's loads, and the reverse —
including overwrites of lines the reader has already loaded once.
Prints one JSON line; exit status 0 only when every byte matched.
"""

import json
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oim_amd import _hipstore as hs  # noqa: E402

import io_model  # noqa: E402
from io_model import run_checked  # noqa: E402


def overwrite(gen, ops):
    """New contents for the ranges of `ops`: writes become fills and
    fills become writes, same offsets and lengths."""
    return [gen.make("fill" if op[0] == "write" else "write",
                     io_model.op_length(op), at=op[1]) for op in ops]


def exchange(writer, reader, model, gen, bdev):
    """`writer` writes, `reader` reads it; then `writer` overwrites what
    `reader` has just loaded and `reader` reads again."""
    ops = gen.batch(17)
    run_checked(writer, model, ops)
    look = io_model.readback(ops) + io_model.guard_reads(ops)
    run_checked(reader, model, look)
    run_checked(writer, model, overwrite(gen, ops))
    run_checked(reader, model, look)
    # And through a throw-away channel: the whole bdev in one read (a
    # pinned bounce buffer freed under a live service kernel waits for
    # its idle exit, so one large read, not one per range).
    assert bdev.read(0, bdev.size_bytes) == bytes(model.data)


def main():
    fallback = sys.argv[1]
    result = {"ok": False}
    try:
        bdev = hs.create_hbm_bdev("em-cross", 512, (64 << 20) // 512,
                                  device=0, persistent=True)
        qa = hs.IoQueue(bdev)
        qb = hs.IoQueue(bdev)
        result["kinds"] = [qa.kind, qb.kind]
        if result["kinds"] != ["persistent", fallback]:
            raise AssertionError(f"unexpected engines {result['kinds']}")
        probe = hs.IoQueue(bdev)       # what bdev.read's channels get
        result["fresh_channel_kind"] = probe.kind
        del probe
        model = io_model.ByteModel(bdev.size_bytes)
        gen = io_model.OpGenerator(bdev.size_bytes, seed=707)
        exchange(qa, qb, model, gen, bdev)   # per-queue writes first
        exchange(qb, qa, model, gen, bdev)   # fallback writes first
        result.update(ok=True, ops=model.ops_checked,
                      tiles=model.tiles_checked, stats=hs.persistent_stats())
    except BaseException as exc:
        result["error"] = f"{type(exc).__name__}: {exc}"
        traceback.print_exc()
    print(json.dumps(result), flush=True)
    return 0 if result["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
