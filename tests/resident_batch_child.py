"""Child process of test_resident_batching.py::test_batch_sizes.

argv[1] is the engine ("persistent" or "shared"). The parent sets
HIPSTORE_BATCH_TILES to the run length under test and the worker count
of both resident kernels to 2 (HIPSTORE_PERSISTENT_WORKERS,
HIPSTORE_SHARED_WORKERS): the shared service reads its knobs when its
one kernel per device is launched, so only a fresh process pins them.
With two workers a backlog of b tiles is claimed in runs of
min(K, ceil(b / 2)): the list sizes below give single tiles, a partial
last run and full runs. Prints one JSON line; exit status 0 only when
every byte matched.
"""

import json
import os
import random
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oim_amd import _hipstore as hs  # noqa: E402

import io_model  # noqa: E402
from io_model import run_checked  # noqa: E402

TILE_COUNTS = (1, 3, 5, 17, 64)


def main():
    engine = sys.argv[1]
    result = {"ok": False, "batch": os.environ.get("HIPSTORE_BATCH_TILES")}
    try:
        bdev = hs.create_hbm_bdev(f"rb-sizes-{engine}", 512, (64 << 20) // 512,
                                  device=0, persistent=True)
        queue = hs.IoQueue(bdev)
        result["kind"] = queue.kind
        if queue.kind != engine:
            raise AssertionError(f"unexpected engine {queue.kind}")
        model = io_model.ByteModel(bdev.size_bytes)
        rng = random.Random(909)
        tiles = rng.sample(range(bdev.size_bytes // io_model.TILE),
                           sum(TILE_COUNTS))
        for count in TILE_COUNTS:
            mine, tiles = tiles[:count], tiles[count:]
            writes = [("write", t * io_model.TILE,
                       rng.randbytes(io_model.TILE)) for t in mine]
            run_checked(queue, model, writes)
            run_checked(queue, model, io_model.readback(writes))
        del queue
        if bdev.read(0, bdev.size_bytes) != bytes(model.data):
            raise AssertionError("bdev differs from the model outside the ops")
        result.update(ok=True, ops=model.ops_checked,
                      tiles=model.tiles_checked)
    except BaseException as exc:
        result["error"] = f"{type(exc).__name__}: {exc}"
        traceback.print_exc()
    print(json.dumps(result), flush=True)
    return 0 if result["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
