"""Child process of test_submit_path_gpu.py::test_iostat_exact.

argv[1] is the resident engine ("persistent" or "shared"; the parent
sets HIPSTORE_SHARED for the latter, which the bdev reads when it is
created, and the hardware-queue count for the four service kernels of
the former, which the runtime reads when it starts). Four queue threads
at QD 8 read 4 KiB 2000 times each through hs.PerfSession; the bdev's
I/O statistics, summed over the threads' shards, must be exactly those
reads. Prints one JSON line; exit status 0 only when they are.
"""

import json
import os
import sys
import traceback

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oim_amd import _hipstore as hs  # noqa: E402

QUEUES, DEPTH, PER_QUEUE, IO = 4, 8, 2000, 4096


def main():
    engine = sys.argv[1]
    result = {"ok": False}
    try:
        bdev = hs.create_hbm_bdev(f"sp-iostat-{engine}", 512, (64 << 20) // 512,
                                  device=0, persistent=True)
        queue = hs.IoQueue(bdev)
        result["kind"] = queue.kind
        del queue
        if result["kind"] != engine:
            raise AssertionError(f"unexpected engine {result['kind']}")
        before = bdev.iostat()
        session = hs.PerfSession(bdev, "randread", IO, DEPTH, QUEUES)
        step = session.step(QUEUES * PER_QUEUE)
        del session
        after = bdev.iostat()
        result.update(io_count=step["io_count"], before=before, after=after)
        if any(before.values()):
            raise AssertionError(f"counted before any request: {before}")
        if step["io_count"] != QUEUES * PER_QUEUE:
            raise AssertionError(f"io_count {step['io_count']}")
        want = dict(num_read_ops=step["io_count"], num_write_ops=0,
                    num_unmap_ops=0, bytes_read=step["io_count"] * IO,
                    bytes_written=0)
        if after != want:
            raise AssertionError(f"iostat {after}, expected {want}")
        result["ok"] = True
    except BaseException as exc:
        result["error"] = f"{type(exc).__name__}: {exc}"
        traceback.print_exc()
    print(json.dumps(result), flush=True)
    return 0 if result["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
