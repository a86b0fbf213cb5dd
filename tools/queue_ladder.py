"""Queue ladder of the resident per-queue engine: where one queue of
k_persistent_copy saturates, and what bounds it.

Drives hs.PerfSession (the benchmark's per-queue driver) with 4 KiB
random reads, unless the shape says otherwise, on an 8 GiB persistent
HBM bdev and prints one JSON line per shape:

    q1_qd1 .. q1_qd64        1 queue at QD 1 / 4 / 16 / 32 / 64
    q4_qd32_4k, q4_qd32_64k  4 queues, QD 32, 4 KiB and 64 KiB
    q14_qd32_512, q14_qd32_4k  14 queues, QD 32, 512 B and 4 KiB
    q1_qd64_w4 / w8 / w16    1 queue, QD 64, HIPSTORE_PERSISTENT_WORKERS
                             4 / 8 / 16: IOPS that scale with the
                             workers mean the queue is worker-bound

    python tools/queue_ladder.py [--steps 7] [--warmup 2] [--shapes NAME ...]

Every shape runs in a process of its own (the engine's knobs are read
from the environment, some of them once per process), which sets
GPU_MAX_HW_QUEUES and HIPSTORE_AFFINITY_BASE the way bench.py does.
HIPSTORE_BATCH_TILES and the other engine knobs are passed through from
the caller's environment and echoed in the line. Each line holds the
median and the min-max of the steps' IOPS, the same as GB/s, and the
median of the steps' p50 and p99 latency. Measurement only; needs a GPU:
there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> queues, queue depth, I/O bytes, I/Os per step, worker waves
SHAPES = {
    "q1_qd1": (1, 1, 4096, 8192, None),
    "q1_qd4": (1, 4, 4096, 32768, None),
    "q1_qd16": (1, 16, 4096, 65536, None),
    "q1_qd32": (1, 32, 4096, 65536, None),
    "q1_qd64": (1, 64, 4096, 65536, None),
    "q4_qd32_4k": (4, 32, 4096, 131072, None),
    "q4_qd32_64k": (4, 32, 65536, 16384, None),
    "q14_qd32_512": (14, 32, 512, 262144, None),
    "q14_qd32_4k": (14, 32, 4096, 131072, None),
    "q1_qd64_w4": (1, 64, 4096, 65536, 4),
    "q1_qd64_w8": (1, 64, 4096, 65536, 8),
    "q1_qd64_w16": (1, 64, 4096, 65536, 16),
}


def spread(values, digits=0):
    return {"median": round(statistics.median(values), digits),
            "min": round(min(values), digits),
            "max": round(max(values), digits)}


def run_shape(name, steps, warmup):
    queues, depth, io_size, step_ios, _ = SHAPES[name]
    # Before HIP initialises: one hardware queue per service kernel, and
    # the queue threads pinned, as in bench.py.
    os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("HIPSTORE_HW_QUEUES",
                                                     "24")
    if (os.cpu_count() or 1) >= queues + 2:
        os.environ.setdefault("HIPSTORE_AFFINITY_BASE", "0")
    sys.path.insert(0, REPO_ROOT)
    import oim_amd._hipstore as hs

    if not hs.gpu_available():
        sys.exit("queue_ladder: no HIP device (no fallback)")
    bdev = hs.create_hbm_bdev("ladder", 512, (8 << 30) // 512, device=0,
                              persistent=True)
    session = hs.PerfSession(bdev, "randread", io_size, depth, queues)
    for _ in range(warmup):
        session.step(step_ios)
    results = [session.step(step_ios) for _ in range(steps)]
    iops = [r["iops"] for r in results]
    print(json.dumps({
        "shape": name, "queues": queues, "queue_depth": depth,
        "io_size": io_size, "steps": steps, "step_ios": step_ios,
        "workers": os.environ.get("HIPSTORE_PERSISTENT_WORKERS", "16"),
        "batch_tiles": os.environ.get("HIPSTORE_BATCH_TILES", "default"),
        "iops": spread(iops),
        "gb_per_s": spread([v * io_size / 1e9 for v in iops], 2),
        "p50_us": round(statistics.median(r["lat_p50_us"]
                                          for r in results), 2),
        "p99_us": round(statistics.median(r["lat_p99_us"]
                                          for r in results), 2),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=7, help="timed steps")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", nargs="+", choices=list(SHAPES),
                    default=list(SHAPES))
    ap.add_argument("--child", choices=list(SHAPES), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 3:
        ap.error("--steps must be at least 3")
    if args.child:
        run_shape(args.child, args.steps, args.warmup)
        return 0
    status = 0
    for name in args.shapes:
        env = dict(os.environ)
        workers = SHAPES[name][4]
        if workers is not None:
            env["HIPSTORE_PERSISTENT_WORKERS"] = str(workers)
        proc = subprocess.run(
            [sys.executable, os.path.abspath(__file__), "--child", name,
             "--steps", str(args.steps), "--warmup", str(args.warmup)],
            env=env, timeout=120)
        if proc.returncode != 0:
            print(json.dumps({"shape": name, "error": proc.returncode}),
                  flush=True)
            status = 1
            break   # a failed GPU process: start nothing more
    return status


if __name__ == "__main__":
    sys.exit(main())
