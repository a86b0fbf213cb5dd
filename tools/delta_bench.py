"""Times the marked gather of an HBM volume (k_pack_marked) and a delta
export built on it against plain hipMemcpyAsync, at 1 %, 10 % and 100 %
of the granules marked (seeded random choice).

    python tools/delta_bench.py [--gib 8] [--granule 4096] [--runs 5]
                                [--dir /dev/shm]

Per shape, in one process, alternating:
  pack          bdev_pack_marked_sync with a sink that discards
  memcpy_once   hipMemcpyAsync of the same byte count, device to pinned
                host (the PCIe ceiling)
  memcpy_runs   one hipMemcpyAsync per run of marked granules (what the
                kernel replaces)
  export        bdev_export_delta against a base that differs in exactly
                the marked granules, to a file under --dir (a tmpfs);
                includes the compare, the CRCs and the file writes
The first three are timed natively (hs.marked_copy_probe: host clock
from the first enqueue to the end of a stream synchronise), the export
around the Python call. One warm-up of each, then medians with min-max.
Prints one JSON line per shape. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oim_amd._hipstore as hs  # noqa: E402

FILL_STEP = 1 << 30


def fill(bdev, value, length):
    for off in range(0, length, FILL_STEP):
        bdev.fill(off, value, min(FILL_STEP, length - off))


def summary(samples, nbytes):
    med = statistics.median(samples)
    return {"median_ms": round(med * 1e3, 3),
            "min_ms": round(min(samples) * 1e3, 3),
            "max_ms": round(max(samples) * 1e3, 3),
            "gb_per_s": round(nbytes / med / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gib", type=float, default=8.0, help="volume size")
    ap.add_argument("--granule", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--export-runs", type=int, default=3)
    ap.add_argument("--percent", type=float, nargs="+",
                    default=[1.0, 10.0, 100.0])
    ap.add_argument("--dir", default="/dev/shm", help="where exports go")
    ap.add_argument("--staging-mib", type=int, default=0,
                    help="staging buffer of the pack runs (0 = default)")
    ap.add_argument("--modes", nargs="+", default=[
        "pack", "memcpy_once", "memcpy_runs", "export"])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not hs.gpu_available():
        sys.exit("delta_bench: no HIP device (no fallback)")

    block = 512
    n = int(args.gib * (1 << 30)) // args.granule
    length = n * args.granule
    live = hs.create_hbm_bdev("deltabench-live", block, length // block,
                              device=args.device)
    base = hs.create_hbm_bdev("deltabench-base", block, length // block,
                              device=args.device)
    fill(base, 0x11, length)
    path = os.path.join(args.dir, f"deltabench-{os.getpid()}.delta")
    rng = np.random.default_rng(20263)

    for percent in args.percent:
        k = max(1, round(n * percent / 100))
        bits = np.zeros(n, dtype=np.uint8)
        if k >= n:
            bits[:] = 1
        else:
            bits[rng.permutation(n)[:k]] = 1
        runs = int(np.count_nonzero(np.diff(bits, prepend=0) == 1))
        bitmap = np.packbits(bits, bitorder="little").tobytes()
        nbytes = k * args.granule
        # live = base everywhere but in the marked granules
        fill(live, 0x11, length)
        if k >= n:
            fill(live, 0x5A, length)
        else:
            hs.bdev_unpack_marked(live, bitmap, args.granule,
                                  bytes([0x5A]) * nbytes)

        def probe(mode):
            r = hs.marked_copy_probe(live, bitmap, args.granule, mode,
                                     staging_bytes=args.staging_mib << 20)
            assert r["granules"] == k, r
            return r["seconds"]

        def export():
            if os.path.exists(path):
                os.unlink(path)  # never two copies in the tmpfs
            t0 = time.perf_counter()
            r = hs.bdev_export_delta(live, path, base=base,
                                     granule=args.granule)
            dt = time.perf_counter() - t0
            assert r["marked"] == k, r
            return dt

        samples = {name: [] for name in args.modes}
        modes = [(name, mode) for name, mode in
                 (("pack", 2), ("memcpy_runs", 1), ("memcpy_once", 0))
                 if name in args.modes]
        for _, mode in modes:  # warm-up
            probe(mode)
        for _ in range(args.runs):
            for name, mode in modes:
                samples[name].append(probe(mode))
        out = {"volume_bytes": length, "granule": args.granule,
               "percent": percent, "marked": k, "runs_of_marked": runs,
               "marked_bytes": nbytes}
        if "export" in args.modes:
            export()
            for _ in range(args.export_runs):
                samples["export"].append(export())
            out["file_bytes"] = os.path.getsize(path)
            os.unlink(path)
        for name, values in samples.items():
            out[name] = summary(values, nbytes)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
