"""Times hs.bdev_diff (k_diff_granules, granule 4096) against the
existing hs.hbm_copy (k_copy_range) over the same extent of two HBM
bdevs. Both move the same number of bytes across HBM (the copy reads N
and writes N, the diff reads 2N), so the unchanged copy kernel is the
yardstick. Runs alternate in one process; prints medians, min-max
spreads and the implied bytes/s as one JSON line.

    python tools/diff_bench.py [--gib 8] [--runs 7] [--granule 4096]

Host clock around calls that end in a stream synchronise (both calls
also create and destroy a stream, which is part of either figure).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oim_amd._hipstore as hs  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(samples, hbm_bytes):
    med = statistics.median(samples)
    return {"median_ms": round(med * 1e3, 3),
            "min_ms": round(min(samples) * 1e3, 3),
            "max_ms": round(max(samples) * 1e3, 3),
            "spread_ms": round((max(samples) - min(samples)) * 1e3, 3),
            "hbm_bytes_per_s": round(hbm_bytes / med)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gib", type=float, default=8.0,
                    help="size of each of the two bdevs")
    ap.add_argument("--runs", type=int, default=7, help="timed runs of each")
    ap.add_argument("--granule", type=int, default=4096)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if not hs.gpu_available():
        sys.exit("diff_bench: no HIP device (no fallback)")

    block = 512  # any granule that is a multiple of 512 is allowed
    blocks = int(args.gib * (1 << 30)) // block
    length = blocks * block // args.granule * args.granule
    a = hs.create_hbm_bdev("diffbench-a", block, blocks, device=args.device)
    b = hs.create_hbm_bdev("diffbench-b", block, blocks, device=args.device)

    def copy():
        hs.hbm_copy(a, 0, b, 0, length)

    result = {}

    def diff():
        result.update(hs.bdev_diff(a, b, length=length,
                                   granule=args.granule, max_report=0))

    # Make the pair identical (and non-trivial), then warm both paths.
    a.fill(0, 0x5A, min(length, 1 << 30))
    copy()
    for _ in range(2):
        diff()
        copy()
    if result["mismatched"] != 0:
        sys.exit(f"diff_bench: copies differ: {result['mismatched']}")

    diff_s, copy_s = [], []
    for _ in range(args.runs):  # alternate: both see the same neighbours
        diff_s.append(timed(diff))
        copy_s.append(timed(copy))
    d = summary(diff_s, 2 * length)
    c = summary(copy_s, 2 * length)
    print(json.dumps({
        "bytes_per_side": length, "granule": args.granule,
        "granules": result["granules"], "runs": args.runs,
        "bdev_diff": d, "hbm_copy": c,
        "diff_minus_copy_median_ms": round(d["median_ms"] - c["median_ms"], 3),
        "within_copy_spread":
            d["median_ms"] <= c["median_ms"] + c["spread_ms"],
    }))


if __name__ == "__main__":
    main()
