"""Times the fingerprint pass of an HBM bdev (hs.bdev_fingerprint,
k_fingerprint_granules) at several granule sizes against hs.bdev_diff
(k_diff_granules): the same access pattern, one wave per granule and
16 B per lane, without the hash arithmetic. The diff runs twice: of the
volume with an identical clone (the yardstick of tools/diff_bench.py,
two streams from HBM) and of the volume with itself (the same unique
bytes from HBM as the fingerprint pass; its second read of an address
hits the caches). All are reported as bytes read per second, the diffs
counting both sides. Then changes 1 % of the granules and times a delta
export against the volume's fingerprint map (base_map) and against the
clone (base), end to end, files included. Prints one JSON line.

    python tools/fingerprint_bench.py [--gib 8] [--runs 7] [--dir /tmp]

Host clock around calls that end in a stream synchronise (every call
also creates and destroys a stream, which is part of either figure).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
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
            "read_bytes_per_s": round(hbm_bytes / med)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gib", type=float, default=8.0, help="volume size")
    ap.add_argument("--runs", type=int, default=7, help="timed runs of each")
    ap.add_argument("--granules", type=int, nargs="+",
                    default=[512, 4096, 65536])
    ap.add_argument("--delta-granule", type=int, default=4096)
    ap.add_argument("--dir", default=None, help="where the files go")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if not hs.gpu_available():
        sys.exit("fingerprint_bench: no HIP device (no fallback)")

    block = 512
    unit = max(args.granules + [args.delta_granule])
    blocks = int(args.gib * (1 << 30)) // unit * unit // block
    length = blocks * block
    vol = hs.create_hbm_bdev("fpbench", block, blocks, device=args.device)
    # Non-trivial content: a random piece, doubled up by device copies.
    have = min(length, 8 << 20)
    vol.write(0, random.Random(1).randbytes(have))
    while have < length:
        step = min(have, length - have)
        hs.hbm_copy(vol, 0, vol, have, step)
        have += step
    clone = hs.create_hbm_bdev("fpbench-base", block, blocks,
                               device=args.device)
    hs.hbm_copy(vol, 0, clone, 0, length)

    out = {"bytes": length, "runs": args.runs, "granule": {}}
    for granule in args.granules:
        def fingerprint():
            hs.bdev_fingerprint(vol, granule, keep=False)

        def diff():
            hs.bdev_diff(vol, clone, granule=granule, max_report=0)

        def diff_self():
            hs.bdev_diff(vol, vol, granule=granule, max_report=0)

        for _ in range(2):
            fingerprint()
            diff()
            diff_self()
        fp_s, diff_s, self_s = [], [], []
        for _ in range(args.runs):  # alternate: all see the same neighbours
            fp_s.append(timed(fingerprint))
            diff_s.append(timed(diff))
            self_s.append(timed(diff_self))
        f = summary(fp_s, length)
        d = summary(diff_s, 2 * length)
        out["granule"][str(granule)] = {
            "bdev_fingerprint": f, "bdev_diff": d,
            "bdev_diff_with_itself": summary(self_s, 2 * length),
            "fingerprint_over_diff_rate":
                round(f["read_bytes_per_s"] / d["read_bytes_per_s"], 3)}

    # 1 % changed: delta against the map, against a clone.
    granule = args.delta_granule
    n = length // granule
    with tempfile.TemporaryDirectory(dir=args.dir) as tmp:
        map_path = os.path.join(tmp, "v.map")
        delta = os.path.join(tmp, "v.delta")
        t_map = timed(lambda: hs.bdev_fingerprint_file(vol, map_path,
                                                       granule=granule))
        changed = random.Random(2).sample(range(n), max(1, n // 100))
        bitmap = bytearray((n + 7) // 8)
        for g in changed:
            bitmap[g // 8] |= 1 << (g % 8)
        hs.bdev_unpack_marked(vol, bytes(bitmap), granule,
                              b"\xC3" * (len(changed) * granule))
        by_map, by_clone = [], []
        saved = set()
        for _ in range(args.runs):
            by_map.append(timed(lambda: saved.add(hs.bdev_export_delta(
                vol, delta, base_map=map_path, overwrite=True)["marked"])))
            by_clone.append(timed(lambda: saved.add(hs.bdev_export_delta(
                vol, delta, base=clone, granule=granule,
                overwrite=True)["marked"])))
        out["delta_1pct"] = {
            "granule": granule, "granules": n, "saved": sorted(saved),
            "map_file_ms": round(t_map * 1e3, 3),
            "base_map_median_ms": round(statistics.median(by_map) * 1e3, 3),
            "base_clone_median_ms":
                round(statistics.median(by_clone) * 1e3, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
