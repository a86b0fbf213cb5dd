"""Times full exports and imports of an HBM volume with and without a
key, alternating in one process, and the XTS kernels on their own.

    python tools/crypt_bench.py [--gib 8] [--granule 4096] [--runs 5]
                                [--dir /dev/shm] [--no-key]

The volume holds seeded random bytes. One warm-up, then `runs` rounds of
export, export with a key, import and import of the encrypted file, each
timed around the Python call (the file is on --dir, a tmpfs). Then, per
round, the kernels alone: k_pack_marked (hs.marked_copy_probe mode 2),
k_xts_pack_marked and k_xts_unpack_marked (hs.xts_marked_probe), all
granules marked and nothing done with the dense stream, timed natively.
Prints one JSON line with medians, min-max and GB/s of volume bytes.
--no-key runs the unencrypted half only, which is all a build without
the feature has. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oim_amd._hipstore as hs  # noqa: E402

STEP = 64 << 20
KEY = bytes(range(64))


def summary(samples, nbytes):
    med = statistics.median(samples)
    return {"median_s": round(med, 4), "min_s": round(min(samples), 4),
            "max_s": round(max(samples), 4),
            "gb_per_s": round(nbytes / med / 1e9, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gib", type=float, default=8.0, help="volume size")
    ap.add_argument("--granule", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm", help="where exports go")
    ap.add_argument("--no-key", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if not hs.gpu_available():
        sys.exit("crypt_bench: no HIP device (no fallback)")

    block = 512
    length = int(args.gib * (1 << 30)) // args.granule * args.granule
    n = length // args.granule
    live = hs.create_hbm_bdev("xtsbench-live", block, length // block,
                              device=args.device)
    back = hs.create_hbm_bdev("xtsbench-back", block, length // block,
                              device=args.device)
    rng = np.random.default_rng(20265)
    for off in range(0, length, STEP):
        size = min(STEP, length - off)
        live.write(off, rng.integers(0, 256, size=size, dtype=np.uint8).tobytes())
    path = os.path.join(args.dir, f"xtsbench-{os.getpid()}.delta")
    modes = [False] if args.no_key else [False, True]
    all_marked = bytes([0xFF]) * (n // 8) + bytes([(1 << (n % 8)) - 1] * (n % 8 != 0))

    out = {"volume_bytes": length, "granule": args.granule}
    samples = {(what, xts): [] for what in ("export", "import")
               for xts in modes}
    kernels = {"k_pack_marked": [], "k_xts_pack_marked": [],
               "k_xts_unpack_marked": []}
    for run in range(args.runs + 1):  # run 0 warms up
        for xts in modes:
            if os.path.exists(path):
                os.unlink(path)  # never two copies in the tmpfs
            kwargs = {"key": KEY} if xts else {}
            t0 = time.perf_counter()
            hs.bdev_export_delta(live, path, granule=args.granule, **kwargs)
            t1 = time.perf_counter()
            hs.bdev_import_delta(back, path, **kwargs)
            t2 = time.perf_counter()
            if run > 0:
                samples[("export", xts)].append(t1 - t0)
                samples[("import", xts)].append(t2 - t1)
        took = {"k_pack_marked": hs.marked_copy_probe(
            live, all_marked, args.granule, 2)["seconds"]}
        if not args.no_key:
            took["k_xts_pack_marked"] = hs.xts_marked_probe(
                live, all_marked, args.granule, KEY)["seconds"]
        if run > 0:
            for name, seconds in took.items():
                kernels[name].append(seconds)
    if hs.bdev_diff(live, back, granule=args.granule)["mismatched"] != 0:
        sys.exit("crypt_bench: restored volume differs")
    os.unlink(path)
    # Last, since it overwrites `back` with whatever the staging held.
    for run in range(0 if args.no_key else args.runs + 1):
        seconds = hs.xts_marked_probe(back, all_marked, args.granule, KEY,
                                      unpack=True)["seconds"]
        if run > 0:
            kernels["k_xts_unpack_marked"].append(seconds)
    for (what, xts), values in samples.items():
        out[what + ("_xts" if xts else "")] = summary(values, length)
    for name, values in kernels.items():
        if values:
            out[name] = summary(values, length)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
