"""Times full exports and imports of an HBM volume with and without
`compress`, per content, alternating in one process.

    python tools/compress_bench.py [--gib 8] [--granule 4096] [--runs 3]
                                   [--dir /dev/shm] [--no-compress]

Contents (seeded):
  sparse   all zero beyond a 5 % random prefix
  text     words drawn from a 200-word list
  random   random bytes
Per content: one warm-up, then `runs` rounds of export, export with
compress, import and import of the compressed file, each timed around
the Python call (the file is on --dir, a tmpfs). Prints one JSON line
per content with medians, min-max, GB/s of volume bytes and the achieved
ratio. --no-compress runs the uncompressed half only, which is all a
build without the feature has. Needs a GPU: there is no fallback.

    python tools/compress_bench.py --dictionary [--changed 0.01] ...

measures an incremental instead: a base volume (text or random; sparse
is skipped), a live volume that differs from it in `--changed` of the
granules by a 64-byte in-place edit, and per round an export against the
base as a version-1, a version-2 (compress) and a version-4 (compress,
dictionary) file, each imported onto a third volume that was put back to
the base state first (untimed). One JSON line per content with the
times, the file sizes and the stored ratios of the changed granules.

    python tools/compress_bench.py --cts ...

adds a third export and import per round to the full-volume run: compress
with a key and cts (a version-5 file, keys "export_cts", "import_cts"),
alternating with the other two, so the cost of encrypting the pieces
reads off one line."""
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
KEY = bytes(range(1, 65))  # for --cts


def content_chunks(kind, length, rng):
    """The volume's bytes in pieces of STEP."""
    words = [bytes(rng.choice(list(b"etaoinshrdlu"), size=rng.integers(2, 10))
                   .astype(np.uint8)) for _ in range(200)]
    for off in range(0, length, STEP):
        n = min(STEP, length - off)
        if kind == "random" or (kind == "sparse" and off < length // 20):
            yield rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        elif kind == "sparse":
            yield bytes(n)
        else:  # 1 MiB of text, repeated with a fresh piece per chunk
            piece = b" ".join(words[i] for i in rng.integers(0, 200, 1 << 18))
            yield (piece[:1 << 20] * (n // (1 << 20) + 1))[:n]


def summary(samples, nbytes):
    med = statistics.median(samples)
    return {"median_s": round(med, 4), "min_s": round(min(samples), 4),
            "max_s": round(max(samples), 4),
            "gb_per_s": round(nbytes / med / 1e9, 3)}


def incremental(args, length, live, back):
    """The --dictionary half: see the module docstring."""
    block = 512
    base = hs.create_hbm_bdev("lzbench-base", block, length // block,
                              device=args.device)
    path = os.path.join(args.dir, f"lzbench-{os.getpid()}.delta")
    undo = path + ".undo"
    n = length // args.granule
    modes = {"v1": {}, "v2": {"compress": True},
             "v4": {"compress": True, "dictionary": True}}
    for kind in args.contents:
        if kind == "sparse":
            continue
        rng = np.random.default_rng(20264)
        off = 0
        for chunk in content_chunks(kind, length, rng):
            for bdev in (base, live, back):
                bdev.write(off, chunk)
            off += len(chunk)
        changed = rng.choice(n, size=max(1, int(n * args.changed)),
                             replace=False)
        for g in changed:  # 64 bytes in place; 512-byte blocks
            at = int(g) * args.granule + args.granule // 2
            sector = bytearray(live.read(at, block))
            sector[:64] = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
            live.write(at, bytes(sector))
        hs.bdev_export_delta(base, undo, base=live, granule=args.granule,
                             overwrite=True)
        out = {"content": kind, "volume_bytes": length, "granule": args.granule,
               "changed_granules": len(changed)}
        samples = {(what, m): [] for what in ("export", "import")
                   for m in modes}
        for run in range(args.runs + 1):  # run 0 warms up
            for m, kwargs in modes.items():
                hs.bdev_import_delta(back, undo)  # back to the base state
                t0 = time.perf_counter()
                info = hs.bdev_export_delta(live, path, base=base,
                                            granule=args.granule,
                                            overwrite=True, **kwargs)
                t1 = time.perf_counter()
                hs.bdev_import_delta(back, path)
                t2 = time.perf_counter()
                if run > 0:
                    samples[("export", m)].append(t1 - t0)
                    samples[("import", m)].append(t2 - t1)
                out["file_bytes_" + m] = info["file_bytes"]
                if "stored_bytes" in info:
                    out["ratio_" + m] = round(
                        len(changed) * args.granule / info["stored_bytes"], 2)
                if hs.bdev_diff(live, back,
                                granule=args.granule)["mismatched"] != 0:
                    sys.exit(f"compress_bench: {kind} {m}: restore differs")
        for (what, m), values in samples.items():
            out[f"{what}_{m}"] = summary(values, length)
        os.unlink(path)
        os.unlink(undo)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--gib", type=float, default=8.0, help="volume size")
    ap.add_argument("--granule", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--contents", nargs="+",
                    default=["sparse", "text", "random"])
    ap.add_argument("--dir", default="/dev/shm", help="where exports go")
    ap.add_argument("--no-compress", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dictionary", action="store_true",
                    help="measure an incremental as version 1, 2 and 4")
    ap.add_argument("--cts", action="store_true",
                    help="also measure compress with a key and cts")
    ap.add_argument("--changed", type=float, default=0.01,
                    help="with --dictionary: share of granules edited")
    args = ap.parse_args()
    if not hs.gpu_available():
        sys.exit("compress_bench: no HIP device (no fallback)")

    block = 512
    length = int(args.gib * (1 << 30)) // args.granule * args.granule
    live = hs.create_hbm_bdev("lzbench-live", block, length // block,
                              device=args.device)
    back = hs.create_hbm_bdev("lzbench-back", block, length // block,
                              device=args.device)
    if args.dictionary:
        return incremental(args, length, live, back)
    path = os.path.join(args.dir, f"lzbench-{os.getpid()}.delta")
    modes = [False] if args.no_compress else [False, True]
    if args.cts:
        modes.append("cts")

    for kind in args.contents:
        rng = np.random.default_rng(20264)
        off = 0
        for chunk in content_chunks(kind, length, rng):
            live.write(off, chunk)
            off += len(chunk)
        out = {"content": kind, "volume_bytes": length,
               "granule": args.granule}
        samples = {(what, lz): [] for what in ("export", "import")
                   for lz in modes}
        for run in range(args.runs + 1):  # run 0 warms up
            for lz in modes:
                if os.path.exists(path):
                    os.unlink(path)  # never two copies in the tmpfs
                kwargs = {"compress": True} if lz else {}
                if lz == "cts":
                    kwargs.update(key=KEY, cts=True)
                t0 = time.perf_counter()
                info = hs.bdev_export_delta(live, path, granule=args.granule,
                                            **kwargs)
                t1 = time.perf_counter()
                hs.bdev_import_delta(back, path, key=kwargs.get("key"))
                t2 = time.perf_counter()
                if run > 0:
                    samples[("export", lz)].append(t1 - t0)
                    samples[("import", lz)].append(t2 - t1)
                if lz == "cts":
                    out["file_bytes_cts"] = info["file_bytes"]
                elif lz:
                    out["file_bytes_lz"] = info["file_bytes"]
                    out["ratio"] = round(length / info["stored_bytes"], 3)
                else:
                    out["file_bytes"] = info["file_bytes"]
        if hs.bdev_diff(live, back, granule=args.granule)["mismatched"] != 0:
            sys.exit(f"compress_bench: {kind}: restored volume differs")
        os.unlink(path)
        for (what, lz), values in samples.items():
            out[what + ("_cts" if lz == "cts" else "_lz" if lz else "")] = \
                summary(values, length)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
