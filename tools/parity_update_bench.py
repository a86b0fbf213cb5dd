"""Times hs.parity_update of P+Q (k_parity_update) with one tracked member
out of k against hs.parity_encode (k_parity_encode) of the same set, the
only way to bring parity up to date without it. Two cases: --percent of
the granules of the tracked member differ from its base (one 512-byte
block each, so one 1 KiB slab per changed granule is dirty), and all of
them differ (every slab dirty). A timed window holds --reps calls back to
back and the windows of the two calls alternate, after warm-up windows of
both. The update runs without refresh, so every call meets the same
differences and does the same work; an even number of calls leaves the
parity as the encode wrote it, which a scrub at the end confirms. Bytes
moved by an update: the member and its base once, plus stored P and Q
read and written in the dirty slabs. Prints one JSON line.

    python tools/parity_update_bench.py [--k 6] [--gib 1] [--member 5]

Host clock around calls that end in a stream synchronise (every call
also creates and destroys a stream, which is part of either figure).
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import oim_amd._hipstore as hs  # noqa: E402

BLOCK = 512
SLAB = 1024


def window_ms(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e3


def summary(samples, moved, reps):
    med = statistics.median(samples)
    return {"median_ms_per_call": round(med / reps, 4),
            "min_ms_per_call": round(min(samples) / reps, 4),
            "max_ms_per_call": round(max(samples) / reps, 4),
            "moved_bytes_per_call": moved,
            "bytes_per_s": round(moved * reps / (med / 1e3))}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--k", type=int, default=6, help="data members")
    ap.add_argument("--gib", type=float, default=1.0, help="member size")
    ap.add_argument("--member", type=int, default=None,
                    help="tracked member (default k - 1: the longest chain)")
    ap.add_argument("--granule", type=int, default=4096)
    ap.add_argument("--percent", type=float, default=1.0)
    ap.add_argument("--runs", type=int, default=9, help="timed windows of each")
    ap.add_argument("--reps", type=int, default=16, help="calls per window")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    member = args.k - 1 if args.member is None else args.member
    if args.runs < 5 or args.reps % 2 or not 0 <= member < args.k:
        ap.error("--runs >= 5, an even --reps and 0 <= --member < k are needed")
    if not hs.gpu_available():
        sys.exit("parity_update_bench: no HIP device (no fallback)")

    length = int(args.gib * (1 << 30)) // args.granule * args.granule
    vols = [hs.create_hbm_bdev(f"parupd-{i}", BLOCK, length // BLOCK,
                               device=args.device) for i in range(args.k + 3)]
    data, (p, q, base) = vols[:args.k], vols[args.k:]
    for i, vol in enumerate(data):  # a random piece, doubled up on the device
        have = min(length, 8 << 20)
        vol.write(0, random.Random(i).randbytes(have))
        while have < length:
            step = min(have, length - have)
            hs.hbm_copy(vol, 0, vol, have, step)
            have += step
    bases = [base if i == member else None for i in range(args.k)]
    n = length // args.granule

    def encode():
        assert hs.parity_encode(data, p, q)["on_gpu"]

    last = {}

    def update():
        last["r"] = hs.parity_update(data, p, q, bases, granule=args.granule,
                                     max_report=0)

    out = {"k": args.k, "member_bytes": length, "tracked": member,
           "granule": args.granule, "runs": args.runs,
           "reps_per_window": args.reps}
    rng = random.Random(1)
    sparse = rng.sample(range(n), max(1, round(n * args.percent / 100)))
    for case in ("sparse", "all"):
        if case == "sparse":  # a clone, then one other block per chosen granule
            hs.hbm_copy(data[member], 0, base, 0, length)
            for g in sparse:
                base.write(g * args.granule, rng.randbytes(BLOCK))
            dirty_slabs = len(sparse)
        else:  # another member's bytes: differs in every slab
            hs.hbm_copy(data[(member + 1) % args.k], 0, base, 0, length)
            dirty_slabs = length // SLAB
        for _ in range(2):
            window_ms(encode, args.reps)
            window_ms(update, args.reps)
        enc, upd = [], []
        for _ in range(args.runs):  # alternate: both see the same neighbours
            enc.append(window_ms(encode, args.reps))
            upd.append(window_ms(update, args.reps))
        check = hs.parity_check(data, p, q, granule=args.granule, max_report=0)
        e = summary(enc, (args.k + 2) * length, args.reps)
        u = summary(upd, 2 * length + 4 * SLAB * dirty_slabs, args.reps)
        out[case] = {
            "changed_granules": last["r"]["changed"]["mismatched"],
            "on_gpu": last["r"]["on_gpu"], "parity_encode_pq": e,
            "parity_update_pq": u,
            "encode_over_update_time": round(
                e["median_ms_per_call"] / u["median_ms_per_call"], 3),
            "scrub_mismatched_after": [check["p"]["mismatched"],
                                       check["q"]["mismatched"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
