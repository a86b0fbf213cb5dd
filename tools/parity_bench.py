"""Times hs.parity_encode of P+Q (k_parity_encode) over k HBM members
against hs.hbm_copy (k_copy_range) moving the same total number of
bytes, the yardstick: a copy of B bytes reads B and writes B, so it is
sized at (k + 2) / 2 members' worth. Both are reported as bytes read
plus bytes written per second. A timed window holds --reps calls back
to back (one 1 GiB-member encode takes about 2 ms), and the windows of
the two are timed alternately, after warm-up runs of both at the timed
sizes. Then times hs.parity_check of the same set at --check-granules
(bytes read per second: k + 2 members). Prints one JSON line.

    python tools/parity_bench.py [--k 6] [--gib 1] [--runs 9] [--reps 16]

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


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(samples, moved):
    med = statistics.median(samples)
    return {"median_ms": round(med * 1e3, 3),
            "min_ms": round(min(samples) * 1e3, 3),
            "max_ms": round(max(samples) * 1e3, 3),
            "moved_bytes": moved,
            "bytes_per_s": round(moved / med)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--k", type=int, default=6, help="data members")
    ap.add_argument("--gib", type=float, default=1.0, help="member size")
    ap.add_argument("--runs", type=int, default=9, help="timed runs of each")
    ap.add_argument("--reps", type=int, default=16,
                    help="calls per timed window")
    ap.add_argument("--check-granules", type=int, nargs="+",
                    default=[512, 4096])
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs must be at least 5")
    if not hs.gpu_available():
        sys.exit("parity_bench: no HIP device (no fallback)")

    block = 512
    length = int(args.gib * (1 << 30)) // 4096 * 4096
    blocks = length // block
    members = [hs.create_hbm_bdev(f"parbench-{i}", block, blocks,
                                  device=args.device)
               for i in range(args.k + 2)]
    # Non-trivial content: a random piece per member, doubled up by
    # device copies.
    for i, vol in enumerate(members[:args.k]):
        have = min(length, 8 << 20)
        vol.write(0, random.Random(i).randbytes(have))
        while have < length:
            step = min(have, length - have)
            hs.hbm_copy(vol, 0, vol, have, step)
            have += step
    data, p, q = members[:args.k], members[args.k], members[args.k + 1]
    moved = (args.k + 2) * length
    # The copy moves the same bytes: (k + 2) / 2 member-sized copies
    # between volumes the encode does not need meanwhile (P -> Q; both
    # are rewritten by the next encode).
    copy_bytes = moved // 2 // 16 * 16
    whole, rest = divmod(copy_bytes, length)

    def encode(reps=args.reps):
        for _ in range(reps):
            r = hs.parity_encode(data, p, q)
            assert r["on_gpu"] and r["length"] == length

    def copy():
        for _ in range(args.reps):
            for _ in range(whole):
                hs.hbm_copy(p, 0, q, 0, length)
            if rest:
                hs.hbm_copy(p, 0, q, 0, rest)

    for _ in range(2):
        encode()
        copy()
    enc_s, copy_s = [], []
    for _ in range(args.runs):  # alternate: both see the same neighbours
        enc_s.append(timed(encode))
        copy_s.append(timed(copy))
    encode(1)  # the last copy overwrote Q
    checks = {}
    for granule in args.check_granules:
        def scrub():
            for _ in range(args.reps):
                checks["last"] = hs.parity_check(data, p, q, granule=granule,
                                                 max_report=0)

        scrub()
        checks[str(granule)] = summary(
            [timed(scrub) for _ in range(args.runs)], args.reps * moved)
    check = checks.pop("last")
    e = summary(enc_s, args.reps * moved)
    c = summary(copy_s, args.reps * 2 * copy_bytes)
    print(json.dumps({
        "k": args.k, "member_bytes": length, "runs": args.runs,
        "reps_per_window": args.reps, "parity_check_pq": checks,
        "parity_encode_pq": e, "hbm_copy": c,
        "hbm_copy_calls_per_run": whole + (1 if rest else 0),
        "encode_over_copy_rate": round(e["bytes_per_s"] / c["bytes_per_s"], 3),
        "last_scrub_mismatched":
            [check["p"]["mismatched"], check["q"]["mismatched"]]}))


if __name__ == "__main__":
    main()
