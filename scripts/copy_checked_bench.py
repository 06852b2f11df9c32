#!/usr/bin/env python3
"""What checking costs: the checked copy kernel against the plain one, in
one process and one window.

For each shape (32 MiB x 32 ops, 256 MiB, 1 GiB) and each access form (plain
non-temporal, cross-GPU coherent on local memory): a sustained warm-up of
both kernels, then 20 rounds in which the plain copy (native.copy_many) and
the checked copy (native.copy_checked_launch) alternate, each launch between
its own pair of events; the medians and their ratio.  The yardstick is the
plain copy of the same window, nothing else.  Rates are payload bytes per
second (each byte is read once and written once).

The sources hold the stream the checked kernel expects, so this is its clean
path (one wave vote, no atomics); --corrupt flips one byte per 4 KiB chunk
to time the path on which every wave commits.

    python scripts/copy_checked_bench.py [--json out.json] [--rounds 20] [--corrupt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import test_nccl_p2p_amd  # noqa: E402
from test_nccl_p2p_amd.ops import fill_  # noqa: E402

MIB = 1 << 20
SHAPES = [("32MiB x 32", 32 * MIB, 32), ("256MiB x 1", 256 * MIB, 1), ("1GiB x 1", 1024 * MIB, 1)]


def warm(fns, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            for fn in fns:
                fn()
        torch.cuda.synchronize()


def alternate(fns, rounds):
    """rounds x len(fns) launches, fns taking turns, an event pair around
    each; per fn the list of its launch times in ms."""
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns]
          for _ in range(rounds)]
    for row in ev:
        for fn, (s, e) in zip(fns, row):
            s.record()
            fn()
            e.record()
    torch.cuda.synchronize()
    return [[row[k][0].elapsed_time(row[k][1]) for row in ev] for k in range(len(fns))]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--corrupt", action="store_true", help="one wrong byte per 4 KiB chunk: every wave commits")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("copy_checked_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for name, nbytes, nops in SHAPES:
        src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        dst = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        for i, s in enumerate(src):
            fill_(s, 1000 + i)
            if args.corrupt:
                s[1::4096] ^= 1
        plain_ops = [(d.data_ptr(), s.data_ptr(), nbytes) for d, s in zip(dst, src)]
        checked_ops = [(d.data_ptr(), s.data_ptr(), nbytes, 1000 + i, 0, i) for i, (d, s) in enumerate(zip(dst, src))]
        for coherent in (False, True):
            def plain():
                nat.copy_many(plain_ops, st, coherent)

            def checked():
                nat.copy_checked_launch(checked_ops, st, coherent)

            found = nat.copy_checked(checked_ops, st, coherent)  # also allocates the records
            wrong = sum(m for m, _ in found)
            assert (wrong > 0) == args.corrupt, found[:4]
            warm([plain, checked], args.warm_seconds)
            ms_plain, ms_checked = alternate([plain, checked], args.rounds)
            total = nbytes * nops
            rec = {
                "shape": name, "bytes": nbytes, "ops": nops, "form": "coherent" if coherent else "plain",
                "corrupt": args.corrupt, "rounds": args.rounds,
                "plain_ms": ms_plain, "checked_ms": ms_checked,
                "plain_tbs": total / (statistics.median(ms_plain) * 1e-3) / 1e12,
                "checked_tbs": total / (statistics.median(ms_checked) * 1e-3) / 1e12,
            }
            rec["checked_over_plain"] = rec["checked_tbs"] / rec["plain_tbs"]
            records.append(rec)
            print("%-11s %-8s plain %.3f TB/s  checked %.3f TB/s  checked/plain %.3f  (median of %d, ms plain %.4f..%.4f, "
                  "checked %.4f..%.4f)" % (name, rec["form"], rec["plain_tbs"], rec["checked_tbs"], rec["checked_over_plain"],
                                           args.rounds, min(ms_plain), max(ms_plain), min(ms_checked), max(ms_checked)),
                  flush=True)
        del src, dst
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
