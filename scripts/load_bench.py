#!/usr/bin/env python3
"""What a background load costs the self cell, and the cell the load.

For each GPU transport (ipc, rccl), each shape (32 MiB x 128, 1 GiB x 32) and
each load (mfma, hbm; one workgroup per CU unless --wgs says otherwise): one
untimed warm-up, then 5 runs of Session.run(..., load=KIND) in one process.  Every such run measures the cell quiet and then
once more beside the load (--load's two passes), so quiet and loaded alternate
in one window and each loaded rate is compared with the quiet rate taken just
before it.  Per run: the cell's loaded / quiet rate (agg_gbs over
quiet_agg_gbs) and the load's during / alone rate; reported are the medians
of the 5, with their min and max, and how many of the 5 windows the load's
train covered to the end.  An uncovered window ran partly on a quiet GPU: its
cell ratio is an upper bound, and --load cannot tell a cell that slowed down by
more than the train's 2x from one that waited behind the train.

Writes load_bench.json (every run) and load_bench.txt (the table) under --out.

    python scripts/load_bench.py [--out profiles/load] [--runs 5] [--wgs N]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import test_nccl_p2p_amd  # noqa: E402

MIB = 1 << 20
SHAPES = [("32MiB x 128", 32 * MIB, 128), ("1GiB x 32", 1024 * MIB, 32)]
TRANSPORTS = ["ipc", "rccl"]
KINDS = ["mfma", "hbm"]


def one(sess, nbytes, iters, spec):
    run = json.loads(sess.run(mode="self", bytes=nbytes, iters=iters, warmup=8, verify=True, load=spec))
    (ph,) = run["phases"]
    assert ph["mismatches"] == 0, "a loaded run did not verify"
    load = ph["load"]
    return {
        "quiet_gbs": load["quiet_agg_gbs"], "loaded_gbs": ph["agg_gbs"], "cell_ratio": ph["agg_gbs"] / load["quiet_agg_gbs"],
        "alone_rate": run["load"]["alone_rate"], "during_rate": load["during_rate"], "unit": run["load"]["unit"],
        "load_ratio": load["during_rate"] / run["load"]["alone_rate"], "launch_us": run["load"]["launch_us"],
        "wgs": run["load"]["wgs"], "window_launches": load["window_launches"], "window_s": load["window_s"],
        "covered": load["covered"],
    }


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "load"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--wgs", type=int, default=0, help="workgroups per launch of the load (0: one per CU)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("load_bench: needs a GPU (no ratio is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    os.makedirs(args.out, exist_ok=True)
    records, lines = [], []
    for transport in TRANSPORTS:
        sess = nat.Session(0, 1, device=0, transport=transport)
        for name, nbytes, iters in SHAPES:
            for kind in KINDS:
                spec = kind + (":%d" % args.wgs if args.wgs else "")
                one(sess, nbytes, iters, spec)  # warm-up: code objects, buffers, connections
                runs = [one(sess, nbytes, iters, spec) for _ in range(args.runs)]
                rec = {"transport": transport, "shape": name, "bytes": nbytes, "iters": iters, "load": kind,
                       "device": sess.device_desc, "runs": runs,
                       "cell_ratio": spread([r["cell_ratio"] for r in runs]),
                       "load_ratio": spread([r["load_ratio"] for r in runs]),
                       "quiet_gbs": spread([r["quiet_gbs"] for r in runs]),
                       "alone_rate": spread([r["alone_rate"] for r in runs]),
                       "launch_us": spread([r["launch_us"] for r in runs]),
                       "covered_runs": sum(1 for r in runs if r["covered"])}
                records.append(rec)
                line = ("%-5s %-12s %-4s cell loaded/quiet %.3f (%.3f..%.3f), quiet %.1f GB/s; load during/alone %.3f "
                        "(%.3f..%.3f), alone %.3f %s, %d workgroups, %.0f us launches; %d of %d windows covered"
                        % (transport, name, kind, rec["cell_ratio"]["median"], rec["cell_ratio"]["min"],
                           rec["cell_ratio"]["max"], rec["quiet_gbs"]["median"], rec["load_ratio"]["median"],
                           rec["load_ratio"]["min"], rec["load_ratio"]["max"], rec["alone_rate"]["median"],
                           runs[0]["unit"], runs[0]["wgs"], rec["launch_us"]["median"], rec["covered_runs"], len(runs)))
                lines.append(line)
                print(line, flush=True)
        del sess
    with open(os.path.join(args.out, "load_bench.json"), "w") as f:
        json.dump(records, f, indent=1)
    with open(os.path.join(args.out, "load_bench.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
