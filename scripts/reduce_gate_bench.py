#!/usr/bin/env python3
"""What fusing the gates into the reduce costs and saves: the gated reduce
kernel (native.gated_reduce) against the plain bf16 reduce at the same fan-in
and size (native.reduce_many) and against the unfused combine it replaces (K
torch scale passes into bf16 scratch, then the plain reduce over the scratch),
in one process and one window.

For each size (about 1 MiB .. 1 GiB, rounded down to whole rows), fan-in K (2,
4, 8 local sources) and row length H (2048, 7168 bf16): a sustained warm-up of
the three, then `--rounds` rounds in which they take turns, each between its
own pair of events; the medians.  The whole measurement is repeated
`--repeats` times: the spread of a ratio is the range of its per-repeat values.
Rates are payload GB/s: bytes of output per second.  From traffic alone the
fused kernel should run at the plain reduce's rate (16 B of gates per K x 2H
bytes read) and about (2K + 1) / (K + 1) x the unfused rate.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --reduce bf16
--reduce-gate H).

    python scripts/reduce_gate_bench.py [--json out.json] [--rounds 20] [--repeats 3]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import test_nccl_p2p_amd  # noqa: E402
from copy_checked_bench import alternate, warm  # noqa: E402

MIB = 1 << 20
SIZES = [1 * MIB, 32 * MIB, 256 * MIB, 1024 * MIB]
FAN_INS = (2, 4, 8)
ROW_ELEMS = (2048, 7168)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reduce_gate_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for size in SIZES:
        for h in ROW_ELEMS:
            rows = size // (2 * h)
            nbytes = rows * 2 * h
            dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))]
            scratch = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))]
            gates = torch.empty(16 * rows, dtype=torch.uint8, device="cuda")
            for k, s in enumerate(src):
                nat.fill_operand(s.data_ptr(), nbytes, 1000 + k, "bf16", st)
            nat.fill_gate(gates.data_ptr(), rows, 77, st)
            gate_cols = gates.view(torch.bfloat16).view(rows, 8)
            src_rows = [s.view(torch.bfloat16).view(rows, h) for s in src]
            scratch_rows = [s.view(torch.bfloat16).view(rows, h) for s in scratch]
            for K in FAN_INS:
                plain_ops = [(dst.data_ptr(), [s.data_ptr() for s in src[:K]], nbytes)]
                scaled_ops = [(dst.data_ptr(), [s.data_ptr() for s in scratch[:K]], nbytes)]
                srcs = [s.data_ptr() for s in src[:K]]

                def fused():
                    nat.gated_reduce(dst.data_ptr(), srcs, nbytes, gates.data_ptr(), h, st)

                def plain():
                    nat.reduce_many(plain_ops, "bf16", st, False)

                def unfused():
                    for k in range(K):
                        torch.mul(src_rows[k], gate_cols[:, k:k + 1], out=scratch_rows[k])
                    nat.reduce_many(scaled_ops, "bf16", st, False)

                reps = []
                for _ in range(args.repeats):
                    warm([fused, plain, unfused], args.warm_seconds)
                    ms = alternate([fused, plain, unfused], args.rounds)
                    reps.append([statistics.median(m) for m in ms])
                gbs = [[nbytes / (m * 1e-3) / 1e9 for m in rep] for rep in reps]
                rec = {
                    "bytes": nbytes, "rows": rows, "row_elems": h, "fan_in": K, "rounds": args.rounds, "repeats": args.repeats,
                    "memory": "one GPU: HBM, no xGMI",
                    "fused_ms": [r[0] for r in reps], "plain_ms": [r[1] for r in reps], "unfused_ms": [r[2] for r in reps],
                    "fused_gbs": [g[0] for g in gbs], "plain_gbs": [g[1] for g in gbs], "unfused_gbs": [g[2] for g in gbs],
                    "fused_over_plain": [g[0] / g[1] for g in gbs], "fused_over_unfused": [g[0] / g[2] for g in gbs],
                    "traffic_expectation_over_unfused": (2 * K + 1) / (K + 1),
                }
                records.append(rec)
                print("%9d B  H=%-5d K=%d  fused %6.0f GB/s  plain %6.0f  unfused %6.0f   fused/plain %.3f..%.3f   "
                      "fused/unfused %.2f..%.2f (traffic alone: %.2f)"
                      % (nbytes, h, K, statistics.median(rec["fused_gbs"]), statistics.median(rec["plain_gbs"]),
                         statistics.median(rec["unfused_gbs"]), min(rec["fused_over_plain"]), max(rec["fused_over_plain"]),
                         min(rec["fused_over_unfused"]), max(rec["fused_over_unfused"]), rec["traffic_expectation_over_unfused"]),
                      flush=True)
            del src, scratch, dst, gates, src_rows, scratch_rows, gate_cols
            torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
