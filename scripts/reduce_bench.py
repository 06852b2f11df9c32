#!/usr/bin/env python3
"""What the receive-and-reduce kernel moves: native.reduce_many against the
copy kernel and the verify kernel, in one process and one window.

For each shape (32 MiB x 32 ops, 1 GiB x 1), fan-in K (2 and 8 local
sources), access form (non-temporal, cross-GPU coherent on local memory) and
element type (u32, f32, bf16): a sustained warm-up of the three kernels, then
20 rounds in which the plain copy of the same output shape (native.copy_many),
the verify of as many bytes (native.verify_many_launch) and the reduce take
turns, each launch between its own pair of events; the medians.  Rates are
bytes read + written per second: (K + 1) x payload for the reduce, 2 x payload
for the copy, 1 x payload (loads only) for the verify.  The two ratios compare
the reduce's traffic rate with those two yardsticks of the same window.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --reduce).

    python scripts/reduce_bench.py [--json out.json] [--rounds 20]
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
SHAPES = [("32MiB x 32", 32 * MIB, 32), ("1GiB x 1", 1024 * MIB, 1)]
FAN_INS = (2, 8)
DTYPES = ("u32", "f32", "bf16")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("reduce_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for name, nbytes, nops in SHAPES:
        total = nbytes * nops
        dst = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        src = [[torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(nops)]
        # The verify kernel's yardstick reads a buffer of its own that holds the
        # stream it expects (its clean path).
        vsrc = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        for i, v in enumerate(vsrc):
            nat.fill(v.data_ptr(), nbytes, 500 + i, st)
        verify_jobs = [(v.data_ptr(), nbytes, 500 + i) for i, v in enumerate(vsrc)]
        for dtype in DTYPES:
            for i, row in enumerate(src):
                for k, s in enumerate(row):
                    nat.fill_operand(s.data_ptr(), nbytes, 1000 + 8 * i + k, dtype, st)
            copy_ops = [(d.data_ptr(), row[0].data_ptr(), nbytes) for d, row in zip(dst, src)]
            for K in FAN_INS:
                reduce_ops = [(d.data_ptr(), [s.data_ptr() for s in row[:K]], nbytes) for d, row in zip(dst, src)]
                for coherent in (False, True):
                    def copy():
                        nat.copy_many(copy_ops, st, coherent)

                    def load():
                        nat.verify_many_launch(verify_jobs, st)

                    def reduce():
                        nat.reduce_many(reduce_ops, dtype, st, coherent)

                    warm([copy, load, reduce], args.warm_seconds)
                    ms_copy, ms_load, ms_reduce = alternate([copy, load, reduce], args.rounds)
                    rec = {
                        "shape": name, "bytes": nbytes, "ops": nops, "dtype": dtype, "fan_in": K,
                        "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                        "copy_ms": ms_copy, "load_ms": ms_load, "reduce_ms": ms_reduce,
                        "copy_traffic_tbs": 2 * total / (statistics.median(ms_copy) * 1e-3) / 1e12,
                        "verify_load_tbs": total / (statistics.median(ms_load) * 1e-3) / 1e12,
                        "reduce_traffic_tbs": (K + 1) * total / (statistics.median(ms_reduce) * 1e-3) / 1e12,
                        "reduce_output_tbs": total / (statistics.median(ms_reduce) * 1e-3) / 1e12,
                    }
                    rec["reduce_over_copy"] = rec["reduce_traffic_tbs"] / rec["copy_traffic_tbs"]
                    rec["reduce_over_load"] = rec["reduce_traffic_tbs"] / rec["verify_load_tbs"]
                    records.append(rec)
                    print("%-11s %-4s K=%d %-8s reduce %.3f TB/s of traffic (copy %.3f, verify loads %.3f): "
                          "reduce/copy %.3f  reduce/load %.3f  (median of %d, reduce ms %.4f..%.4f)"
                          % (name, dtype, K, rec["form"], rec["reduce_traffic_tbs"], rec["copy_traffic_tbs"],
                             rec["verify_load_tbs"], rec["reduce_over_copy"], rec["reduce_over_load"], args.rounds,
                             min(ms_reduce), max(ms_reduce)), flush=True)
        del src, dst, vsrc
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
