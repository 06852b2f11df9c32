#!/usr/bin/env python3
"""What the wire formats cost the receiver and the sender: native.wire_unpack_many
and native.wire_pack against the plain copy kernel, in one process and one window.

For each shape (32 MiB x 32 ops, 1 GiB x 1; payload bytes), format (mxfp8,
mxfp6, mxfp4; --formats picks) and access form (non-temporal, cross-GPU coherent on local memory): a
sustained warm-up, then 20 rounds in which the plain copy of the payload
(native.copy_many), the unpack in both lane mappings (split, contiguous) and
the pack take turns, each launch (the pack: one launch per op) between its
own pair of events; the medians.  Reported per kernel: payload GB/s (bf16
bytes delivered or consumed per second) and traffic, bytes read + written per
second: payload + wire image for unpack and pack, 2 x payload for the copy.
The pack has no cross-GPU form and is timed in the local one only.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --wire).

    python scripts/wire_bench.py [--json out.json] [--rounds 20]
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
FORMATS = ("mxfp8", "mxfp6", "mxfp4")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--formats", default=",".join(FORMATS), help="comma-separated subset of " + ", ".join(FORMATS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wire_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for name, nbytes, nops in SHAPES:
        total = nbytes * nops
        dst = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        src = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]  # the copy's source, the pack's payload
        copy_ops = [(d.data_ptr(), s.data_ptr(), nbytes) for d, s in zip(dst, src)]
        for fmt in args.formats.split(","):
            wb = nat.wire_bytes(nbytes, fmt)
            wire = [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(nops)]
            packed = [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(nops)]
            for i, (w, s) in enumerate(zip(wire, src)):
                nat.fill_packed(w.data_ptr(), nbytes, 1000 + i, fmt, st)
                nat.wire_unpack(s.data_ptr(), w.data_ptr(), nbytes, fmt, st)  # the pack's input: bf16 inside the contract
            unpack_ops = [(d.data_ptr(), w.data_ptr(), nbytes) for d, w in zip(dst, wire)]
            for coherent in (False, True):
                def copy():
                    nat.copy_many(copy_ops, st, coherent)

                def split():
                    nat.wire_unpack_many(unpack_ops, fmt, st, coherent, 0, "split")

                def contiguous():
                    nat.wire_unpack_many(unpack_ops, fmt, st, coherent, 0, "contiguous")

                def pack():
                    for p, s in zip(packed, src):
                        nat.wire_pack(p.data_ptr(), s.data_ptr(), nbytes, fmt, st)

                fns = [copy, split, contiguous] + ([] if coherent else [pack])
                warm(fns, args.warm_seconds)
                ms = dict(zip(("copy", "split", "contiguous", "pack"), alternate(fns, args.rounds)))
                rec = {"shape": name, "bytes": nbytes, "ops": nops, "format": fmt, "wire_bytes": wb,
                       "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                       "ms": ms}
                for k, v in ms.items():
                    s = statistics.median(v) * 1e-3
                    rec[k + "_payload_gbs"] = total / s / 1e9
                    rec[k + "_traffic_tbs"] = (2 * total if k == "copy" else total + wb * nops) / s / 1e12
                records.append(rec)
                line = "%-11s %-5s %-8s copy %6.0f GB/s (%.3f TB/s traffic)" % (name, fmt, rec["form"], rec["copy_payload_gbs"],
                                                                                 rec["copy_traffic_tbs"])
                for k in list(ms)[1:]:
                    line += " | %s %6.0f GB/s payload, %.3f TB/s traffic (%.3fx copy's)" % (
                        k, rec[k + "_payload_gbs"], rec[k + "_traffic_tbs"], rec[k + "_traffic_tbs"] / rec["copy_traffic_tbs"])
                print(line, flush=True)
            del wire, packed
            torch.cuda.empty_cache()
        del src, dst
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
