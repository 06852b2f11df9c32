#!/usr/bin/env python3
"""What the fused sum of wire images buys: native.wire_reduce (both lane
mappings) against the two-launch path, the bf16 reduce and the plain copy, in
one process and one window.

For each shape (32 MiB x 32 ops, 1 GiB x 1; payload bytes), format (mxfp8,
mxfp6, mxfp4; --formats picks), fan-in (2, 4, 8) and access form (non-temporal, cross-GPU coherent on
local memory): a sustained warm-up, then 20 rounds in which the candidates take
turns, each between its own pair of events; the medians.  Candidates:
  split, contiguous  native.wire_reduce, one launch per op, in that lane mapping;
  two_pass           (a) native.wire_unpack_many of the K images of every op into
                     bf16 scratch, then native.reduce_many over the scratch;
  reduce_bf16        (b) native.reduce_many over K bf16 operands at the same fan-in;
  copy               (c) native.copy_many of the payload.
Reported per candidate: payload GB/s (bf16 bytes of sum delivered per second)
and traffic, bytes read + written per second: K images + payload for the fused
kernel, K images + 2 K payloads + payload for the two passes, (K + 1) payloads
for the bf16 reduce, 2 payloads for the copy.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --reduce bf16
--reduce-wire FORMAT).

    python scripts/wire_reduce_bench.py [--json out.json] [--rounds 20]
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
FAN_INS = (2, 4, 8)
NAMES = ("split", "contiguous", "two_pass", "reduce_bf16", "copy")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--formats", default=",".join(FORMATS), help="comma-separated subset of " + ", ".join(FORMATS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wire_reduce_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for name, nbytes, nops in SHAPES:
        total = nbytes * nops
        dst = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        # bf16 scratch of the two-pass path, also the operands of the bf16 reduce and the copy's source.
        wide = [[torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(nops)]
        copy_ops = [(d.data_ptr(), w[0].data_ptr(), nbytes) for d, w in zip(dst, wide)]
        for fmt in args.formats.split(","):
            wb = nat.wire_bytes(nbytes, fmt)
            images = [[torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(nops)]
            for i, (ims, ws) in enumerate(zip(images, wide)):
                for k, (im, w) in enumerate(zip(ims, ws)):
                    nat.fill_packed(im.data_ptr(), nbytes, 1000 + 8 * i + k, fmt, st)
                    nat.wire_unpack(w.data_ptr(), im.data_ptr(), nbytes, fmt, st)  # finite bf16 for the reduce
            for fan_in in FAN_INS:
                unpack_ops = [(w.data_ptr(), im.data_ptr(), nbytes) for ims, ws in zip(images, wide)
                              for im, w in zip(ims[:fan_in], ws[:fan_in])]
                reduce_ops = [(d.data_ptr(), [w.data_ptr() for w in ws[:fan_in]], nbytes) for d, ws in zip(dst, wide)]
                fused_ops = [(d.data_ptr(), [im.data_ptr() for im in ims[:fan_in]]) for d, ims in zip(dst, images)]
                for coherent in (False, True):
                    def fused(lanes):
                        for d, srcs in fused_ops:
                            nat.wire_reduce(d, srcs, nbytes, fmt, st, coherent, 0, lanes)

                    def two_pass():
                        nat.wire_unpack_many(unpack_ops, fmt, st, coherent)
                        nat.reduce_many(reduce_ops, "bf16", st, coherent)

                    fns = [lambda: fused("split"), lambda: fused("contiguous"), two_pass,
                           lambda: nat.reduce_many(reduce_ops, "bf16", st, coherent), lambda: nat.copy_many(copy_ops, st, coherent)]
                    warm(fns, args.warm_seconds)
                    ms = dict(zip(NAMES, alternate(fns, args.rounds)))
                    read = wb * nops * fan_in
                    traffic = {"split": read + total, "contiguous": read + total, "two_pass": read + (2 * fan_in + 1) * total,
                               "reduce_bf16": (fan_in + 1) * total, "copy": 2 * total}
                    rec = {"shape": name, "bytes": nbytes, "ops": nops, "format": fmt, "wire_bytes": wb, "fan_in": fan_in,
                           "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                           "ms": ms}
                    line = "%-11s %-5s K=%d %-8s" % (name, fmt, fan_in, rec["form"])
                    for k, v in ms.items():
                        s = statistics.median(v) * 1e-3
                        rec[k + "_payload_gbs"] = total / s / 1e9
                        rec[k + "_traffic_tbs"] = traffic[k] / s / 1e12
                        line += " | %s %5.0f GB/s %.2f TB/s" % (k, rec[k + "_payload_gbs"], rec[k + "_traffic_tbs"])
                    records.append(rec)
                    print(line, flush=True)
            del images
            torch.cuda.empty_cache()
        del dst, wide
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
