#!/usr/bin/env python3
"""What fusing the requantisation into the sum of wire images buys:
native.wire_reduce_packed (both lane mappings) against the two launches it
replaces, in one process and one window.

One shape, 32 MiB x 32 ops of payload; for each format (mxfp8, mxfp4), fan-in
(2, 4, 8) and access form (non-temporal, cross-GPU coherent on local memory): a
sustained warm-up, then 20 rounds in which the candidates take turns, each
between its own pair of events; the medians and the quartiles.  Candidates:
  split, contiguous  native.wire_reduce_packed, one launch per op, in that lane mapping;
  two_launch         native.wire_reduce (Auto lanes) of every op into bf16 scratch,
                     then native.wire_pack of the scratch: the same buffers, the
                     same image bit for bit (compared once per cell before timing).
Reported per candidate: payload GB/s (bf16 bytes of sum represented per second)
and traffic, bytes read + written per second: K images + 1 image for the fused
kernel, K images + 2 payloads + 1 image for the two launches.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --reduce bf16
--reduce-wire FORMAT --reduce-out wire).

    python scripts/wire_reduce_pack_bench.py [--json out.json] [--rounds 20]
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
NBYTES, NOPS = 32 * MIB, 32
FORMATS = ("mxfp8", "mxfp4")
FAN_INS = (2, 4, 8)
NAMES = ("split", "contiguous", "two_launch")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wire_reduce_pack_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    total = NBYTES * NOPS
    scratch = [torch.empty(NBYTES, dtype=torch.uint8, device="cuda") for _ in range(NOPS)]
    records = []
    for fmt in FORMATS:
        wb = nat.wire_bytes(NBYTES, fmt)
        images = [[torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(NOPS)]
        out = {name: [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(NOPS)] for name in NAMES}
        for i, ims in enumerate(images):
            for k, im in enumerate(ims):
                nat.fill_packed(im.data_ptr(), NBYTES, 1000 + 8 * i + k, fmt, st)
        for fan_in in FAN_INS:
            srcs = [[im.data_ptr() for im in ims[:fan_in]] for ims in images]
            for coherent in (False, True):
                def fused(lanes):
                    for d, s in zip(out[lanes], srcs):
                        nat.wire_reduce_packed(d.data_ptr(), s, NBYTES, fmt, st, coherent, 0, lanes)

                def two_launch():
                    for d, w, s in zip(out["two_launch"], scratch, srcs):
                        nat.wire_reduce(w.data_ptr(), s, NBYTES, fmt, st, coherent, 0, "auto")
                        nat.wire_pack(d.data_ptr(), w.data_ptr(), NBYTES, fmt, st)

                fns = [lambda: fused("split"), lambda: fused("contiguous"), two_launch]
                for fn in fns:
                    fn()
                torch.cuda.synchronize()
                same = all(torch.equal(a, c) and torch.equal(b, c) for a, b, c in zip(out["split"], out["contiguous"], out["two_launch"]))
                warm(fns, args.warm_seconds)
                ms = dict(zip(NAMES, alternate(fns, args.rounds)))
                read = wb * NOPS * fan_in
                traffic = {"split": read + wb * NOPS, "contiguous": read + wb * NOPS, "two_launch": read + 2 * total + wb * NOPS}
                rec = {"bytes": NBYTES, "ops": NOPS, "format": fmt, "wire_bytes": wb, "fan_in": fan_in,
                       "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                       "images_equal": same, "ms": ms}
                line = "%-5s K=%d %-8s equal=%s" % (fmt, fan_in, rec["form"], same)
                for k, v in ms.items():
                    q = statistics.quantiles(v, n=4)
                    s = q[1] * 1e-3
                    rec[k + "_ms_quartiles"] = q
                    rec[k + "_payload_gbs"] = total / s / 1e9
                    rec[k + "_traffic_tbs"] = traffic[k] / s / 1e12
                    line += " | %s %.3f ms (%.3f-%.3f) %5.0f GB/s %.2f TB/s" % (k, q[1], q[0], q[2], rec[k + "_payload_gbs"],
                                                                               rec[k + "_traffic_tbs"])
                records.append(rec)
                print(line, flush=True)
        del images, out
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
