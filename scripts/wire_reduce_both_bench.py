#!/usr/bin/env python3
"""What storing both outputs from one launch buys at the turn-around hop of a
two-shot quantised all-reduce: native.wire_reduce_packed with `both` (both lane
mappings) against the launches it replaces, in one process and one window.

Two shapes, 32 MiB x 32 ops and 1 GiB x 1 op of payload; for each format
(mxfp8, mxfp6, mxfp4), fan-in (2, 4, 8) and access form (non-temporal, cross-GPU
coherent on local memory): a sustained warm-up, then 20 rounds in which the
candidates take turns, each between its own pair of events; the medians and the
quartiles.  Candidates:
  split, contiguous  native.wire_reduce_packed(both=...), one launch per op, in that lane mapping;
  baseline           what the same hop took before, on the same buffers:
                     mxfp8 / mxfp4: native.wire_reduce_packed (Auto) into the image, then
                       native.wire_unpack (Auto) of that image into the bf16 output;
                     mxfp6: native.wire_reduce (Auto) into bf16 scratch, native.wire_pack of
                       the scratch, native.wire_unpack of the image.
The three candidates' images and bf16 outputs are compared once per cell before
timing.  Reported per candidate: payload GB/s (bf16 bytes of sum represented per
second) and the median's quartiles.

On one GPU every source is local HBM: no xGMI link is involved, and a link
number needs a run over a node (p2p_matrix --transport ipc --reduce bf16
--reduce-wire FORMAT --reduce-out both).

    python scripts/wire_reduce_both_bench.py [--json out.json] [--rounds 20]
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
SHAPES = ((32 * MIB, 32), (1024 * MIB, 1))
FORMATS = ("mxfp8", "mxfp6", "mxfp4")
FAN_INS = (2, 4, 8)
NAMES = ("split", "contiguous", "baseline")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wire_reduce_both_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for nbytes, nops in SHAPES:
        total = nbytes * nops
        scratch = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        bf16 = {name: [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)] for name in NAMES}
        for fmt in FORMATS:
            wb = nat.wire_bytes(nbytes, fmt)
            images = [[torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(nops)]
            out = {name: [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(nops)] for name in NAMES}
            for i, ims in enumerate(images):
                for k, im in enumerate(ims):
                    nat.fill_packed(im.data_ptr(), nbytes, 1000 + 8 * i + k, fmt, st)
            for fan_in in FAN_INS:
                srcs = [[im.data_ptr() for im in ims[:fan_in]] for ims in images]
                for coherent in (False, True):
                    def fused(lanes):
                        for d, b, s in zip(out[lanes], bf16[lanes], srcs):
                            nat.wire_reduce_packed(d.data_ptr(), s, nbytes, fmt, st, coherent, 0, lanes, False, b.data_ptr())

                    def baseline():
                        for d, b, w, s in zip(out["baseline"], bf16["baseline"], scratch, srcs):
                            if fmt == "mxfp6":
                                nat.wire_reduce(w.data_ptr(), s, nbytes, fmt, st, coherent, 0, "auto")
                                nat.wire_pack(d.data_ptr(), w.data_ptr(), nbytes, fmt, st)
                            else:
                                nat.wire_reduce_packed(d.data_ptr(), s, nbytes, fmt, st, coherent, 0, "auto")
                            nat.wire_unpack(b.data_ptr(), d.data_ptr(), nbytes, fmt, st, False, 0, "auto")

                    fns = [lambda: fused("split"), lambda: fused("contiguous"), baseline]
                    for fn in fns:
                        fn()
                    torch.cuda.synchronize()
                    same = all(torch.equal(a, c) and torch.equal(b, c)
                               for o in (out, bf16) for a, b, c in zip(o["split"], o["contiguous"], o["baseline"]))
                    warm(fns, args.warm_seconds)
                    ms = dict(zip(NAMES, alternate(fns, args.rounds)))
                    rec = {"bytes": nbytes, "ops": nops, "format": fmt, "wire_bytes": wb, "fan_in": fan_in,
                           "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                           "outputs_equal": same, "ms": ms}
                    line = "%4dMiBx%-2d %-5s K=%d %-8s equal=%s" % (nbytes // MIB, nops, fmt, fan_in, rec["form"], same)
                    for k, v in ms.items():
                        q = statistics.quantiles(v, n=4)
                        rec[k + "_ms_quartiles"] = q
                        rec[k + "_payload_gbs"] = total / (q[1] * 1e-3) / 1e9
                        line += " | %s %.3f ms (%.3f-%.3f) %5.0f GB/s" % (k, q[1], q[0], q[2], rec[k + "_payload_gbs"])
                    records.append(rec)
                    print(line, flush=True)
            del images, out
            torch.cuda.empty_cache()
        del scratch, bf16
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
