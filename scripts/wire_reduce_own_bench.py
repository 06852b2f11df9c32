#!/usr/bin/env python3
"""What the fused sum onto a bf16 own shard buys (--reduce-own bf16):
native.wire_reduce(..., own_bf16=True) in both lane mappings against the two
launches it replaces, in one process and one window, with the all-image kernel
at the same fan-in for context.  scripts/wire_reduce_bench.py's method.

For each shape (32 MiB x 32 ops, 1 GiB x 1; payload bytes), format (mxfp8,
mxfp6, mxfp4; --formats picks), fan-in (2, 4, 8) and access form (local: every
source non-temporal; cross-GPU: the K - 1 incoming images read coherently from
local memory, the own shard local as always): a sustained warm-up, then 20
rounds in which the candidates take turns, each between its own pair of events;
the medians.  Candidates:
  own_split, own_contiguous    native.wire_reduce with own_bf16, one launch per op, in that lane mapping
                               (mxfp6: load_block and store_block through LDS / straight from the lane);
  two_launch                   native.wire_unpack_many of the K - 1 incoming images of every op into bf16
                               scratch, then native.reduce_many over the own shard and the scratch;
  all_image                    native.wire_reduce over K images (Auto lanes): the hop --reduce-own wire times;
  pack_split, pack_contiguous  native.wire_reduce_packed with own_bf16 (mxfp8, mxfp4): the requantised output.
Reported per candidate: payload GB/s (bf16 bytes of sum per second).

On one GPU every source is local HBM: no xGMI link is involved.

    python scripts/wire_reduce_own_bench.py [--json out.json] [--rounds 20]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", help="write the records here")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=0.3)
    ap.add_argument("--formats", default=",".join(FORMATS), help="comma-separated subset of " + ", ".join(FORMATS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("wire_reduce_own_bench: needs a GPU (no rate is reported without one)")
    nat = test_nccl_p2p_amd.require_native()
    torch.cuda.set_device(0)
    st = torch.cuda.current_stream().cuda_stream
    records = []
    for name, nbytes, nops in SHAPES:
        total = nbytes * nops
        dst = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        own = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(nops)]
        for i, o in enumerate(own):
            nat.fill_wire_operand(o.data_ptr(), nbytes, 2000 + 8 * i, st)
        # bf16 scratch of the two-launch path: one per incoming image.
        wide = [[torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS) - 1)] for _ in range(nops)]
        for fmt in args.formats.split(","):
            wb = nat.wire_bytes(nbytes, fmt)
            images = [[torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(max(FAN_INS))] for _ in range(nops)]
            for i, ims in enumerate(images):
                for k, im in enumerate(ims):
                    nat.fill_packed(im.data_ptr(), nbytes, 2000 + 8 * i + k, fmt, st)
            pdst = [torch.empty(wb, dtype=torch.uint8, device="cuda") for _ in range(nops)]
            packs = fmt != "mxfp6"
            names = ["own_split", "own_contiguous", "two_launch", "all_image"] + (["pack_split", "pack_contiguous"] if packs else [])
            for fan_in in FAN_INS:
                # Operand 0 is the own shard, operands 1..K-1 the images of streams 1..K-1 of the op.
                own_ops = [(d.data_ptr(), p.data_ptr(), [o.data_ptr()] + [im.data_ptr() for im in ims[1:fan_in]])
                           for d, p, o, ims in zip(dst, pdst, own, images)]
                image_ops = [(d.data_ptr(), [im.data_ptr() for im in ims[:fan_in]]) for d, ims in zip(dst, images)]
                unpack_ops = [(w.data_ptr(), im.data_ptr(), nbytes) for ims, ws in zip(images, wide)
                              for im, w in zip(ims[1:fan_in], ws)]
                reduce_ops = [(d.data_ptr(), [o.data_ptr()] + [w.data_ptr() for w in ws[:fan_in - 1]], nbytes)
                              for d, o, ws in zip(dst, own, wide)]
                for coherent in (False, True):
                    mask = ((1 << fan_in) - 2) if coherent else 0  # the incoming images; the own shard stays local

                    def fused(lanes):
                        for d, _, srcs in own_ops:
                            nat.wire_reduce(d, srcs, nbytes, fmt, st, mask, 0, lanes, True)

                    def packed(lanes):
                        for _, p, srcs in own_ops:
                            nat.wire_reduce_packed(p, srcs, nbytes, fmt, st, mask, 0, lanes, True)

                    def two_launch():
                        nat.wire_unpack_many(unpack_ops, fmt, st, coherent)
                        nat.reduce_many(reduce_ops, "bf16", st, False)

                    def all_image():
                        for d, srcs in image_ops:
                            nat.wire_reduce(d, srcs, nbytes, fmt, st, coherent, 0, "auto")

                    fns = [lambda: fused("split"), lambda: fused("contiguous"), two_launch, all_image]
                    if packs:
                        fns += [lambda: packed("split"), lambda: packed("contiguous")]
                    warm(fns, args.warm_seconds)
                    ms = dict(zip(names, alternate(fns, args.rounds)))
                    rec = {"shape": name, "bytes": nbytes, "ops": nops, "format": fmt, "wire_bytes": wb, "fan_in": fan_in,
                           "form": "coherent" if coherent else "local", "rounds": args.rounds, "memory": "one GPU: HBM, no xGMI",
                           "ms": ms}
                    line = "%-11s %-5s K=%d %-8s" % (name, fmt, fan_in, rec["form"])
                    for k, v in ms.items():
                        rec[k + "_payload_gbs"] = total / (statistics.median(v) * 1e-3) / 1e9
                        line += " | %s %5.0f" % (k, rec[k + "_payload_gbs"])
                    records.append(rec)
                    print(line + " GB/s", flush=True)
            del images, pdst
            torch.cuda.empty_cache()
        del dst, own, wide
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(records, f, indent=1)


if __name__ == "__main__":
    main()
