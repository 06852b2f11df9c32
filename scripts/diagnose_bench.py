#!/usr/bin/env python3
"""Rate of the diagnosis kernel (csrc/diagnose.hip) against the register-staged
verify on the same buffer, in one process: a clean buffer, an all-zero one and
one filled from the sixth candidate's seed (every candidate evaluated for
every word).  Sustained warm-up, then per round 20 event-timed launches of
each kernel, the two alternating round by round; the median per kernel.

    python scripts/diagnose_bench.py [--size 1G] [--rounds 3] [--json FILE]

Prints one JSON object: TB/s per case for both kernels and their ratio
(profiles/diagnose/README.md keeps a run)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from test_nccl_p2p_amd import require_native  # noqa: E402


def per_launch_ms(fn, reps=20):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    return [s.elapsed_time(e) for s, e in ev]


def warm(fn, seconds):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(16):
            fn()
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1G")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    nat = require_native()
    nbytes = nat.parse_size(args.size)
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream().cuda_stream
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    ptr = buf.data_ptr()
    seed = 11
    cands = [(100 + k, 0) for k in range(6)]
    cases = {"clean": lambda: nat.fill(ptr, nbytes, seed, stream, 0),
             "zero": lambda: buf.zero_(),
             "sixth_candidate": lambda: nat.fill(ptr, nbytes, cands[5][0], stream, 0)}

    def verify():
        nat.verify_launch(ptr, nbytes, seed, 2, True, stream)

    def diagnose():
        nat.diagnose_launch(ptr, nbytes, seed, cands, 0, stream)

    out = {"bytes": nbytes, "granule": nat.diagnose_granule(nbytes), "device": torch.cuda.get_device_name(0),
           "cases": {}}
    for name, prepare in cases.items():
        prepare()
        torch.cuda.synchronize()
        recs = nat.diagnose(ptr, nbytes, seed, cands, 0, stream)
        damaged = sum(sum(r[3:5]) + sum(r[6:]) for r in recs)
        assert damaged == nat.verify(ptr, nbytes, seed, 2, True, stream)[0], name
        warm(verify, 0.2)
        warm(diagnose, 0.2)
        ms = {"verify_stride": [], "diagnose": []}
        for r in range(args.rounds):
            order = [("verify_stride", verify), ("diagnose", diagnose)]
            for key, fn in (order if r % 2 == 0 else order[::-1]):
                ms[key] += per_launch_ms(fn)
        tbs = {k: nbytes / (statistics.median(v) * 1e-3) / 1e12 for k, v in ms.items()}
        out["cases"][name] = {"damaged_words": damaged, "verify_stride_tbs": round(tbs["verify_stride"], 3),
                              "diagnose_tbs": round(tbs["diagnose"], 3),
                              "diagnose_over_verify": round(tbs["diagnose"] / tbs["verify_stride"], 3),
                              "diagnose_ms_median": round(statistics.median(ms["diagnose"]), 4)}
    text = json.dumps(out)
    print(text)
    if args.json:
        with open(args.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
