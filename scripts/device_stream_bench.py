#!/usr/bin/env python3
"""Device-initiated stream sweep (--device-stream) on one GPU, with the
host-posted pull rates and the device ping-pong beside it.

    python scripts/device_stream_bench.py --out profiles/device_stream [--parent-exe PATH/p2p_matrix]

For the self cell (one process) and for two processes on one GPU (torchrun):

  * Session.device_stream over sizes 16 B -> 1 MiB (x4 steps), depth 1, 8 and
    32 (skipped where depth x bytes passes the 4 MiB cap) and 1, 4 and 8
    channels, --repeats timed calls each (default 5); a row is the median of
    each column over the repeats (cell 0 -> 0, or 0 -> 1 of the uni form);
  * Session.device_latency at every size up to its 64 KiB limit, in the same
    session: a depth-1 message plus its credit is one round trip, so the
    depth-1 gap is compared with twice the one-way time;
  * with --parent-exe (a p2p_matrix built from the commit before the stream
    existed), the host-posted pull of --transport ipc at 4 KiB -> 1 MiB with
    the same iteration count and events timing, and the ratio of the
    device-stream rate (depth 8, 1 channel) to it.

Writes <out>/device_stream_bench.json (everything) and device_stream_bench.txt
(the tables).  Nothing is asserted: these are records.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [16 << (2 * k) for k in range(9)]  # 16 B .. 1 MiB, x4
DEPTHS = [1, 8, 32]
CHANNELS = [1, 4, 8]
RING_CAP = 4 << 20
PING_MAX = 64 << 10
COLUMNS = ("gbs", "mmsgs", "gap_p50_us", "gap_p99_us", "recv_gbs")


def worker(args):
    """One rank of the sweep; rank 0 prints one JSON line per row."""
    import torch

    from test_nccl_p2p_amd.parallel.session import create_session

    device = int(os.environ.get("P2P_FUZZ_DEVICE", os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    sess = create_session("ipc", device=device, timeout_s=120.0)
    root = sess.rank == 0

    def emit(row):
        if root:
            sys.stdout.write(json.dumps(row) + "\n")
            sys.stdout.flush()

    for nbytes in [s for s in SIZES if s <= PING_MAX]:
        lat = json.loads(sess.device_latency(nbytes, args.iters, min(args.iters, 100)))
        emit({"kind": "pingpong", "bytes": nbytes, "one_way_us": lat["pairs"][0]["one_way_us"]})
    for depth in DEPTHS:
        sizes = [s for s in SIZES if depth * s <= RING_CAP]
        for channels in CHANNELS:
            reps = [json.loads(sess.device_stream(sizes, depth=depth, channels=channels, iters=args.iters, dir="uni"))
                    for _ in range(args.repeats)]
            for k, nbytes in enumerate(sizes):
                cells = [r[k]["device_stream"]["cells"][0] for r in reps]
                assert all(c["wrong_vectors"] == 0 for c in cells)
                vals = {"gbs": [c["gbs"] for c in cells], "mmsgs": [c["mmsgs"] for c in cells],
                        "gap_p50_us": [c["gap_us"]["p50"] for c in cells], "gap_p99_us": [c["gap_us"]["p99"] for c in cells],
                        "recv_gbs": [c["recv_gbs"] for c in cells]}
                row = {"kind": "stream", "bytes": nbytes, "depth": depth, "channels": channels, "iters": args.iters,
                       "repeats": args.repeats, "src": cells[0]["src"], "dst": cells[0]["dst"], "samples": vals}
                row.update({c: statistics.median(v) for c, v in vals.items()})
                emit(row)
    sess.barrier()
    del sess


def run_worker(nranks, args):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--iters", str(args.iters), "--repeats", str(args.repeats)]
    if nranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks),
               "--master-addr", "127.0.0.1", "--master-port", str(args.port)] + cmd[1:]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT,
                         env=dict(os.environ, P2P_FUZZ_DEVICE="0", P2P_IPC_POOL="1G"))
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("sweep with %d rank(s) failed (exit %d)" % (nranks, out.returncode))
    return [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]


def run_parent(nranks, args):
    """Host-posted pull rates of the parent's binary: {bytes: GB/s}."""
    js = os.path.join(args.out, "parent_host_posted_%d.jsonl" % nranks)
    tail = ["--transport", "ipc", "--sizes", "4K:1M:4", "-n", str(args.iters), "--timing", "events", "--dir", "uni",
            "--no-compat", "--json", js, "--timeout", "120"]
    if nranks == 1:
        cmd = [args.parent_exe, "--mode", "self"] + tail
    else:
        cmd = [args.mpirun, "-n", str(nranks), args.parent_exe, "--device", "0", "--mode", "pair"] + tail
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout, cwd=ROOT,
                         env=dict(os.environ, P2P_IPC_POOL="1G"))
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit("the parent's binary failed (exit %d)" % out.returncode)
    rates = {}
    for line in open(js):
        rec = json.loads(line)
        if rec.get("type") != "run":
            continue
        flows = [f for ph in rec["phases"] for f in ph["flows"] if (f["src"], f["dst"]) in ((0, 0), (0, 1))]
        rates[rec["bytes"]] = flows[0]["gbs"]
    return rates


def size_name(b):
    return "%dM" % (b >> 20) if b >= 1 << 20 else "%dK" % (b >> 10) if b >= 1 << 10 else "%d" % b


def tables(result):
    lines = []
    for cell in result["cells"]:
        rows = [r for r in cell["rows"] if r["kind"] == "stream"]
        ping = {r["bytes"]: r["one_way_us"]["p50"] for r in cell["rows"] if r["kind"] == "pingpong"}
        lines.append("== %s: %d messages per channel, median of %d timed launches ==" % (
            cell["name"], result["iters"], result["repeats"]))
        lines.append("%8s %5s %4s %10s %10s %11s %11s %10s" % ("size", "depth", "ch", "GB/s", "Mmsg/s", "gap p50 us",
                                                               "gap p99 us", "recv GB/s"))
        for r in rows:
            lines.append("%8s %5d %4d %10.3f %10.3f %11.2f %11.2f %10.3f" % (
                size_name(r["bytes"]), r["depth"], r["channels"], r["gbs"], r["mmsgs"], r["gap_p50_us"], r["gap_p99_us"],
                r["recv_gbs"]))
        lines.append("")
        lines.append("-- depth 1, 1 channel, against the device ping-pong of the same session --")
        lines.append("%8s %11s %16s %10s" % ("size", "gap p50 us", "one-way p50 us", "gap / one-way"))
        for r in rows:
            if r["depth"] == 1 and r["channels"] == 1 and r["bytes"] in ping:
                lines.append("%8s %11.2f %16.2f %10.2f" % (size_name(r["bytes"]), r["gap_p50_us"], ping[r["bytes"]],
                                                          r["gap_p50_us"] / ping[r["bytes"]]))
        if cell.get("parent_host_posted_gbs"):
            lines.append("")
            lines.append("-- depth 8, against the host-posted pull of the parent commit's binary (events timing) --")
            lines.append("%8s %16s %14s %14s %10s %10s" % ("size", "host-posted GB/s", "stream 1ch GB/s", "stream 8ch GB/s",
                                                          "1ch ratio", "8ch ratio"))
            for b, host in sorted((int(k), v) for k, v in cell["parent_host_posted_gbs"].items()):
                one = [r["gbs"] for r in rows if (r["bytes"], r["depth"], r["channels"]) == (b, 8, 1)]
                eight = [r["gbs"] for r in rows if (r["bytes"], r["depth"], r["channels"]) == (b, 8, 8)]
                if not one or not eight:
                    continue  # 1 MiB x depth 8 passes the ring cap
                lines.append("%8s %16.3f %14.3f %14.3f %10.2f %10.2f" % (size_name(b), host, one[0], eight[0], one[0] / host,
                                                                          eight[0] / host))
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/device_stream")
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-exe", default="", help="p2p_matrix built from the parent commit (host-posted comparison)")
    ap.add_argument("--mpirun", default=os.environ.get("P2P_MPIRUN", "/opt/conda/bin/mpirun"))
    ap.add_argument("--port", type=int, default=29611)
    ap.add_argument("--timeout", type=float, default=500.0)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    os.makedirs(args.out, exist_ok=True)
    result = {"iters": args.iters, "repeats": args.repeats, "columns": COLUMNS, "cells": []}
    for nranks, name in ((1, "self cell (one process, 0 -> 0)"), (2, "two processes on one GPU (0 -> 1)")):
        t0 = time.time()
        cell = {"name": name, "nranks": nranks, "rows": run_worker(nranks, args)}
        if args.parent_exe:
            cell["parent_host_posted_gbs"] = run_parent(nranks, args)
        cell["seconds"] = time.time() - t0
        result["cells"].append(cell)
        print("%s: %d rows in %.0f s" % (name, len(cell["rows"]), cell["seconds"]), flush=True)
    with open(os.path.join(args.out, "device_stream_bench.json"), "w") as f:
        json.dump(result, f)
        f.write("\n")
    text = tables(result)
    with open(os.path.join(args.out, "device_stream_bench.txt"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
