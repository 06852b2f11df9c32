"""--device-stream end to end on ONE MI355X through the IPC transport: the self
cell in one process, two and four processes sharing the GPU (their rings and
flags in each other's hipIpc-mapped pages), and Session.device_stream.

What is asserted is what the records say about themselves and what cannot be
otherwise: every pair of every round present in both directions, every vector
of the verification launch compared and none wrong, the rate identities, a
sender's span no longer than the host waited, no rate above the memory's
roof.  There is no floor on any rate: on one GPU the link is HBM, and the
numbers are in profiles/device_stream/.
"""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import MPIRUN, ROOT, ensure_built, free_port

pytestmark = pytest.mark.gpu

ROOF_GBS = 4000.0  # 8.0 TB/s HBM3E peak, read + write (tests/test_timing_gpu.py)
VERIFY_ITERS = 256


@pytest.fixture(scope="module")
def exe():
    ensure_built("gpu")
    return os.path.join(ROOT, "build", "p2p_matrix")


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b))


def stream_records(lines):
    recs = [json.loads(l)["device_stream"] for l in lines if '"device_stream"' in l]
    # Existing readers pick their lines by these substrings.
    assert not any('"latency"' in l or '"run"' in l for l in lines if '"device_stream"' in l)
    return recs


def check_records(recs, nranks, sizes, forms, channels, depth, iters, wall_s):
    """One record per (form, size), forms in order; each with every ordered
    pair (the self cell for one rank), verified, consistent and plausible."""
    assert [(r["form"], r["bytes"]) for r in recs] == [(f, b) for f in forms for b in sizes]
    pairs = {(0, 0)} if nranks == 1 else {(a, b) for a in range(nranks) for b in range(nranks) if a != b}
    for r in recs:
        assert (r["nranks"], r["channels"], r["depth"], r["iters"]) == (nranks, channels, depth, iters), r
        assert r["verify_iters"] == min(iters, VERIFY_ITERS) and r["wrong_vectors"] == 0
        cells = {(c["src"], c["dst"]): c for c in r["cells"]}
        assert set(cells) == pairs and len(r["cells"]) == len(pairs), sorted(cells)
        msgs = channels * iters
        for c in r["cells"]:
            print("STREAM %s %7d B  %d->%d  %.3f GB/s  %.3f Mmsg/s  gap p50 %.2f us  recv %.3f GB/s  wall/span %.1f" % (
                r["form"], r["bytes"], c["src"], c["dst"], c["gbs"], c["mmsgs"], c["gap_us"]["p50"], c["recv_gbs"],
                c["wall_s"] / c["span_s"]))
            assert c["wrong_vectors"] == 0
            assert c["checked_vectors"] == min(iters, VERIFY_ITERS) * (r["bytes"] // 16) * channels, c
            # The record's own identities; rates and spans carry nine digits.
            assert c["span_s"] > 0 and c["recv_span_s"] > 0
            assert rel(c["gbs"] * 1e9 * c["span_s"], msgs * r["bytes"]) <= 1e-6, c
            assert rel(c["mmsgs"] * 1e6 * c["span_s"], msgs) <= 1e-6, c
            assert rel(c["recv_gbs"] * 1e9 * c["recv_span_s"], channels * (iters - 1) * r["bytes"]) <= 1e-6, c
            assert c["gap_us"]["n"] == iters and 0 < c["gap_us"]["p50"] <= c["gap_us"]["p99"]
            # Channel 0's gaps lie inside the sender's span.
            assert c["gap_us"]["mean"] * iters * 1e-6 <= c["span_s"] * (1 + 1e-5), c
            # One GPU, one clock: the first arrival follows the sender's first stamp and the
            # last precedes its final credit, so the receiver's span lies inside the sender's.
            assert c["recv_span_s"] <= c["span_s"], c
            # A kernel cannot have run longer than the host waited for it.
            assert c["span_s"] <= c["wall_s"] <= wall_s, (c, wall_s)
            assert c["gbs"] <= ROOF_GBS and c["recv_gbs"] <= ROOF_GBS, c


@pytest.mark.parametrize("channels", [1, 4, 8])
def test_self_cell(exe, tmp_path, channels):
    """One process: senders and receivers of every channel in one launch
    (8 channels: 16 roles, as many as a launch carries)."""
    js = tmp_path / "r.json"
    t0 = time.perf_counter()
    out = subprocess.run([exe, "--transport", "ipc", "--mode", "self", "--size", "4K", "-n", "2", "--no-compat",
                          "--device-stream", "--stream-sizes", "16,4K,64K", "--stream-iters", "300",
                          "--stream-channels", str(channels), "--json", str(js)],
                         capture_output=True, text=True, timeout=120)
    wall_s = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    assert "== device stream, one direction at a time: %d channel(s) of depth 8" % channels in out.stdout
    assert "== device stream, both directions of a pair at once" in out.stdout
    check_records(stream_records(js.read_text().splitlines()), 1, [16, 4096, 65536], ["uni", "bi"], channels, 8, 300,
                  wall_s)


@pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")
@pytest.mark.parametrize("nranks", [2, 3, 4])
def test_ranks_on_one_gpu(exe, tmp_path, nranks):
    """Several processes on one GPU stream into each other's pages: every
    pair of every round, both directions, one at a time and both at once.
    With three ranks one of them sits out every round, and that run also asks
    for messages of 100 bytes: they are sent, checked and reported as 112
    bytes, 7 vectors each."""
    js = tmp_path / "r.json"
    odd = nranks == 3
    t0 = time.perf_counter()
    out = subprocess.run([MPIRUN, "-n", str(nranks), exe, "--transport", "ipc", "--device", "0", "--mode", "ring",
                          "--size", "4K", "-n", "2", "--no-compat", "--dir", "both", "--device-stream", "--stream-sizes",
                          "16,100,4K,64K" if odd else "16,4K,64K", "--stream-iters", "200", "--stream-channels", "2",
                          "--json", str(js), "--timeout",
                          "60"], capture_output=True, text=True, timeout=240)
    wall_s = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-3000:]
    assert "== device stream, one direction at a time: 2 channel(s) of depth 8" in out.stdout
    if nranks > 2:
        assert "device stream bi, 64K messages: GB/s (row = sender, col = receiver)" in out.stdout
    recs = stream_records(js.read_text().splitlines())
    check_records(recs, nranks, [16, 112, 4096, 65536] if odd else [16, 4096, 65536], ["uni", "bi"], 2, 8, 200, wall_s)
    if odd:
        assert all(c["checked_vectors"] == 200 * 7 * 2 for r in recs if r["bytes"] == 112 for c in r["cells"])
        assert sum(r["bytes"] == 112 for r in recs) == 2


def session_calls(nranks):
    script = os.path.join("tests", "scripts", "device_stream_session.py")
    cmd = [sys.executable, script] if nranks == 1 else [
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr",
        "127.0.0.1", "--master-port", str(free_port()), script]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=180, cwd=ROOT,
                         env=dict(os.environ, P2P_FUZZ_DEVICE="0", P2P_IPC_POOL="1G"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and lines[0]["world"] == nranks, out.stdout[-2000:]
    return lines[0]["calls"]


@pytest.mark.parametrize("nranks", [1, 2])
def test_session_device_stream(native, nranks):
    """Session.device_stream, twice on one session with different channel
    counts and depths: the page is laid out again in between."""
    calls = session_calls(nranks)
    assert len(calls) == 2
    for c in calls:
        a = c["call"]
        forms = ["uni", "bi"] if a["dir"] == "both" else [a["dir"]]
        check_records([r["device_stream"] for r in c["records"]], nranks, a["sizes"], forms, a["channels"], a["depth"],
                      a["iters"], c["wall_s"])


def test_session_refuses_what_the_kernel_refuses(native):
    import torch

    torch.cuda.set_device(0)
    s = native.Session(0, 1, device=0, transport="ipc", timeout_s=60)
    for kw, names in ((dict(sizes=[4096], depth=65), "depth 1..64"), (dict(sizes=[4096], channels=9), "1..8 channels"),
                      (dict(sizes=[2 << 20]), "1 MiB"), (dict(sizes=[1 << 20], depth=8), "at most 4 MiB")):
        with pytest.raises(RuntimeError, match=names.replace(".", r"\.")):
            s.device_stream(**kw)
    # The session is still good for a stream within the limits.
    rec = json.loads(s.device_stream([1040], depth=2, channels=1, iters=50, dir="uni"))
    assert rec[0]["device_stream"]["cells"][0]["checked_vectors"] == 50 * 65
    del s
