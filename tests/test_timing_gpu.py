"""Tier T3: the times and rates the engine reports on ONE MI355X, bracketed by
clocks it does not own.

Two references, both hard bounds:

  * The host wall clock.  An event interval lies inside the host interval
    that posted it and waited for it, so a reported time is <= the host's
    time for the same window and a reported rate is >= bytes / wall.
  * The memory roof.  An on-GPU copy of B bytes reads B and writes B; at the
    8.0 TB/s HBM3E peak no self-path flow moves more than 4000 GB/s of
    payload.  Messages are 64 MiB over 32 distinct receive slots (2 GiB, far
    beyond the 256 MB Infinity Cache), so the cache cannot serve them.

Together they refuse a factor-of-two error in either direction and most
off-by-one-mark errors in the flattering one.  Every test prints the ratios
it measured (wall / event, reported GB/s / roof): how tight the bracket was.
"""
import json
import os
import subprocess
import time

import pytest
import torch

from conftest import MPIRUN, ROOT, ensure_built

pytestmark = pytest.mark.gpu

MSG = 64 << 20
ROOF_GBS = 4000.0  # 8.0 TB/s HBM3E peak, read + write
ITERS = 32
MSGS, DEPTH, STEPS = 8, 4, 4  # 4 steps x 8 messages: 32 receive slots


@pytest.fixture(scope="module")
def session(native, request):
    """(transport, its 1-rank session): one session alive at a time; pytest
    runs the tests of one transport together."""
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    s = native.Session(0, 1, device=0, transport=request.param, timeout_s=120)
    yield request.param, s
    del s


def on(*transports):
    return pytest.mark.parametrize("session", transports, indirect=True)


def rel(a, b):
    return abs(a - b) / max(abs(a), abs(b))


def check_identities(run, ph):
    """What the record says about itself; num() prints 6 digits."""
    nbytes, flows = run["bytes"], ph["flows"]
    for f in flows:
        assert rel(f["gbs"], nbytes / f["seconds"] / 1e9) <= 1e-5, f
        assert rel(f["gbps"], 8 * f["gbs"]) <= 1e-5, f
    assert rel(ph["agg_gbs"], nbytes * len(flows) / ph["seconds_per_iter"] / 1e9) <= 1e-5, ph
    assert rel(max(f["seconds"] for f in flows), ph["seconds_per_iter"]) <= 1e-5, ph


@on("rccl", "rccl:4", "ipc")
def test_run_events_between_wall_clock_and_roof(session):
    transport, s = session
    run = json.loads(s.run(mode="self", dir="uni", bytes=MSG, iters=ITERS, warmup=2, verify=True))
    (ph,) = run["phases"]
    (flow,) = ph["flows"]
    assert ph["mismatches"] == 0 and run["verify_coverage"] == 1 and ph["generations"] == ITERS, ph
    event_s, wall_s = ph["seconds_per_iter"] * ITERS, ph["wall_seconds"]
    print("TIMING run events %-7s wall/event %.3f  gbs %.1f  gbs/roof %.3f" %
          (transport, wall_s / event_s, flow["gbs"], flow["gbs"] / ROOF_GBS))
    assert event_s <= wall_s
    assert flow["gbs"] <= ROOF_GBS
    assert flow["gbs"] >= MSG * ITERS / wall_s / 1e9
    check_identities(run, ph)
    # With K communicators a sample is a round of K messages divided by K:
    # ITERS / K per-message samples, which tile the window when K divides it.
    k = int(transport.split(":")[1]) if ":" in transport else 1
    n = flow["iter_us"]["n"]
    assert n == ITERS // k
    assert rel(flow["iter_us"]["mean"] * n * k / 1e6, event_s) <= 1 / (2 * n), flow


@on("rccl", "rccl:4", "ipc")
def test_run_wallclock_between_wall_clock_and_roof(session):
    transport, s = session
    run = json.loads(s.run(mode="self", dir="uni", bytes=MSG, iters=ITERS, warmup=2, timing="wallclock", verify=True))
    (ph,) = run["phases"]
    (flow,) = ph["flows"]
    assert ph["mismatches"] == 0
    timed_s, wall_s = ph["seconds_per_iter"] * ITERS, ph["wall_seconds"]
    it = flow["iter_us"]
    print("TIMING run wallclock %-7s wall/timed %.4f  samples/timed %.3f  gbs %.1f  gbs/roof %.3f" %
          (transport, wall_s / timed_s, it["mean"] * it["n"] / 1e6 / timed_s, flow["gbs"], flow["gbs"] / ROOF_GBS))
    assert timed_s <= wall_s
    assert it["n"] == ITERS  # one host-timed sample per iteration, whatever the communicators
    assert it["mean"] * it["n"] / 1e6 <= timed_s
    assert flow["gbs"] <= ROOF_GBS
    check_identities(run, ph)


def bracket_steps(session, d, first, label):
    """run_steps(first, STEPS) between two hook marks and two host clock
    readings; the bounds of one run.  The host clock is read before the first
    mark is posted and after the last one was waited for, so the event
    interval lies inside the host's however the thread is scheduled."""
    t0 = time.perf_counter()
    a = session._mark()
    d.run_steps(first, STEPS)
    b = session._mark()
    d.sync()
    t1 = time.perf_counter()
    ms = d.step_ms()
    assert len(ms) == STEPS
    event_ms, wall_ms = session._elapsed_ms(a, b), (t1 - t0) * 1e3
    rates = [d.job_bytes_per_step(first + k) / (ms[k] * 1e-3) / 1e9 for k in range(STEPS)]
    print("TIMING steps %-16s steps/event %.4f  wall/event %.3f  best gbs %.1f  gbs/roof %.3f" %
          (label, sum(ms) / event_ms, wall_ms / event_ms, max(rates), max(rates) / ROOF_GBS))
    assert all(m > 0 for m in ms), ms
    assert sum(ms) <= event_ms <= wall_ms, (ms, event_ms, wall_ms)
    assert all(r <= ROOF_GBS for r in rates), rates
    v = d.verify_steps(first, STEPS)  # the timed work was the real work
    assert v["mismatches"] == 0 and v["timed_msgs"] == v["verified_msgs"] == STEPS * MSGS, v


@pytest.mark.parametrize("session,graph", [("rccl", False), ("rccl:4", False), ("ipc", False), ("ipc", True)],
                         indirect=["session"])
def test_step_driver_between_marks_and_wall_clock(native, session, graph):
    transport, session = session
    d = native.StepDriver(session, "self", "bi", MSG, msgs=MSGS, verify=True, batch=True, graph=graph, depth=DEPTH)
    assert d.depth == DEPTH and d.graphs == graph
    d.connect()
    label = transport + (" graph" if graph else "")
    bracket_steps(session, d, 0, label)
    # reset() hands the event slots out again: only the new steps are
    # reported, and the same bounds hold for them.
    d.reset()
    d.poison()
    bracket_steps(session, d, STEPS, label + " again")
    del d


@on("rccl:4", "rccl:8")
def test_marks_on_several_streams_add_up(native, session):
    """A mark on K communicators is an event on the main stream and on each
    side stream with pending work, later marks carrying the latest side event
    forward.  Intervals between consecutive marks must not be negative and
    must add up to the interval around them: a side-stream reference that is
    lost or taken from the wrong mark moves an interval by about a whole
    step, the tolerance is an eighth of one."""
    transport, session = session
    d = native.StepDriver(session, "self", "bi", MSG, msgs=MSGS, verify=True, batch=True, depth=DEPTH)
    d.connect()
    d.reset()
    t0 = time.perf_counter()
    marks = [session._mark()]
    for k in range(STEPS):
        d.step(k)
        marks.append(session._mark())
    d.sync()
    t1 = time.perf_counter()
    parts = [session._elapsed_ms(marks[i], marks[i + 1]) for i in range(STEPS)]
    whole = session._elapsed_ms(marks[0], marks[-1])
    step = whole / STEPS
    print("TIMING marks %-7s parts %s whole %.4f  wall/event %.3f" %
          (transport, " ".join("%.4f" % p for p in parts), whole, (t1 - t0) * 1e3 / whole))
    assert all(p >= 0 for p in parts), parts
    assert abs(sum(parts) - whole) <= step / (2 * STEPS), (parts, whole)
    assert whole <= (t1 - t0) * 1e3
    assert d.job_bytes_per_step(0) * STEPS / (whole * 1e-3) / 1e9 <= ROOF_GBS
    ms = d.step_ms()
    assert len(ms) == STEPS and sum(ms) <= whole, (ms, whole)
    assert d.verify_steps(0, STEPS)["mismatches"] == 0
    # Reused event slots: after a clear no earlier side event may stand in for
    # a stream, so a fresh pair of marks around one step obeys the same bounds.
    d.reset()
    session._clear_marks()
    t0 = time.perf_counter()
    m0 = session._mark()
    d.step(STEPS)
    m1 = session._mark()
    d.sync()
    t1 = time.perf_counter()
    one = session._elapsed_ms(m0, m1)
    (inner,) = d.step_ms()
    print("TIMING marks %-7s after clear: step %.4f  pair %.4f  wall %.4f  earlier steps %.4f" %
          (transport, inner, one, (t1 - t0) * 1e3, step))
    assert 0 <= inner <= one <= (t1 - t0) * 1e3
    assert d.job_bytes_per_step(STEPS) / (one * 1e-3) / 1e9 <= ROOF_GBS
    del d


@pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")
def test_two_ranks_on_one_gpu(tmp_path):
    """Two ranks of the CLI share the GPU, so no roof applies; the record's
    identities and the wall-clock bound do."""
    ensure_built("gpu")
    js = tmp_path / "r.json"
    iters = 16
    out = subprocess.run([MPIRUN, "-n", "2", os.path.join(ROOT, "build", "p2p_matrix"), "--transport", "ipc",
                          "--mode", "tournament", "--dir", "bi", "--size", "64M", "-n", str(iters), "--verify",
                          "--no-compat", "--json", str(js), "--device", "0", "--timeout", "60"],
                         capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    (run,) = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert run["bytes"] == MSG and run["iters"] == iters and run["timing"] == "events"
    (ph,) = run["phases"]
    assert ph["mismatches"] == 0 and sorted((f["src"], f["dst"]) for f in ph["flows"]) == [(0, 1), (1, 0)]
    print("TIMING two ranks wall/event %s" % " ".join("%.3f" % (ph["wall_seconds"] / (f["seconds"] * iters))
                                                      for f in ph["flows"]))
    assert rel(max(f["seconds"] for f in ph["flows"]), ph["seconds_per_iter"]) <= 1e-5
    for f in ph["flows"]:
        assert f["seconds"] * iters <= ph["wall_seconds"], (f, ph["wall_seconds"])
        assert f["iter_us"]["n"] == iters
    check_identities(run, ph)
