"""T3r: the IPC push / relay rendezvous observed live on one MI355X.

The suite's other checks look at the receive slots after a sync and a host
barrier, when any order of the flags would have delivered the bytes.  Here one
rank's stream is held by a gate while a step is posted (tests/scripts/
rendezvous_probe.py): the rank that depends on it must be seen busy at every
poll of the hold, and a receiver whose own stream has finished must find its
slot complete before any collective call.  The flag protocol itself is checked
against a model in the host tests (T0r, tests/host/test_main.cpp)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, free_port

pytestmark = pytest.mark.gpu


def probe(nranks, transport, case, size):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nranks), "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "tests/scripts/rendezvous_probe.py", transport, case, size]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT,
                         env=dict(os.environ, P2P_FUZZ_DEVICE="0", P2P_IPC_POOL="1G"))
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(l)
    assert out.returncode == 0, (lines, out.stderr[-3000:])
    by_rank = {l["rank"]: l for l in lines}
    assert sorted(by_rank) == list(range(nranks)), lines
    for l in lines:
        assert l["failed"] is None and l["case"] == case, l
        assert l["mismatches"] == 0 and l["verified_msgs"] == l["timed_msgs"] == 1, l
    return by_rank


def held_busy(line):
    """The watching rank polled through the whole hold and never saw its stream idle."""
    return line["polls"] >= 10 and line["idle_polls"] == 0


def test_writer_waits_for_ready(native):
    """The receiver's stream is held, so it has not said `ready`: the writer's
    stream stays parked in its pre-signal and writes nothing."""
    r = probe(2, "ipc:push", "ready", "1M")
    assert held_busy(r[0]), r[0]


def test_receive_completes_after_the_data(native):
    """The writer's stream is held: the receiver has posted `ready` and waits
    for `done`.  Released, its own stream's end is enough for the slot to
    verify, with no barrier in between."""
    r = probe(2, "ipc:push", "done", "1M")
    assert held_busy(r[1]), r[1]
    assert r[1]["local_slots"] == 1 and r[1]["local_wrong"] == 0, r[1]


def test_receive_waits_for_every_relay(native):
    """Four ranks, one 4 MiB message 0 -> 1 in stripes through ranks 2 and 3:
    with rank 2 held, the receive does not complete although the direct
    stripe and rank 3's are free to land; afterwards the whole slot verifies."""
    r = probe(4, "ipc:relay", "relay", "4M")
    assert held_busy(r[1]), r[1]
    assert r[1]["local_slots"] == 1 and r[1]["local_wrong"] == 0, r[1]
