"""torchrun helper: the push / relay rendezvous observed live, with one rank's
stream held by a gate (tests/test_rendezvous_gpu.py).

    torchrun --nproc-per-node N tests/scripts/rendezvous_probe.py <transport> <case> [size]

One eager step whose only flow is 0 -> 1.  A rank arms a stream gate before
the step is posted, so its part of the rendezvous cannot run; the rank that
depends on it must then be seen busy at every poll until the gate is released:

    ready   rank 1 (the receiver) is held: rank 0, the writer, is parked in its
            pre-signal, because nobody has said the slot is ready;
    done    rank 0 (the writer) is held: rank 1 has posted ready and waits for
            `done`; after the release it checks the slot itself, before any
            barrier, so the data must be there when its own stream is;
    relay   rank 2 (a relay of the message) is held: rank 1 stays busy although
            the direct stripe and rank 3's have landed.

Three times, conditions and not measurements: the hold (HOLD_S) is far longer
than the unguarded step (a 1-4 MiB copy and two one-wave launches: tens of
microseconds), the gate's deadline (GATE_S) far longer than the hold, the
session's timeout far longer than that.  Nothing here is meant to expire; if
the gate does, the case fails.  Every rank prints one JSON line and stops at
its first failed step.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from test_nccl_p2p_amd import require_native  # noqa: E402
from test_nccl_p2p_amd.parallel.session import create_session  # noqa: E402

HOLD_S = 0.3
GATE_S = 5.0
SESSION_S = 60.0
# case -> (the rank whose stream is held, the rank that must stay busy, does the receiver check its slot itself)
CASES = {"ready": (1, 0, False), "done": (0, 1, True), "relay": (2, 1, True)}


def emit(out):
    # One write per line: the ranks share a pipe.
    sys.stdout.write(json.dumps(out) + "\n")
    sys.stdout.flush()


def main():
    transport, case = sys.argv[1], sys.argv[2]
    nat = require_native()
    size = nat.parse_size(sys.argv[3] if len(sys.argv) > 3 else "1M")
    held, watcher, local_check = CASES[case]
    rank = int(os.environ.get("RANK", 0))
    out = {"rank": rank, "case": case, "failed": None}
    state = {"sess": None, "armed": False}

    def fail(step, **more):
        out.update(failed=step, **more)
        if state["armed"]:
            state["sess"]._gate_release()  # never leave the stream held
        emit(out)
        sys.exit(2)

    import torch
    device = int(os.environ.get("P2P_FUZZ_DEVICE", os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    sess = state["sess"] = create_session(transport, device=device, timeout_s=SESSION_S)
    n = sess.world
    d = nat.StepDriver(sess, "pair", "uni", size, 1, True, False, False, depth=1, salt=5)
    steps = [k for k in range(d.phases) if d.phase_flows(k) == [(0, 1)]]
    if len(steps) != 1:
        fail("schedule", steps=steps)
    k = steps[0]
    if case == "relay":
        vias = [via for via, _, _ in nat.plan_routes(n, [(0, 1)], size)[0]]
        if held not in vias:
            fail("plan", vias=vias)
    d.connect()
    d.poison()

    if rank == held:
        if not sess._gate_arm(GATE_S):
            fail("arm")
        state["armed"] = True
    sess.barrier()
    d.step(k)
    if rank == watcher:
        polls, idle = 0, 0
        until = time.monotonic() + HOLD_S
        while time.monotonic() < until:
            idle += bool(sess._stream_idle())
            polls += 1
            time.sleep(0.001)
        out.update(polls=polls, idle_polls=idle)
        if idle or polls < 10:
            fail("hold")
    sess.barrier()
    if rank == held:
        sess._gate_release()
        state["armed"] = False
    d.sync()
    if local_check and rank == 1:
        # This rank's stream is done: the slot must hold the message now, with
        # no barrier or other collective in between to order anything.
        wrong, slots = 0, d.deliveries(k)
        for ptr, nbytes, src, msg in slots:
            wrong += nat.verify(ptr, nbytes, d.msg_seed(src, msg))[0]
        out.update(local_slots=len(slots), local_wrong=int(wrong))
        if wrong or len(slots) != 1:
            fail("local verify")
    if sess._gate_timed_out():
        fail("gate expired")
    err = sess._async_error()
    if err:
        fail("async error", error=err)
    sess.barrier()
    v = d.verify_steps(k, 1)
    out.update(mismatches=int(v["mismatches"]), verified_msgs=int(v["verified_msgs"]), timed_msgs=int(v["timed_msgs"]))
    if v["mismatches"] or v["verified_msgs"] != 1:
        fail("verify_steps")
    emit(out)
    del d, sess
    return 0


if __name__ == "__main__":
    sys.exit(main())
