"""Helper of tests/test_device_stream_gpu.py: Session.device_stream over the IPC
transport, one rank or several under torchrun on one GPU.

    [torchrun --nproc-per-node N] tests/scripts/device_stream_session.py

Two calls on one session, the second with another channel count and depth, so
the transport lays its page out again between them.  Rank 0 prints one JSON
line: for each call its arguments, the records Session.device_stream returned
and the host's wall clock around the call.
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from test_nccl_p2p_amd.parallel.session import create_session  # noqa: E402

CALLS = [
    dict(sizes=[16, 1040, 4096], depth=4, channels=2, iters=200, dir="both"),
    dict(sizes=[65536], depth=8, channels=1, iters=300, dir="uni"),
]


def main():
    import torch
    device = int(os.environ.get("P2P_FUZZ_DEVICE", os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(device)
    sess = create_session("ipc", device=device, timeout_s=60.0)
    out = []
    for call in CALLS:
        sess.barrier()
        t0 = time.perf_counter()
        records = json.loads(sess.device_stream(**call))
        out.append(dict(call=call, wall_s=time.perf_counter() - t0, records=records))
    sess.barrier()
    if sess.rank == 0:
        sys.stdout.write(json.dumps({"world": sess.world, "calls": out}) + "\n")
        sys.stdout.flush()
    del sess


if __name__ == "__main__":
    main()
