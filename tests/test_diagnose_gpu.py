"""Tier T3: mismatch diagnosis end to end on the GPU transports: p2p_matrix
with injected faults and --diagnose, on RCCL (one rank) and on the IPC
transport (two ranks on one GPU).  Every test here starts the binary as a
child process and leaves the GPU alone itself: this file is collected before
tests/test_ipc_gpu.py, whose 8-rank runs share the one GPU with whatever
context the pytest process holds.  The kernel's own tests, which use the GPU
from this process, are in tests/test_kernels_diagnose_gpu.py, next to the
other in-process kernel tests."""
import json
import os
import subprocess

import pytest

from conftest import MPIRUN, ROOT, ensure_built
from test_diagnose import check_fault_run

pytestmark = pytest.mark.gpu


def run_gpu(tmp_path, args, fault, ranks):
    ensure_built("gpu")
    js = tmp_path / "r.json"
    cmd = [os.path.join(ROOT, "build", "p2p_matrix")] + args + ["--size", "1M", "-n", "3", "--verify", "--no-compat",
                                                                 "--diagnose", "2", "--timeout", "60", "--json", str(js)]
    if ranks > 1:
        cmd = [MPIRUN, "-n", str(ranks)] + cmd
    env = {k: v for k, v in os.environ.items() if k != "P2P_DIAGNOSE"}
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=dict(env, P2P_INJECT_FAULT=fault))
    return out, [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]


def test_skipped_deliveries_are_diagnosed_on_rccl(tmp_path):
    out, runs = run_gpu(tmp_path, ["--mode", "self"], "skip-some@0", 1)
    check_fault_run(out, runs, "skip-some@0")


@pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")
@pytest.mark.parametrize("fault", ["corrupt@1:1", "stale@1:1"])
def test_fault_is_diagnosed_on_ipc(tmp_path, fault):
    out, runs = run_gpu(tmp_path, ["--transport", "ipc", "--device", "0"], fault, 2)
    check_fault_run(out, runs, fault)
