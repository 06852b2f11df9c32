"""--reduce-gate through the IPC pull engine: 2 and 4 processes on ONE MI355X
combine their own shard and the messages they pull from each other's
hipIpc-mapped send buffers in the gfx950 gated reduce kernel; every kept sum
is checked."""
import json
import os
import subprocess

import pytest

from conftest import MPIRUN, ROOT, ensure_built

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")]


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "build", "p2p_matrix")
    if not os.path.exists(path):
        ensure_built("gpu")
    return path


def _run(exe, n, args, env=None):
    cmd = [MPIRUN, "-n", str(n), exe, "--transport", "ipc", "--ipc-engine", "kernel", "--device", "0", "--no-compat",
           "--timeout", "60", "-n", "3", "--reduce", "bf16", "--reduce-gate", "512", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,fan_in", [(2, 2), (4, 4)])
def test_ipc_gated_sum_verifies(exe, tmp_path, n, fan_in):
    js = tmp_path / "r.json"
    out = _run(exe, n, ["--mode", "ring,allpairs", "--sizes", "5120,1M", "--json", str(js)])
    assert out.returncode == 0, out.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert len(runs) == 2 * 3  # sizes x (ring: uni + bi; allpairs)
    assert all(r["verify_coverage"] == 1.0 and r["reduce"]["gate"] == {"row_elems": 512} for r in runs)
    assert all(ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert max(r["reduce"]["fan_in"] for r in runs) == fan_in


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_ipc_gated_sum_faults_exit_2(exe, fault):
    out = _run(exe, 2, ["--mode", "ring", "--size", "1M"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_session_run_reduce_gate(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, reduce="bf16", reduce_gate=2048))
    assert run["reduce"] == {"dtype": "bf16", "fan_in": 2, "gate": {"row_elems": 2048}} and run["verify_coverage"] == 1.0
    assert all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="reduce_gate"):
        sess.run("self", "uni", 1 << 20, 1, 0, "events", True, reduce="bf16", reduce_gate=768)
