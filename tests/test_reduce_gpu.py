"""--reduce through the IPC pull engine: 1, 2, 4 and 8 processes on ONE MI355X
sum their own shard and the messages they pull from each other's hipIpc-mapped
send buffers in the gfx950 reduce kernel; every kept sum is checked."""
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
    cmd = ([MPIRUN, "-n", str(n)] if n > 1 else []) + [exe, "--transport", "ipc", "--device", "0", "--no-compat",
                                                       "--timeout", "60", "-n", "3"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,modes,fan_in", [(1, "self", 2), (2, "pair,ring,allpairs", 2), (4, "pair,ring,allpairs", 4)])
@pytest.mark.parametrize("dtype", ["u32", "f32", "bf16"])
def test_ipc_reduce_verifies(exe, tmp_path, dtype, n, modes, fan_in):
    js = tmp_path / "r.json"
    out = _run(exe, n, ["--reduce", dtype, "--mode", modes, "--sizes", "4100,1M", "--verify", "--json", str(js)])
    assert out.returncode == 0, out.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert len(runs) == 2 * (1 if n == 1 else 5)  # sizes x (pair, ring: uni + bi; allpairs)
    assert all(r["verify_coverage"] == 1.0 and r["reduce"]["dtype"] == dtype for r in runs)
    assert all(ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert max(r["reduce"]["fan_in"] for r in runs) == fan_in


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_ipc_reduce_faults_exit_2(exe, fault):
    out = _run(exe, 2, ["--reduce", "bf16", "--mode", "ring", "--size", "1M", "--verify"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_eight_ranks_fan_in_eight(exe, tmp_path):
    js = tmp_path / "r.json"
    out = _run(exe, 8, ["--reduce", "f32", "--mode", "allpairs", "--size", "64K", "--verify", "--json", str(js)])
    assert out.returncode == 0, out.stderr[-3000:]
    (run,) = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert run["reduce"] == {"dtype": "f32", "fan_in": 8} and run["verify_coverage"] == 1.0
    assert all(ph["mismatches"] == 0 for ph in run["phases"])


def test_session_run_reduce(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, reduce="bf16"))
    assert run["reduce"] == {"dtype": "bf16", "fan_in": 2} and run["verify_coverage"] == 1.0
    assert all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="reduce"):
        sess.run("self", "uni", 4098, 1, 0, "events", True, reduce="bf16")
