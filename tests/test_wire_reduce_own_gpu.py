"""--reduce-own bf16 through the IPC pull engine: 1, 2 and 8 processes on ONE
MI355X add the images they pull from hipIpc-mapped send buffers to their own
bf16 shard in one launch of the gfx950 wire-reduce kernels; every kept sum, bf16
or requantised, is checked bit for bit."""
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


def _run(exe, n, fmt, args, env=None):
    cmd = ([MPIRUN, "-n", str(n)] if n > 1 else []) + [exe, "--transport", "ipc", "--device", "0", "--no-compat", "--timeout", "60",
                                                       "-n", "3", "--reduce", "bf16", "--reduce-wire", fmt, "--reduce-own", "bf16",
                                                       "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,modes,fmt,out", [(1, "self", "mxfp6", "bf16"), (2, "ring,allpairs", "mxfp8", "bf16"),
                                             (2, "ring,allpairs", "mxfp4", "wire"), (8, "allpairs", "mxfp4", "bf16"),
                                             (8, "allpairs", "mxfp6", "bf16"), (8, "allpairs", "mxfp8", "wire")])
def test_ipc_reduce_own_bf16_verifies(native, exe, tmp_path, n, modes, fmt, out):
    js = tmp_path / "r.json"
    res = _run(exe, n, fmt, ["--reduce-out", out, "--mode", modes, "--sizes", "8256,1M", "--json", str(js)])
    assert res.returncode == 0 and "reduce-own=bf16" in res.stdout, res.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["own"] == "bf16" and ("out" in r["reduce"]) == (out == "wire") for r in runs)
    assert {r["bytes"] for r in runs} == {8256, 1 << 20}
    assert max(r["reduce"]["fan_in"] for r in runs) == (2 if n == 1 else n)  # self: own + own; allpairs: own + n - 1


def test_ipc_reduce_own_bf16_fault_exits_2(exe):
    out = _run(exe, 2, "mxfp8", ["--mode", "ring", "--size", "1M"], env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_session_run_reduce_own_bf16(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, reduce="bf16", reduce_wire="mxfp4", reduce_own="bf16"))
    assert run["reduce"]["own"] == "bf16" and run["verify_coverage"] == 1.0 and all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="reduce_own"):
        sess.run("self", "uni", 1 << 20, 1, 0, "events", True, reduce="bf16", reduce_own="bf16")
