"""--reduce-out both through the IPC pull engine: 1, 2 and 8 processes on ONE
MI355X sum the images they pull from hipIpc-mapped send buffers and store, from
one launch of the gfx950 wire-reduce-pack kernels, the sum's image and the bf16
it widens to; both outputs of every kept generation are checked bit for bit."""
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
                                                       "-n", "3", "--reduce", "bf16", "--reduce-wire", fmt, "--reduce-out", "both",
                                                       "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,modes,fmt,own", [(1, "self", "mxfp6", False), (2, "ring,allpairs", "mxfp8", False),
                                             (2, "ring,allpairs", "mxfp6", True), (8, "allpairs", "mxfp4", False),
                                             (8, "allpairs", "mxfp6", False)])
def test_ipc_reduce_out_both_verifies(native, exe, tmp_path, n, modes, fmt, own):
    js = tmp_path / "r.json"
    res = _run(exe, n, fmt, ["--mode", modes, "--sizes", "8256,1M", "--json", str(js)] + (["--reduce-own", "bf16"] if own else []))
    assert res.returncode == 0 and "reduce-out=both" in res.stdout, res.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["out"] == {"format": fmt, "bytes": native.wire_bytes(r["bytes"], fmt), "both": True} for r in runs)
    assert all(("own" in r["reduce"]) == own for r in runs) and {r["bytes"] for r in runs} == {8256, 1 << 20}
    assert max(r["reduce"]["fan_in"] for r in runs) == (2 if n == 1 else n)  # self: own + own; allpairs: own + n - 1


def test_ipc_reduce_out_both_fault_exits_2(exe):
    out = _run(exe, 2, "mxfp6", ["--mode", "ring", "--size", "1M"], env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_session_run_reduce_out_both(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, reduce="bf16", reduce_wire="mxfp6", reduce_out="both"))
    assert run["reduce"]["out"]["both"] is True and run["verify_coverage"] == 1.0 and all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="reduce_out='wire'"):
        sess.run("self", "uni", 1 << 20, 1, 0, "events", True, reduce="bf16", reduce_wire="mxfp6", reduce_out="wire")
