"""--reduce-out wire through the IPC pull engine: 1, 2, 4 and 8 processes on ONE
MI355X sum their own MXFP8 / MXFP4 image and the images they pull from
hipIpc-mapped send buffers and store the requantised sum, one launch of the
gfx950 wire-reduce-pack kernel; every kept image is checked bit for bit."""
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
                                                       "-n", "3", "--reduce", "bf16", "--reduce-wire", fmt, "--reduce-out", "wire",
                                                       "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,modes,fmt", [(1, "self", "mxfp8"), (2, "pair,ring,allpairs", "mxfp4"), (4, "pair,ring,allpairs", "mxfp8"),
                                         (8, "allpairs", "mxfp4")])
def test_ipc_reduce_out_wire_verifies(native, exe, tmp_path, n, modes, fmt):
    js = tmp_path / "r.json"
    out = _run(exe, n, fmt, ["--mode", modes, "--sizes", "8256,1M", "--json", str(js)])
    assert out.returncode == 0 and "reduce-out=wire" in out.stdout, out.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["out"] == {"format": fmt, "bytes": native.wire_bytes(r["bytes"], fmt)} for r in runs)
    assert {r["bytes"] for r in runs} == {8256, 1 << 20}
    assert max(r["reduce"]["fan_in"] for r in runs) == (2 if n == 1 else n)  # self: own + own; allpairs: own + n - 1


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_ipc_reduce_out_wire_faults_exit_2(exe, fault):
    out = _run(exe, 2, "mxfp8", ["--mode", "ring", "--size", "1M"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_session_run_reduce_out_wire(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, reduce="bf16", reduce_wire="mxfp8", reduce_out="wire"))
    assert run["reduce"]["out"] == {"format": "mxfp8", "bytes": native.wire_bytes(1 << 20, "mxfp8")}
    assert run["verify_coverage"] == 1.0 and all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="reduce_out"):
        sess.run("self", "uni", 1 << 20, 1, 0, "events", True, reduce="bf16", reduce_out="wire")
