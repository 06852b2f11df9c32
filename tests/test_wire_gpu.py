"""--wire through the IPC pull engine: 1, 2 and 4 processes on ONE MI355X pull
each other's MXFP8 / MXFP4 wire images from hipIpc-mapped send buffers and
widen them to bf16 in the gfx950 unpack kernel; every kept slot is checked."""
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


@pytest.mark.parametrize("n,modes", [(1, "self"), (2, "pair,ring,allpairs"), (4, "pair,ring,allpairs")])
@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4"])
def test_ipc_wire_verifies(native, exe, tmp_path, fmt, n, modes):
    js = tmp_path / "r.json"
    out = _run(exe, n, ["--wire", fmt, "--mode", modes, "--sizes", "8256,1M", "--verify", "--json", str(js)])
    assert out.returncode == 0 and "wire=" + fmt in out.stdout, out.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert len(runs) == 2 * (1 if n == 1 else 5)  # sizes x (pair, ring: uni + bi; allpairs)
    assert all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert sorted({(r["wire"]["format"], r["wire"]["payload_bytes"], r["wire"]["wire_bytes"]) for r in runs}) == \
        [(fmt, b, native.wire_bytes(b, fmt)) for b in (8256, 1 << 20)]


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_ipc_wire_faults_exit_2(exe, fault):
    out = _run(exe, 2, ["--wire", "mxfp8", "--mode", "ring", "--size", "1M", "--verify"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]


def test_session_run_wire(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run("self", "uni", 1 << 20, 3, 1, "events", True, wire="mxfp8"))
    assert run["wire"] == {"format": "mxfp8", "payload_bytes": 1 << 20, "wire_bytes": native.wire_bytes(1 << 20, "mxfp8")}
    assert run["verify_coverage"] == 1.0 and all(ph["mismatches"] == 0 for ph in run["phases"])
    with pytest.raises(Exception, match="wire"):
        sess.run("self", "uni", 4128, 1, 0, "events", True, wire="mxfp8")
