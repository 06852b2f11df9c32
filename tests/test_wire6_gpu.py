"""mxfp6 through the IPC pull engine: 1, 2 and 8 processes on ONE MI355X pull
each other's 6-bit wire images from hipIpc-mapped send buffers and widen them
(--wire) or sum them (--reduce-wire) in the gfx950 kernels; every kept slot is
checked bit for bit."""
import json
import os
import subprocess

import pytest

from conftest import MPIRUN, ROOT, ensure_built

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")]

FMT = "mxfp6"
SIZE = 8256  # a full tile and a one-block (odd, padded) one
OPTION = {"wire": ["--wire", FMT], "reduce-wire": ["--reduce", "bf16", "--reduce-wire", FMT]}


@pytest.fixture(scope="module")
def exe():
    path = os.path.join(ROOT, "build", "p2p_matrix")
    if not os.path.exists(path):
        ensure_built("gpu")
    return path


def _run(exe, n, args, env=None):
    cmd = ([MPIRUN, "-n", str(n)] if n > 1 else []) + [exe, "--transport", "ipc", "--ipc-engine", "kernel", "--device", "0",
                                                       "--no-compat", "--timeout", "60", "-n", "3", "--size", str(SIZE),
                                                       "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, P2P_IPC_POOL="1G", **(env or {})))


@pytest.mark.parametrize("n,modes", [(1, "self"), (2, "pair,ring,allpairs"), (8, "ring,allpairs")])
@pytest.mark.parametrize("option", sorted(OPTION))
def test_ipc_verifies(native, exe, tmp_path, option, n, modes):
    js, reduce = tmp_path / "r.json", option == "reduce-wire"
    out = _run(exe, n, OPTION[option] + ["--mode", modes, "--json", str(js)])
    assert out.returncode == 0 and option + "=" + FMT in out.stdout, out.stderr[-3000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    wire = {"format": FMT, "payload_bytes": SIZE, "wire_bytes": native.wire_bytes(SIZE, FMT)}
    assert all((r["reduce"]["wire"] if reduce else r["wire"]) == wire and (not reduce or "wire" not in r) for r in runs)
    assert not reduce or max(r["reduce"]["fan_in"] for r in runs) == max(2, n)  # self: own + own; allpairs: own + n - 1


@pytest.mark.parametrize("option", sorted(OPTION))
def test_ipc_corrupt_exits_2(exe, option):
    out = _run(exe, 2, OPTION[option] + ["--mode", "ring"], env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-3000:]
