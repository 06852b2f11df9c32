"""--reduce-wire without a GPU: the shared sum of wire images against the
float64 / float32 PyTorch reference, and the engine path through the host
transport."""
import json
import os
import subprocess

import pytest

from test_nccl_p2p_amd.ops import reference_wire_operands, reference_wire_pack, reference_wire_reduce

FORMATS = ["mxfp8", "mxfp4"]
SIZES = [64, 4032, 8192, 8256, 3 * 8192 + 192]


@pytest.mark.parametrize("fan_in", [1, 2, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_sum_matches_reference(native, fmt, fan_in):
    for nbytes in SIZES:
        ops = [reference_wire_operands(nbytes, 900 + k) for k in range(fan_in)]
        images = [bytes(reference_wire_pack(w, fmt).numpy()) for w in ops]
        assert native.host_wire_reduce(images, nbytes, fmt) == bytes(reference_wire_reduce(ops, fmt).numpy()), nbytes


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,fmt", [(2, "mxfp8"), (3, "mxfp4")])
def test_host_transport_sums_and_verifies(native, mpirun, host_build, tmp_path, n, fmt):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--reduce", "bf16", "--reduce-wire", fmt, "--mode", "ring,allpairs", "--size", "8256",
                                       "-n", "3", "--verify", "--json", str(js)])
    assert out.returncode == 0 and "reduce-wire=" + fmt in out.stdout, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    wire = {"format": fmt, "payload_bytes": 8256, "wire_bytes": native.wire_bytes(8256, fmt)}
    assert all(r["reduce"] == {"dtype": "bf16", "fan_in": r["reduce"]["fan_in"], "wire": wire} and "wire" not in r for r in runs)
    assert max(r["reduce"]["fan_in"] for r in runs) == n  # allpairs: own + n - 1


def test_host_transport_fault_exits_2(mpirun, host_build):
    out = _run(mpirun, host_build, 2, ["--reduce", "bf16", "--reduce-wire", "mxfp4", "--mode", "ring", "--size", "8256", "-n", "3",
                                       "--verify"], env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("args,reason", [
    (["--transport", "host"], "needs --reduce bf16"), (["--transport", "host", "--reduce", "f32"], "payload is bf16"),
    (["--transport", "host", "--reduce", "u32"], "payload is bf16"),
    (["--transport", "host", "--reduce", "bf16", "--wire", "mxfp8"], "--wire"),
    (["--transport", "shm", "--reduce", "bf16"], "sums no wire images"),
    (["--transport", "ipc", "--ipc-engine", "sdma", "--reduce", "bf16"], "sums no wire images"),
    (["--transport", "host", "--reduce", "bf16", "--size", "4128"], "not a multiple of 64"),
    (["--transport", "ipc", "--reduce", "bf16", "--verify-inline"], "--verify-inline"),
    (["--transport", "host", "--reduce", "bf16", "--diagnose", "1"], "--diagnose"),
    (["--transport", "host", "--reduce", "bf16", "--reference"], "--reference"),
    (["--transport", "host", "--reduce", "bf16", "--resume"], "--resume")])
def test_refusals_name_their_reason(native, args, reason):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--reduce-wire", "mxfp8"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--reduce-wire" in out.stderr and reason in out.stderr, (out.returncode, out.stderr[-500:])


def test_nothing_new_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--reduce", "bf16", "--mode", "ring", "--size", "8256", "-n", "2", "--verify", "--json", str(js)])
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert out.returncode == 0 and runs and all(r["reduce"] == {"dtype": "bf16", "fan_in": 2} for r in runs)
    assert "wire" not in out.stdout
