"""--reduce-out wire without a GPU: the shared requantised sum of wire images
against the float64 / float32 PyTorch reference, the engine path through the
host transport, and the option's refusals."""
import json
import os
import subprocess

import pytest

from test_nccl_p2p_amd.ops import reference_wire_operands, reference_wire_pack, reference_wire_reduce_packed

FORMATS = ["mxfp8", "mxfp4"]
SIZES = [64, 4032, 8192, 8256, 3 * 8192 + 192]


@pytest.mark.parametrize("fan_in", [1, 2, 8])
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_packed_sum_matches_reference(native, fmt, fan_in):
    for nbytes in SIZES:
        ops = [reference_wire_operands(nbytes, 900 + k) for k in range(fan_in)]
        images = [bytes(reference_wire_pack(w, fmt).numpy()) for w in ops]
        assert native.host_wire_reduce_packed(images, nbytes, fmt) == bytes(reference_wire_reduce_packed(ops, fmt).numpy()), nbytes


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat", "--reduce", "bf16",
           "--size", "8256", "-n", "3", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,fmt", [(2, "mxfp8"), (3, "mxfp4")])
def test_host_transport_sums_packs_and_verifies(native, mpirun, host_build, tmp_path, n, fmt):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--reduce-wire", fmt, "--reduce-out", "wire", "--mode", "ring,allpairs", "--json", str(js)])
    assert out.returncode == 0 and "reduce-out=wire" in out.stdout, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["out"] == {"format": fmt, "bytes": native.wire_bytes(8256, fmt)} for r in runs)


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_host_transport_fault_exits_2(mpirun, host_build, fault):
    out = _run(mpirun, host_build, 2, ["--reduce-wire", "mxfp4", "--reduce-out", "wire", "--mode", "ring"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


OK = ["--transport", "host", "--reduce", "bf16", "--reduce-wire", "mxfp8"]


@pytest.mark.parametrize("args,reason", [
    (["--transport", "host"], "needs --reduce bf16 --reduce-wire"),
    (["--transport", "host", "--reduce", "bf16"], "needs --reduce bf16 --reduce-wire"),
    (["--transport", "host", "--reduce", "f32", "--reduce-wire", "mxfp8"], "needs --reduce bf16 --reduce-wire"),
    (["--transport", "shm", "--reduce", "bf16", "--reduce-wire", "mxfp8"], "sums no wire images"),
    (["--transport", "ipc", "--ipc-engine", "sdma", "--reduce", "bf16", "--reduce-wire", "mxfp8"], "sums no wire images"),
    (["--transport", "ipc", "--reduce", "bf16", "--reduce-wire", "mxfp8", "--verify-inline"], "--verify-inline"),
    (OK + ["--diagnose", "1"], "--diagnose"), (OK + ["--reference"], "--reference"), (OK + ["--resume"], "--resume")])
def test_refusals_name_their_reason(native, args, reason):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--reduce-out", "wire"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--reduce-out" in out.stderr and reason in out.stderr, (out.returncode, out.stderr[-500:])


def test_no_out_key_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--reduce-wire", "mxfp8", "--reduce-out", "bf16", "--mode", "ring", "--json", str(js)])
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert out.returncode == 0 and runs and all("out" not in r["reduce"] for r in runs) and "reduce-out" not in out.stdout
