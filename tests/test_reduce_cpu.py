"""--reduce without a GPU: the shared sum against the plain-PyTorch reference,
the operand map, and the engine path through the host transport."""
import json
import os
import subprocess

import pytest
import torch

from test_nccl_p2p_amd.ops import reference_operands, reference_reduce, words_to_bytes

DTYPES = ["u32", "f32", "bf16"]


def _bytes(words):
    return bytes(words_to_bytes(words).numpy())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 2, 8])
def test_host_reduce_matches_reference(native, dtype, k):
    for nbytes in (4, 12, 16, 4096, 4100):
        ops = [reference_operands(nbytes, 77 + 13 * i, dtype) for i in range(k)]
        assert native.host_reduce([_bytes(o) for o in ops], dtype) == _bytes(reference_reduce(ops, dtype)), nbytes


@pytest.mark.parametrize("dtype,shifts", [("f32", (0,)), ("bf16", (0, 16))])
def test_operands_are_finite_with_pinned_exponent(dtype, shifts):
    w = reference_operands(1 << 16, 5, dtype)
    for s in shifts:  # the exponent field of the f32, or of each bf16 half
        e = (w >> (s + (23 if dtype == "f32" else 7))) & 0xFF
        assert int(e.min()) >= 64 and int(e.max()) <= 127


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,mode,fan_in", [(2, "pair", 2), (2, "ring", 2), (2, "allpairs", 2),
                                           (4, "pair", 2), (4, "ring", 3), (4, "allpairs", 4)])
@pytest.mark.parametrize("dtype", ["u32", "bf16"])
def test_host_transport_reduces_and_verifies(mpirun, host_build, tmp_path, n, mode, fan_in, dtype):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--reduce", dtype, "--mode", mode, "--size", "4100", "-n", "3", "--verify",
                                       "--json", str(js)])
    assert out.returncode == 0, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["reduce"]["dtype"] == dtype and r["verify_coverage"] == 1.0 for r in runs)
    assert max(r["reduce"]["fan_in"] for r in runs) == fan_in


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_host_transport_reduce_faults_exit_2(mpirun, host_build, fault):
    out = _run(mpirun, host_build, 2, ["--reduce", "bf16", "--mode", "ring", "--size", "4100", "-n", "3", "--verify"],
               env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("args", [["--transport", "shm"], ["--transport", "rccl"], ["--transport", "ipc", "--ipc-engine", "sdma"],
                                  ["--transport", "host", "--size", "4098"], ["--transport", "ipc", "--verify-inline"],
                                  ["--transport", "host", "--diagnose", "1"], ["--transport", "host", "--reference"],
                                  ["--transport", "host", "--resume"]])
def test_refusals_name_the_option(native, args):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--reduce", "f32"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--reduce" in out.stderr, (out.returncode, out.stderr[-500:])


def test_no_reduce_key_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--mode", "ring", "--size", "4100", "-n", "2", "--verify", "--json", str(js)])
    assert out.returncode == 0 and '"reduce"' not in js.read_text()
