"""--reduce-gate without a GPU: the shared gated sum against the plain-PyTorch
reference, the gate map, and the engine path through the host transport."""
import json
import os
import subprocess

import pytest
import torch

from test_nccl_p2p_amd.ops import reference_gated_reduce, reference_gates, reference_operands, words_to_bytes


def _bytes(words):
    return bytes(words_to_bytes(words).numpy())


@pytest.mark.parametrize("h", [512, 1536])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_host_gated_reduce_matches_reference(native, k, h):
    rows = 5
    ops = [reference_operands(rows * 2 * h, 77 + 13 * i, "bf16") for i in range(k)]
    gates = reference_gates(rows, 4242)
    assert native.host_gated_reduce([_bytes(o) for o in ops], _bytes(gates), h) == _bytes(reference_gated_reduce(ops, gates, h))


def test_gates_are_positive_and_in_range():
    w = reference_gates(1 << 14, 5)
    g = torch.cat([w & 0xFFFF, w >> 16]).to(torch.int16).view(torch.bfloat16).to(torch.float32)
    assert float(g.min()) >= 2.0**-4 and float(g.max()) < 1.0


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat",
           "--reduce", "bf16", "--reduce-gate", "512", "--size", "5120", "-n", "3", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,mode,fan_in", [(2, "ring", 2), (4, "ring", 3), (4, "allpairs", 4)])
def test_host_transport_gated_sum_verifies(mpirun, host_build, tmp_path, n, mode, fan_in):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--mode", mode, "--json", str(js)])
    assert out.returncode == 0, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["reduce"]["gate"] == {"row_elems": 512} and r["verify_coverage"] == 1.0 for r in runs)
    assert max(r["reduce"]["fan_in"] for r in runs) == fan_in


def test_host_transport_gated_fault_exits_2(mpirun, host_build):
    out = _run(mpirun, host_build, 2, ["--mode", "ring"], env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("args", [["--transport", "host", "--reduce-gate", "512", "--size", "5120"],  # no --reduce bf16
                                  ["--transport", "host", "--reduce", "f32", "--reduce-gate", "512", "--size", "5120"],
                                  ["--transport", "host", "--reduce", "bf16", "--reduce-gate", "768", "--size", "6144"],
                                  ["--transport", "host", "--reduce", "bf16", "--reduce-gate", "512", "--size", "5632"],
                                  ["--transport", "host", "--reduce", "bf16", "--reduce-gate", "512", "--size", "5120",
                                   "--reduce-wire", "mxfp8"],
                                  ["--transport", "shm", "--reduce", "bf16", "--reduce-gate", "512", "--size", "5120"],
                                  ["--transport", "ipc", "--ipc-engine", "sdma", "--reduce", "bf16", "--reduce-gate", "512",
                                   "--size", "5120"],
                                  ["--transport", "host", "--reduce", "bf16", "--reduce-gate", "512", "--size", "5120",
                                   "--diagnose", "1"]])
def test_refusals_name_the_option(native, args):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))"] + args,
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--reduce-gate" in out.stderr, (out.returncode, out.stderr[-500:])


def test_more_than_eight_operands_refused(mpirun, host_build):
    out = _run(mpirun, host_build, 9, ["--mode", "allpairs"])
    assert out.returncode == 1 and "--reduce-gate" in out.stderr, (out.returncode, out.stderr[-500:])
