"""--reduce-own bf16 without a GPU: the shared sum of a bf16 own shard and wire
images against the float64 / float32 PyTorch reference, and the engine path
through the host transport."""
import json
import os
import subprocess

import pytest

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_pack, reference_wire_reduce,
                                   reference_wire_reduce_packed, words_to_bytes)

SIZES = [64, 4032, 8192 + 64, 2 * 8192 + 65 * 64, 3 * 8192 + 192]


@pytest.mark.parametrize("fan_in", [1, 2, 8])
@pytest.mark.parametrize("fmt,packed", [("mxfp8", False), ("mxfp6", False), ("mxfp4", False), ("mxfp8", True), ("mxfp4", True)])
def test_host_sum_matches_reference(native, fmt, packed, fan_in):
    host, ref = (native.host_wire_reduce_packed, reference_wire_reduce_packed) if packed else (native.host_wire_reduce, reference_wire_reduce)
    for nbytes in SIZES:
        ops = [reference_wire_operands(nbytes, 950 + k) for k in range(fan_in)]
        srcs = [bytes(words_to_bytes(ops[0]).numpy())] + [bytes(reference_wire_pack(w, fmt).numpy()) for w in ops[1:]]
        assert host(srcs, nbytes, fmt, own_bf16=True) == bytes(ref(ops, fmt, own_bf16=True).numpy()), nbytes


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat", "--reduce", "bf16",
           "--mode", "ring,allpairs", "--size", "8256", "-n", "3", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,fmt,out", [(2, "mxfp8", "bf16"), (3, "mxfp4", "bf16"), (3, "mxfp6", "bf16"), (2, "mxfp8", "wire"),
                                       (3, "mxfp8", "wire")])
def test_host_transport_sums_and_verifies(mpirun, host_build, tmp_path, n, fmt, out):
    js = tmp_path / "r.json"
    res = _run(mpirun, host_build, n, ["--reduce-wire", fmt, "--reduce-own", "bf16", "--reduce-out", out, "--json", str(js)])
    assert res.returncode == 0 and "reduce-own=bf16" in res.stdout, res.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["own"] == "bf16" and ("out" in r["reduce"]) == (out == "wire") for r in runs)
    assert max(r["reduce"]["fan_in"] for r in runs) == n  # allpairs: own + n - 1


@pytest.mark.parametrize("args,option,reason", [
    (["--reduce", "bf16"], "--reduce-own bf16", "needs --reduce bf16 --reduce-wire"),
    (["--reduce-wire", "mxfp8"], "--reduce-own bf16", "needs --reduce bf16 --reduce-wire"),
    (["--reduce", "bf16", "--reduce-wire", "mxfp8", "--reduce-own", "fp8"], "--reduce-own 'fp8'", "bf16 or wire"),
    (["--reduce", "bf16", "--reduce-wire", "mxfp6", "--reduce-out", "wire"], "--reduce-out wire", "mxfp6"),
    (["--reduce", "bf16", "--reduce-wire", "mxfp8", "--transport", "shm"], "--reduce-wire", "sums no wire images"),
    (["--reduce", "bf16", "--reduce-wire", "mxfp8", "--size", "4128"], "--reduce-wire", "not a multiple of 64"),
    (["--reduce", "bf16", "--reduce-wire", "mxfp8", "--diagnose", "1"], "--reduce-wire", "--diagnose")])
def test_refusals_name_their_reason(native, args, option, reason):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--transport", "host", "--reduce-own", "bf16"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and option in out.stderr and reason in out.stderr, (out.returncode, out.stderr[-500:])


def test_nothing_new_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--reduce-wire", "mxfp8", "--json", str(js)])
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert out.returncode == 0 and runs and all("own" not in r["reduce"] for r in runs) and "reduce-own" not in out.stdout
