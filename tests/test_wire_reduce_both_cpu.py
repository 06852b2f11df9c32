"""--reduce-out both without a GPU: the shared requantised sum for mxfp6 against
the float64 / float32 PyTorch reference, the engine path through the host
transport (the image and the bf16 it widens to, both checked), and the
option's refusals."""
import json
import os
import subprocess

import pytest

from test_nccl_p2p_amd.ops import reference_wire_operands, reference_wire_pack, reference_wire_reduce_packed, words_to_bytes

SIZES = [64, 4032, 8192, 8256, 3 * 8192 + 192]


@pytest.mark.parametrize("own", [False, True], ids=["images", "own-bf16"])
@pytest.mark.parametrize("fan_in", [1, 2, 8])
def test_host_packed_sum_serves_mxfp6(native, fan_in, own):
    for nbytes in SIZES:
        ops = [reference_wire_operands(nbytes, 950 + k) for k in range(fan_in)]
        images = [bytes(reference_wire_pack(w, "mxfp6").numpy()) for w in ops]
        if own:
            images[0] = bytes(words_to_bytes(ops[0]).numpy())
        got = native.host_wire_reduce_packed(images, nbytes, "mxfp6", own_bf16=own)
        assert got == bytes(reference_wire_reduce_packed(ops, "mxfp6", own_bf16=own).numpy()), nbytes


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat", "--reduce", "bf16",
           "--size", "8256", "-n", "3", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,fmt,own", [(2, "mxfp8", False), (3, "mxfp6", False), (2, "mxfp6", True), (3, "mxfp4", False)])
def test_host_transport_stores_and_verifies_both(native, mpirun, host_build, tmp_path, n, fmt, own):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--reduce-wire", fmt, "--reduce-out", "both", "--mode", "ring,allpairs", "--json", str(js)] +
               (["--reduce-own", "bf16"] if own else []))
    assert out.returncode == 0 and "reduce-out=both" in out.stdout, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["reduce"]["out"] == {"format": fmt, "bytes": native.wire_bytes(8256, fmt), "both": True} for r in runs)
    assert all(("own" in r["reduce"]) == own for r in runs)


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_host_transport_fault_exits_2(mpirun, host_build, fault):
    out = _run(mpirun, host_build, 2, ["--reduce-wire", "mxfp6", "--reduce-out", "both", "--mode", "ring"], env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("args,named,reason", [
    (["--reduce-out", "both", "--transport", "host", "--reduce", "bf16"], "--reduce-out both", "needs --reduce bf16 --reduce-wire"),
    (["--reduce-out", "both", "--transport", "shm", "--reduce", "bf16", "--reduce-wire", "mxfp6"], "--reduce-out both", "sums no wire images"),
    (["--reduce-out", "both", "--transport", "ipc", "--reduce", "bf16", "--reduce-wire", "mxfp6", "--verify-inline"], "--reduce-out both",
     "--verify-inline"),
    (["--reduce-out", "all", "--transport", "host", "--reduce", "bf16", "--reduce-wire", "mxfp6"], "--reduce-out 'all'", "bf16, wire or both"),
    (["--reduce-out", "wire", "--transport", "host", "--reduce", "bf16", "--reduce-wire", "mxfp6"], "--reduce-out wire", "--reduce-out both")])
def test_refusals_name_their_reason(native, args, named, reason):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))"] + args,
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and named in out.stderr and reason in out.stderr, (out.returncode, out.stderr[-500:])


def test_nothing_new_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--reduce-wire", "mxfp6", "--mode", "ring", "--json", str(js)])
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert out.returncode == 0 and runs and all("out" not in r["reduce"] for r in runs) and "reduce-out" not in out.stdout
