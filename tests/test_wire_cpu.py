"""--wire without a GPU: the shared pack / unpack against the float64 PyTorch
reference, the size identities, and the engine path through the host transport."""
import json
import os
import subprocess

import pytest

from test_nccl_p2p_amd.ops import reference_wire_operands, reference_wire_pack, reference_wire_roundtrip, words_to_bytes

FORMATS = ["mxfp8", "mxfp4"]
SIZES = [64, 128, 4032, 8192, 8192 + 64, 3 * 8192 + 192, (1 << 20) + 64]


@pytest.mark.parametrize("fmt", FORMATS)
def test_host_pack_and_unpack_match_reference(native, fmt):
    for nbytes in SIZES:
        w = reference_wire_operands(nbytes, 4242)
        image = bytes(reference_wire_pack(w, fmt).numpy())
        assert native.host_wire_pack(bytes(words_to_bytes(w).numpy()), fmt) == image, nbytes
        assert native.host_wire_unpack(image, nbytes, fmt) == bytes(reference_wire_roundtrip(w, fmt).numpy()), nbytes


def test_operands_are_normal_and_walk_the_binades():
    w = reference_wire_operands(1 << 16, 5)
    fields = set()
    for s in (7, 23):  # the exponent field of each half
        e = (w >> s) & 0xFF
        assert int(e.min()) >= 64 and int(e.max()) <= 110
        fields |= set(e.tolist())
    assert fields == set(range(64, 111))


@pytest.mark.parametrize("fmt,eb", [("mxfp8", 32), ("mxfp4", 16)])
def test_wire_bytes_identities(native, fmt, eb):
    full = 128 * eb + 128  # 4224 / 2176: a multiple of 16
    assert full % 16 == 0 and native.wire_bytes(0, fmt) == 0 and native.wire_bytes(8192, fmt) == full
    for blocks in (1, 15, 16, 17, 127, 128, 129, 255, 256, 257, 3 * 128 + 5):
        rest = blocks % 128
        want = blocks // 128 * full + -(-(rest * (eb + 1)) // 16) * 16
        assert native.wire_bytes(64 * blocks, fmt) == want, blocks
    with pytest.raises(ValueError, match="64"):
        native.wire_bytes(96, fmt)


def _run(mpirun, host_build, n, args, env=None):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, **(env or {})))


@pytest.mark.parametrize("n,modes", [(2, "pair,ring,allpairs"), (3, "ring,allpairs")])
@pytest.mark.parametrize("fmt", FORMATS)
def test_host_transport_unpacks_and_verifies(native, mpirun, host_build, tmp_path, n, modes, fmt):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, n, ["--wire", fmt, "--mode", modes, "--size", "8256", "-n", "3", "--verify", "--json", str(js)])
    assert out.returncode == 0 and "wire=" + fmt in out.stdout, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    assert all(r["wire"] == {"format": fmt, "payload_bytes": 8256, "wire_bytes": native.wire_bytes(8256, fmt)} for r in runs)


@pytest.mark.parametrize("fault", ["corrupt@1", "skip@1"])
def test_host_transport_wire_faults_exit_2(mpirun, host_build, fault):
    out = _run(mpirun, host_build, 2, ["--wire", "mxfp4", "--mode", "ring", "--size", "8256", "-n", "3", "--verify"],
               env={"P2P_INJECT_FAULT": fault})
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr, out.stderr[-2000:]


@pytest.mark.parametrize("args,reason", [
    (["--transport", "shm"], "widens nothing"), (["--transport", "rccl"], "widens nothing"),
    (["--transport", "ipc", "--ipc-engine", "sdma"], "widens nothing"),
    (["--transport", "host", "--size", "4128"], "not a multiple of 64"),
    (["--transport", "host", "--reduce", "bf16"], "--reduce"), (["--transport", "ipc", "--verify-inline"], "--verify-inline"),
    (["--transport", "host", "--diagnose", "1"], "--diagnose"), (["--transport", "host", "--reference"], "--reference"),
    (["--transport", "host", "--resume"], "--resume")])
def test_refusals_name_their_reason(native, args, reason):
    # run_cli parses before it starts anything: a refusal is exit status 1.
    out = subprocess.run([os.sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--wire", "mxfp8"] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--wire" in out.stderr and reason in out.stderr, (out.returncode, out.stderr[-500:])


def test_no_wire_key_without_the_option(mpirun, host_build, tmp_path):
    js = tmp_path / "r.json"
    out = _run(mpirun, host_build, 2, ["--mode", "ring", "--size", "8256", "-n", "2", "--verify", "--json", str(js)])
    assert out.returncode == 0 and '"wire"' not in js.read_text() and "wire" not in out.stdout
