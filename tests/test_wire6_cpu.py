"""mxfp6 (e2m3) as a wire format without a GPU: the shared pack / unpack / sum
against the float64 PyTorch reference, the padded tile formula, and the engine
path through the host transport."""
import json
import os
import subprocess
import sys

import pytest

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_pack, reference_wire_reduce,
                                   reference_wire_roundtrip, words_to_bytes)

FMT = "mxfp6"
SIZES = [64, 128, 4032, 8192, 8192 + 64, 3 * 8192 + 192, (1 << 20) + 64]


def test_host_pack_and_unpack_match_reference(native):
    for nbytes in SIZES:
        w = reference_wire_operands(nbytes, 4242)
        image = bytes(reference_wire_pack(w, FMT).numpy())
        assert native.host_wire_pack(bytes(words_to_bytes(w).numpy()), FMT) == image, nbytes
        assert native.host_wire_unpack(image, nbytes, FMT) == bytes(reference_wire_roundtrip(w, FMT).numpy()), nbytes


@pytest.mark.parametrize("fan_in", [1, 2, 8])
def test_host_sum_matches_reference(native, fan_in):
    for nbytes in SIZES[:-1]:
        ops = [reference_wire_operands(nbytes, 900 + k) for k in range(fan_in)]
        images = [bytes(reference_wire_pack(w, FMT).numpy()) for w in ops]
        assert native.host_wire_reduce(images, nbytes, FMT) == bytes(reference_wire_reduce(ops, FMT).numpy()), nbytes


def test_wire_bytes_identities(native):
    def align16(x):
        return -(-x // 16) * 16

    assert native.wire_bytes(0, FMT) == 0 and native.wire_bytes(8192, FMT) == 3200
    for fmt, eb in ((FMT, 24), ("mxfp8", 32), ("mxfp4", 16)):  # one formula; for 32 and 16 it is the unpadded one
        for blocks in (1, 2, 3, 15, 16, 17, 63, 127, 128, 129, 255, 257, 3 * 128 + 5):
            rest = blocks % 128
            want = blocks // 128 * (128 * eb + 128) + align16(align16(eb * rest) + rest)
            assert native.wire_bytes(64 * blocks, fmt) == want, (fmt, blocks)
            assert eb != 24 or len(reference_wire_pack(reference_wire_operands(64 * blocks, 1), fmt)) == want, blocks
            assert eb == 24 or want == blocks // 128 * (128 * eb + 128) + align16(rest * (eb + 1)), (fmt, blocks)


def _run(mpirun, host_build, n, args):
    cmd = [mpirun, "-n", str(n), os.path.join(host_build, "p2p_matrix_host"), "--transport", "host", "--no-compat",
           "--size", "8256", "-n", "3", "--verify"] + args
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("n,modes", [(2, "pair,ring,allpairs"), (3, "ring,allpairs")])
@pytest.mark.parametrize("reduce", [False, True], ids=["wire", "reduce-wire"])
def test_host_transport_verifies(native, mpirun, host_build, tmp_path, n, modes, reduce):
    js = tmp_path / "r.json"
    option = ["--reduce", "bf16", "--reduce-wire", FMT] if reduce else ["--wire", FMT]
    out = _run(mpirun, host_build, n, option + ["--mode", modes, "--json", str(js)])
    assert out.returncode == 0 and ("reduce-wire=" if reduce else "wire=") + FMT in out.stdout, out.stderr[-2000:]
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    assert runs and all(r["verify_coverage"] == 1.0 and ph["mismatches"] == 0 for r in runs for ph in r["phases"])
    wire = {"format": FMT, "payload_bytes": 8256, "wire_bytes": native.wire_bytes(8256, FMT)}
    assert all((r["reduce"]["wire"] if reduce else r["wire"]) == wire and (not reduce or "wire" not in r) for r in runs)
    assert not reduce or max(r["reduce"]["fan_in"] for r in runs) == n  # allpairs: own + n - 1


def test_reduce_out_wire_refusal_names_the_format(native):
    out = subprocess.run([sys.executable, "-c",
                          "import sys, test_nccl_p2p_amd as p; sys.exit(p.require_native().run_cli(sys.argv[1:]))",
                          "--transport", "host", "--reduce", "bf16", "--reduce-wire", FMT, "--reduce-out", "wire"],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and "--reduce-out wire" in out.stderr and FMT in out.stderr, (out.returncode, out.stderr[-500:])
