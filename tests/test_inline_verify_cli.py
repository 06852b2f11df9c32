"""Tier T1, --verify-inline without a GPU: the option is refused where no
kernel of the project's own moves the payload, --help lists it, the PyTorch
contract of the checked copy (reference_copy_check) agrees with the verify
contract it extends, and the corrupt-send fault is caught by the check after
timing on the host transport."""
import os
import subprocess

import pytest
import torch

from test_nccl_p2p_amd.ops import reference_bytes, reference_copy_check, reference_verify

NONE = 2**64 - 1
SUPPORTED = "--transport ipc --ipc-engine kernel"


def run(mpirun, exe, n, args, env=None, timeout=120):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([mpirun, "-n", str(n), exe] + args, capture_output=True, text=True, timeout=timeout, env=e)


@pytest.mark.mpi
def test_host_transport_refuses_inline(mpirun, host_build):
    """Every rank exits with the usage status before anything is allocated;
    the message names the combination that supports the option."""
    exe = os.path.join(host_build, "p2p_matrix_host")
    out = run(mpirun, exe, 2, ["--transport", "host", "--size", "64K", "-n", "3", "--verify-inline"])
    assert out.returncode == 1, (out.returncode, out.stderr[-2000:])
    assert SUPPORTED in out.stderr
    assert out.stdout == ""
    env = run(mpirun, exe, 2, ["--transport", "shm", "--size", "64K", "-n", "3"], env={"P2P_VERIFY_INLINE": "1"})
    assert env.returncode == 1 and SUPPORTED in env.stderr
    # --no-verify leaves nothing to compare with: the environment default is dropped, not refused.
    off = run(mpirun, exe, 2, ["--transport", "host", "--size", "64K", "-n", "3", "--no-verify", "--compat-only"],
              env={"P2P_VERIFY_INLINE": "1"})
    assert off.returncode == 0, off.stderr[-2000:]


def test_help_lists_the_option(host_build):
    exe = os.path.join(host_build, "p2p_matrix_host")
    out = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0
    assert "--verify-inline" in out.stdout and "P2P_VERIFY_INLINE" in out.stdout
    assert "corrupt-send" in out.stdout


@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, 4096, 4096 + 5, 3 * 4096 + 1024 + 16 * 37 + 5])
def test_reference_copy_check_is_reference_verify_at_offset_0(nbytes):
    buf = reference_bytes(nbytes, 77)
    assert reference_copy_check(buf, 77) == (0, NONE)
    for seed, flips in ((77, [0]), (77, [nbytes - 1]), (77, [nbytes // 2, nbytes - 1]), (78, [])):
        b = buf.clone()
        for off in flips:
            if nbytes:
                b[off] ^= 0x41
        want = reference_verify(b, seed)
        assert reference_copy_check(b, seed) == (want.mismatches, want.first_bad)


def test_reference_copy_check_at_an_offset():
    """A slice of the stream from a 4 KiB multiple on checks clean against that
    offset, wrong against any other, and reports stream bytes."""
    off, n = 3 * 4096, 2 * 4096 + 7
    part = reference_bytes(off + n, 5)[off:]
    assert reference_copy_check(part, 5, off) == (0, NONE)
    assert reference_copy_check(part, 5, 0).mismatches > 0
    part = part.clone()
    part[4097] ^= 1
    assert reference_copy_check(part, 5, off) == (1, off + 4096)


def test_reference_copy_check_agrees_with_host_verify(native):
    for nbytes in (1, 19, 4096 + 6, 70001):
        data = bytearray(bytes(reference_bytes(nbytes, 9).tolist()))
        assert native.host_verify(bytes(data), 9)[0] == 0
        assert bytes(native.host_fill(nbytes, 9)) == bytes(data)
        data[nbytes // 3] ^= 0x10
        data[nbytes - 1] ^= 0x80
        m, _, first = native.host_verify(bytes(data), 9)
        assert reference_copy_check(torch.tensor(list(data), dtype=torch.uint8), 9) == (m, first)


@pytest.mark.mpi
def test_corrupt_send_is_caught_after_timing_on_the_host_transport(mpirun, host_build):
    """corrupt-send@0: rank 0 zeroes the head of its generation-0 send region
    after the warmup.  With a generation per iteration the check after timing
    sees that delivery: exit 2."""
    exe = os.path.join(host_build, "p2p_matrix_host")
    out = run(mpirun, exe, 2, ["--transport", "host", "--size", "64K", "-n", "4", "-w", "2", "--verify", "--no-compat"],
              env={"P2P_INJECT_FAULT": "corrupt-send@0"})
    assert out.returncode == 2, out.stderr[-2000:]
    assert "VERIFICATION FAILED" in out.stderr and "generation-0 send region" in out.stderr
    ok = run(mpirun, exe, 2, ["--transport", "host", "--size", "64K", "-n", "4", "-w", "2", "--verify", "--no-compat"])
    assert ok.returncode == 0, ok.stderr[-2000:]
