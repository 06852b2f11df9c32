"""--device-stream without a GPU: the option is refused on the transports that
have no one-sided path, its limits are named at the command line, --help
lists it, a run without it prints nothing of it, and the page layout
(csrc/stream_layout.hpp through native.stream_layout) is aligned, disjoint
and complete over a grid of shapes."""
import itertools
import json
import os
import subprocess

import pytest

ONE_SIDED = "needs a one-sided transport (--transport ipc)"


@pytest.fixture(scope="module")
def exe(host_build):
    return os.path.join(host_build, "p2p_matrix_host")


def cli(exe, *args):
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("transport", ["host", "shm"])
def test_refused_without_a_one_sided_transport(exe, transport):
    """The wording and the exit status of --device-latency, before any rank starts."""
    out = cli(exe, "--transport", transport, "--size", "16K", "-n", "2", "--device-stream")
    assert out.returncode == 1, (out.returncode, out.stderr[-2000:])
    assert "--device-stream " + ONE_SIDED in out.stderr and "%s has none" % transport in out.stderr
    assert out.stdout == ""
    lat = cli(exe, "--transport", transport, "--size", "16K", "-n", "2", "--device-latency")
    assert lat.returncode == 1 and lat.stderr == out.stderr.replace("--device-stream", "--device-latency")


def test_refused_with_reference(exe):
    out = cli(exe, "--transport", "ipc", "--device-stream", "--reference")
    assert out.returncode == 1 and "--reference" in out.stderr and out.stdout == ""


BAD = [
    (["--stream-depth", "0"], "depth 1..64"),
    (["--stream-depth", "65"], "depth 1..64"),
    (["--stream-channels", "0"], "1..8 channels"),
    (["--stream-channels", "9"], "1..8 channels"),
    (["--stream-sizes", "2M"], "1 MiB"),
    (["--stream-depth", "2", "--stream-sizes", "16,4K,1M,2M"], "1 MiB"),
    (["--stream-sizes", "0"], "positive whole number of bytes"),
    (["--stream-depth", "64", "--stream-sizes", "128K"], "at most 4 MiB"),
    (["--stream-depth", "5", "--stream-sizes", "1M"], "at most 4 MiB"),
    (["--stream-iters", "0"], "1..100000"),
    (["--stream-iters", "100001"], "1..100000"),
    (["--stream-depth", "x"], "whole number"),
]


@pytest.mark.parametrize("args,names", BAD, ids=[" ".join(a) for a, _ in BAD])
def test_limits_are_named_at_the_command_line(exe, args, names):
    """The kernel's limits, checked while the command line is read (the host
    binary has no IPC transport to open: it never gets that far)."""
    out = cli(exe, "--transport", "ipc", "--device-stream", *args)
    assert out.returncode == 1, (out.returncode, out.stderr[-2000:])
    assert names in out.stderr, out.stderr
    assert out.stdout == ""


def test_limits_hold_at_their_edges(exe):
    """64 x 64K and 4 x 1M are exactly 4 MiB: accepted (--dry-run ends the
    program before it would open the IPC transport the host binary lacks)."""
    for args in (["--stream-depth", "64", "--stream-sizes", "64K"], ["--stream-depth", "4", "--stream-sizes", "1M"],
                 ["--stream-channels", "8", "--stream-iters", "100000"]):
        out = cli(exe, "--transport", "ipc", "--device-stream", "--dry-run", *args)
        assert out.returncode == 0, out.stderr[-2000:]


def test_stream_options_need_the_option(exe):
    out = cli(exe, "--transport", "host", "--stream-depth", "4")
    assert out.returncode == 1 and "need --device-stream" in out.stderr


def test_help_lists_the_options(exe):
    out = cli(exe, "--help")
    assert out.returncode == 0
    for opt in ("--device-stream", "--stream-sizes", "--stream-depth", "--stream-channels", "--stream-iters"):
        assert opt in out.stdout
    assert "[16:64K]" in out.stdout and "[2000]" in out.stdout


def test_a_run_without_the_option_says_nothing_of_it(exe, tmp_path):
    js = tmp_path / "r.json"
    out = cli(exe, "--transport", "host", "--mode", "self", "--size", "16K", "-n", "2", "--latency", "--latency-iters", "5",
              "--json", str(js))
    assert out.returncode == 0, out.stderr[-2000:]
    assert "device stream" not in out.stdout and "device_stream" not in out.stdout
    lines = js.read_text().splitlines()
    assert lines and all("device_stream" not in l for l in lines)
    assert all("device_stream" not in json.loads(l) for l in lines)


# ------------------------------------------------------------- the layout ----

GRID = list(itertools.product([1, 2, 3, 8], [1, 3, 8], [1, 2, 8, 64], [16, 24, 1040, 4096, 65536]))


def check_layout(lay, n, channels, depth, nbytes):
    sent = (nbytes + 15) // 16 * 16
    assert (lay["n"], lay["channels"], lay["depth"], lay["bytes"]) == (n, channels, depth, sent)
    assert lay["self_slot"] == n
    regions = lay["regions"]
    # A header and a ring per (source slot 0..n, channel), and the credit area.
    assert len(regions) == 2 * (n + 1) * channels + 1
    names = [r[0] for r in regions]
    assert len(set(names)) == len(names)
    assert "tail %d.%d" % (n, channels - 1) in names and "ring %d.0" % n in names and names[-1] == "credit"
    for name, off, size in regions:
        assert off % 256 == 0, (name, off)
        assert size > 0
    spans = sorted((off, off + size) for _, off, size in regions)
    assert spans[0][0] == 0
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, "regions overlap"
    # Nothing unaccounted for: the page is the sum of its regions.
    assert sum(size for _, _, size in regions) == lay["total"] == spans[-1][1]
    assert lay["total"] <= lay["cap"]
    where = dict((name, (off, size)) for name, off, size in regions)
    for r in range(n + 1):
        for c in range(channels):
            assert where["tail %d.%d" % (r, c)] == (lay["tail"][r][c], lay["header_bytes"])
            ring = where["ring %d.%d" % (r, c)]
            assert ring[0] == lay["ring"][r][c] == lay["tail"][r][c] + lay["header_bytes"]
            assert ring[1] == lay["ring_bytes"] >= depth * sent
    # One 128-byte head line per (destination slot 0..n, channel), inside the credit area.
    heads = sorted(h for row in lay["head"] for h in row)
    assert len(heads) == (n + 1) * channels and len(lay["head"]) == n + 1
    assert heads[0] == lay["credit_offset"] == where["credit"][0]
    assert all(b - a == lay["credit_line"] == 128 for a, b in zip(heads, heads[1:]))
    assert heads[-1] + 128 <= lay["credit_offset"] + lay["credit_bytes"]


@pytest.mark.parametrize("n,channels,depth,nbytes", [g for g in GRID if g[2] * ((g[3] + 15) // 16 * 16) <= 4 << 20])
def test_layout_is_aligned_disjoint_and_complete(native, n, channels, depth, nbytes):
    check_layout(native.stream_layout(n, channels, depth, nbytes), n, channels, depth, nbytes)


def test_layout_refuses_what_the_kernel_refuses(native):
    for args, names in (((2, 9, 8, 4096), "1..8 channels"), ((2, 0, 8, 4096), "1..8 channels"),
                        ((2, 1, 65, 16), "depth 1..64"), ((2, 1, 0, 16), "depth 1..64"),
                        ((2, 1, 1, (1 << 20) + 1), "1 MiB"), ((2, 1, 1, 0), "1 MiB"),
                        ((2, 1, 8, 1 << 20), "at most 4 MiB"), ((0, 1, 1, 16), "rank count"),
                        ((600, 8, 64, 65536), "cap")):
        with pytest.raises(ValueError, match=names.replace(".", r"\.")):
            native.stream_layout(*args)


def test_layout_properties(native):
    """The same properties over drawn shapes, where hypothesis is installed."""
    hyp = pytest.importorskip("hypothesis")
    st = hyp.strategies

    @hyp.settings(max_examples=150, deadline=None)
    @hyp.given(st.integers(1, 16), st.integers(1, 8), st.integers(1, 64), st.integers(1, 1 << 20))
    def prop(n, channels, depth, nbytes):
        hyp.assume(depth * ((nbytes + 15) // 16 * 16) <= 4 << 20)
        check_layout(native.stream_layout(n, channels, depth, nbytes), n, channels, depth, nbytes)

    prop()
