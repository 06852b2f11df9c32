"""bench.py's plain run (no --full: the headline alone) and --dump-outputs:
what the last timed step delivered, written as .npy, identical from run to
run and equal to the senders' PRNG streams."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, free_port

# Fields the untimed sections fill in: null in a plain run.
SECTION_FIELDS = ("p50_latency_us", "p50_latency_preposted_us", "reference_semantics", "reference_semantics_stock",
                  "pair_serial_events", "method_ratio", "concurrency_ratio", "extras", "ipc_transport",
                  "xgmi_pair_sweep", "untimed_skipped")
SALT = 1  # bench/headline.py: the headline driver's payload salt


def run_bench(args, nproc=1, timeout=240):
    cmd = [sys.executable]
    if nproc > 1:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr",
                "127.0.0.1", "--master-port", str(free_port())]
    out = subprocess.run(cmd + ["bench.py", "--gpus", str(nproc)] + args, capture_output=True, text=True,
                         timeout=timeout, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def expected(nat, chunks, size):
    """The bytes the chunk table names, from the host reference of the fill
    kernel: message m of sender s is the PRNG stream msg_seed(s, m)
    (csrc/step_driver.cpp)."""
    streams, parts = {}, []
    for msg, src, off, length in chunks.astype(np.int64):
        key = (int(src), int(msg))
        if key not in streams:
            seed = nat.payload_seed(key[0], size, SALT * 1000003 + key[1] + 1)
            streams[key] = np.frombuffer(nat.host_fill(size, seed), dtype=np.uint8)
        parts.append(streams[key][off:off + length])
    return np.concatenate(parts).astype(np.float32)


def check_dump(nat, d, rank, size, msgs, senders):
    data = np.load(os.path.join(d, "recv_rank%d.npy" % rank))
    chunks = np.load(os.path.join(d, "recv_rank%d_chunks.npy" % rank))
    assert data.dtype == np.float32 and chunks.dtype == np.float64 and chunks.shape[1] == 4
    assert data.size == int(chunks[:, 3].sum()) and data.nbytes + chunks.nbytes <= 64 << 20
    # Every message of the step, from every sender, first and last chunk included.
    assert {(int(m), int(s)) for m, s in chunks[:, :2]} == {(m, s) for m in range(msgs) for s in senders}
    for m in range(msgs):
        mine = chunks[chunks[:, 0] == m]
        assert mine[:, 2].min() == 0 and (mine[:, 2] + mine[:, 3]).max() == size, (m, mine)
    assert np.array_equal(data, expected(nat, chunks, size))
    return data, chunks


@pytest.mark.parametrize("size,msgs,whole", [("6000", 3, True), ("4M", 4, False)])
def test_plain_run_ends_with_the_headline_and_dumps_its_last_step(native, tmp_path, size, msgs, whole):
    """No --full: the run times its steps and prints the line, no untimed
    section runs.  --steps sets the timed steps.  --dump-outputs writes the
    last step's deliveries (whole, or a fixed sample of 4 KiB chunks of every
    message), the same bytes in a second run, equal to the reference."""
    nbytes = native.parse_size(size)
    args = ["--steps", "3", "--warmup", "2", "--transport", "host", "--size", size, "--msgs", str(msgs)]
    r, out = run_bench(args + ["--dump-outputs", str(tmp_path / "a")])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r
    assert r["full"] is False and r["value"] > 0 and r["ms_per_step"] > 0 and r["verify_mismatches"] == 0
    assert r["steps"] == 3 and len(r["rank0_step_ms"]) == 3 and r["verify_detail"]["timed_msgs"] == 3 * msgs
    assert all(r[k] is None for k in SECTION_FIELDS), {k: r[k] for k in SECTION_FIELDS if r[k] is not None}
    names = [n for n, _ in r["timeline_s"]["entries"]]
    assert "headline/timed" in names and "headline/dump_outputs" in names
    assert not any(n.startswith(("section:", "agree:")) or n == "untimed" for n in names), names
    d = r["outputs_dumped"]
    assert d["step"] == 4 and d["messages"] == msgs and d["bytes_delivered"] == msgs * nbytes
    assert (d["bytes_sampled"] == d["bytes_delivered"]) == whole
    a, chunks = check_dump(native, str(tmp_path / "a"), 0, nbytes, msgs, [0])
    run_bench(args + ["--dump-outputs", str(tmp_path / "b")])
    assert np.array_equal(a, np.load(tmp_path / "b" / "recv_rank0.npy"))
    assert np.array_equal(chunks, np.load(tmp_path / "b" / "recv_rank0_chunks.npy"))


def test_full_runs_the_untimed_sections(native):
    r, _ = run_bench(["--full", "--steps", "3", "--warmup", "2", "--transport", "host", "--size", "64K", "--msgs", "2",
                      "--latency-iters", "10", "--sweep-max", "64K", "--ref-iters", "8"])
    assert r["full"] is True and r["outputs_dumped"] is None and r["p50_latency_us"] > 0
    assert r["reference_semantics"]["uni"]["gbs_mean"] > 0 and r["extras"]["self_sweep"] and r["ipc_transport"]


def test_dump_outputs_every_rank_writes_its_own(native, tmp_path):
    """Two ranks: each writes what its peer sent it in the last step."""
    r, _ = run_bench(["--steps", "2", "--warmup", "1", "--transport", "host", "--size", "64K", "--msgs", "2",
                      "--dump-outputs", str(tmp_path)], nproc=2)
    assert r["full"] is False and r["verify_mismatches"] == 0
    for rank in (0, 1):
        check_dump(native, str(tmp_path), rank, 64 << 10, 2, [1 - rank])


@pytest.mark.gpu
def test_plain_run_dumps_the_rccl_step_on_the_gpu(native, tmp_path):
    """The same through RCCL on the GPU: 4 x 4 MiB per step is over the
    whole-message limit, so the gfx950 copy kernel gathers the sampled chunks."""
    r, _ = run_bench(["--steps", "3", "--warmup", "1", "--size", "4M", "--msgs", "4", "--dump-outputs", str(tmp_path)])
    assert r["transport"] == "rccl" and r["full"] is False and r["verify_mismatches"] == 0
    assert all(r[k] is None for k in SECTION_FIELDS)
    assert r["outputs_dumped"]["bytes_sampled"] < r["outputs_dumped"]["bytes_delivered"] == 16 << 20
    check_dump(native, str(tmp_path), 0, 4 << 20, 4, [0])
