"""Tier T1, --load without a GPU: the option is refused where there is no GPU
to load or no quiet pass measured the same way, a bad KIND[:WGS] is a usage
error, --help lists it, the train arithmetic (load_plan) keeps its promises,
the extended table of a loaded record reads as documented, the PyTorch
reference of the matrix-core load has the properties its kernel test relies
on, and a run without the option has no trace of it."""
import json
import math
import os
import subprocess

import pytest
import torch

from test_nccl_p2p_amd.ops.load import (operand_values, reference_hbm_sum, reference_mfma_tiles,
                                        reference_operands)


def cli(exe, args, timeout=120, env=None):
    return subprocess.run([exe] + args, capture_output=True, text=True, timeout=timeout,
                          env=dict(os.environ, **(env or {})))


@pytest.fixture(scope="module")
def host_exe(host_build):
    return os.path.join(host_build, "p2p_matrix_host")


@pytest.mark.parametrize("args, why", [
    (["--transport", "host"], "--transport host"),
    (["--transport", "shm"], "--transport shm"),
    (["--transport", "rccl", "--reference"], "--reference"),
    (["--transport", "ipc", "--resume", "--json", "unused.json"], "--resume"),
])
def test_refusals_say_why(host_exe, args, why):
    out = cli(host_exe, ["--mode", "self", "--size", "64K", "-n", "2", "--load", "mfma"] + args)
    assert out.returncode == 1, (out.returncode, out.stderr[-2000:])
    assert "--load cannot be combined with " + why + ":" in out.stderr
    assert out.stdout == ""
    # The order of the options does not matter.
    out = cli(host_exe, args + ["--load=hbm:8", "--mode", "self"])
    assert out.returncode == 1 and "--load cannot be combined with " + why in out.stderr


@pytest.mark.parametrize("spec", ["gemm", "mfma:0", "hbm:-3", "mfma:", "mfma:4x", "", ":8", "hbm:1e3"])
def test_bad_spec_is_a_usage_error(host_exe, spec):
    out = cli(host_exe, ["--transport", "rccl", "--load", spec])
    assert out.returncode == 1, (spec, out.returncode)
    assert "--load" in out.stderr and "mfma|hbm[:WGS]" in out.stderr
    assert out.stdout == ""


def test_load_needs_a_value(host_exe):
    out = cli(host_exe, ["--transport", "rccl", "--load"])
    assert out.returncode == 1 and "--load needs a value" in out.stderr


def test_usage_names_the_option(native, host_exe):
    assert "--load KIND[:WGS]" in native.usage()
    out = cli(host_exe, ["--help"])
    assert out.returncode == 0 and "--load KIND[:WGS]" in out.stdout and "mfma" in out.stdout and "hbm" in out.stdout


# ---- load_plan ----

LAUNCH = [250e-6, 180e-6, 1.3e-3]
EXPECTED = [0.0, 1e-6, 2e-4, 3.3e-3, 0.05, 0.7, 1.9, 2.2, 30.0]


@pytest.mark.parametrize("launch_s", LAUNCH)
def test_load_plan_properties(native, launch_s):
    cap = native.MAX_LOAD_LAUNCHES
    assert cap == 16384
    prev = 0
    for e in EXPECTED:
        n, covers = native.load_plan(e, launch_s)
        assert 1 <= n <= cap
        assert n >= prev, "the count is monotone in expected_s"
        prev = n
        assert covers == pytest.approx(n * launch_s, rel=1e-12)
        if n < cap:
            assert covers >= 2 * e, "until the cap, the train covers twice the expected time"
            assert n == max(1, math.ceil(2 * e / launch_s))
        else:
            assert 2 * e / launch_s >= cap - 1
    assert native.load_plan(1e9, launch_s)[0] == cap
    assert native.load_plan(1.0, 0.0) == (0, 0.0)  # not calibrated: no train


# ---- the printer ----

def phase(label, agg, quiet, covered=True, launches=80, done=61, window=40, window_s=0.01, during=500.0, ranks=(0,)):
    return {"label": label, "agg_gbs": agg,
            "load": {"quiet_agg_gbs": quiet, "launches": launches, "launches_done": done, "window_launches": window,
                     "window_s": window_s, "during_rate": during, "covered": covered, "ranks": list(ranks)}}


def test_table_of_a_loaded_record(native):
    text = native.load_table("mfma", 256, 251.0, 600.0, "TFLOP/s",
                             [phase("0->1", 45.0, 50.0), phase("1->0", 50.0, 50.0, window=60, window_s=0.03, during=300.0)])
    lines = text.splitlines()
    assert lines[0] == "  under load, '0->1': 45.00 GB/s = 0.900 x quiet 50.00 GB/s"
    assert lines[1] == "  under load, '1->0': 50.00 GB/s = 1.000 x quiet 50.00 GB/s"
    # The load's rate over both windows, weighted by their lengths: (500 * 0.01 + 300 * 0.03) / 0.04 = 350.
    assert lines[2] == ("  load mfma, 256 workgroups, 251 us launches on rank(s) 0: alone 600.000 TFLOP/s, during the "
                        "windows 350.000 TFLOP/s (0.583 x); 100 launches in 0.0400 s of windows (122 of 160 enqueued ran)")
    assert len(lines) == 3 and "WARNING" not in text


def test_table_warns_when_a_train_ran_out(native):
    text = native.load_table("hbm", 64, 240.0, 3.1, "TB/s", [phase("self", 900.0, 1200.0, covered=False, ranks=(0, 2))])
    assert "0.750 x quiet" in text and "rank(s) 0,2" in text and "TB/s" in text
    assert text.splitlines()[-1].startswith("  WARNING: the load's train ran out before a window ended")
    assert native.load_table("hbm", 64, 240.0, 3.1, "TB/s", []) == ""


# ---- the references ----

def test_operands_are_exact_in_bf16_and_products_in_f32():
    w = torch.arange(0, 2**16, dtype=torch.int64) * 65521 + 7
    v = operand_values(w)
    assert set((v * 8).to(torch.int64).tolist()) == set(range(-15, 16))
    assert torch.equal(v.to(torch.bfloat16).to(torch.float32), v)
    a, b = reference_operands(3, 11)
    assert a.shape == (12, 32, 16) and b.shape == (12, 16, 32)
    # f32 accumulation in any order gives the f64 product: every partial sum is exact.
    assert torch.equal((a @ b).double(), a.double() @ b.double())


def test_reference_tiles_follow_the_cd_map():
    a, b = reference_operands(1, 5)
    t = reference_mfma_tiles(1, 5)
    assert t.shape == (4, 64, 16) and t.dtype == torch.float32
    c = a[2] @ b[2]
    for lane, reg in ((0, 0), (31, 3), (32, 0), (63, 15), (40, 9)):
        row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        assert t[2, lane, reg] == c[row, lane & 31]
    assert not torch.equal(t, reference_mfma_tiles(1, 6))
    assert not torch.equal(c, c.T)  # an asymmetric product: a transposed store would show


def test_reference_hbm_sum():
    data = torch.tensor([0xFFFFFFFF - 2**32, 1, 2, -1], dtype=torch.int32)
    assert reference_hbm_sum(data, 3) == 3 * (0xFFFFFFFF + 1 + 2 + 0xFFFFFFFF)


# ---- off means absent ----

def test_without_the_option_nothing_mentions_a_load(host_exe, tmp_path):
    js = tmp_path / "r.json"
    out = cli(host_exe, ["--transport", "host", "--mode", "self", "--size", "64K", "-n", "3", "--json", str(js)])
    assert out.returncode == 0, out.stderr[-2000:]
    assert "load" not in out.stdout

    def keys(o):
        if isinstance(o, dict):
            for k, v in o.items():
                yield k
                yield from keys(v)
        elif isinstance(o, list):
            for v in o:
                yield from keys(v)

    recs = [json.loads(l) for l in js.read_text().splitlines()]
    runs = [r for r in recs if r.get("type") == "run"]
    assert len(runs) == 1
    assert not [k for r in runs for k in keys(r) if "load" in k]
