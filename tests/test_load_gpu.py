"""--load on ONE MI355X: BackgroundLoad's train and its cancel, and the self
cell of both GPU transports measured quiet and then beside a matrix-core and
an HBM-streaming load.  What the load costs the cell, or the cell the load, is
reported, never asserted: these tests check that both passes ran, verified,
and that the window saw the load at work."""
import json
import os
import subprocess
import time

import pytest

from conftest import MPIRUN, ROOT, ensure_built

pytestmark = pytest.mark.gpu

SELF = ["--mode", "self", "--size", "64M", "-n", "64", "--no-compat"]
PHASE_LOAD_KEYS = {"quiet_agg_gbs", "launches", "launches_done", "window_launches", "window_s", "during_rate", "covered",
                   "ranks"}


@pytest.fixture(scope="module")
def exe():
    ensure_built("gpu")
    return os.path.join(ROOT, "build", "p2p_matrix")


def launch(exe, nranks, args, tmp_path, env=None):
    """The run's CompletedProcess and its JSON run records."""
    js = tmp_path / "r.json"
    cmd = ([MPIRUN, "-n", str(nranks)] if nranks > 1 else []) + [exe, "--device", "0", "--json", str(js),
                                                                 "--timeout", "60"] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, **(env or {})))
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l] if js.exists() else []
    return out, runs


def check_loaded(quiet, loaded, kind, wgs=None):
    assert "load" not in quiet and not [ph for ph in quiet["phases"] if "load" in ph]
    info = loaded["load"]
    assert set(info) == {"kind", "wgs", "launch_us", "alone_rate", "unit"}
    assert info["kind"] == kind and info["unit"] == {"mfma": "TFLOP/s", "hbm": "TB/s"}[kind]
    assert info["wgs"] == wgs if wgs else info["wgs"] >= 1
    assert info["launch_us"] > 0 and info["alone_rate"] > 0
    for key in ("mode", "dir", "bytes", "iters", "warmup", "timing", "verify", "timed_msgs", "verified_msgs",
                "verify_coverage"):
        assert loaded[key] == quiet[key], key
    assert len(loaded["phases"]) == len(quiet["phases"]) >= 1
    for q, ph in zip(quiet["phases"], loaded["phases"]):
        assert ph["label"] == q["label"] and ph["mismatches"] == 0 and q["mismatches"] == 0
        l = ph["load"]
        assert set(l) == PHASE_LOAD_KEYS
        assert l["quiet_agg_gbs"] == q["agg_gbs"]
        assert l["window_launches"] >= 1 and l["during_rate"] > 0 and l["window_s"] > 0
        assert 0 <= l["launches_done"] <= l["launches"] and l["window_launches"] <= l["launches_done"]
        assert isinstance(l["covered"], bool)
        print("LOAD %s %s %s: cell %.1f GB/s = %.3f x quiet; load %.3f %s during = %.3f x alone; covered %s"
              % (kind, ph["label"], loaded["bytes"], ph["agg_gbs"], ph["agg_gbs"] / q["agg_gbs"], l["during_rate"],
                 info["unit"], l["during_rate"] / info["alone_rate"], l["covered"]))


def test_background_load_trains_and_cancels(native):
    import torch
    torch.cuda.set_device(0)
    load = native.BackgroundLoad("mfma", 8)
    assert (load.kind, load.wgs, load.unit) == ("mfma", 8, "TFLOP/s")
    load.calibrate()
    assert load.alone_rate > 0 and load.launch_s > 0
    t0 = time.monotonic()
    load.start(0.5)
    st = load.stop()
    assert time.monotonic() - t0 < 2.0
    assert st["launches"] == native.load_plan(0.5, load.launch_s)[0]
    assert 0 <= st["launches_done"] < st["launches"], "the cancel cut the train"
    assert st["window_launches"] == 0 and st["window_s"] == 0  # no window was opened
    # A second train on the same object, a window around some work on another stream.
    from test_nccl_p2p_amd.ops import fill_
    t = torch.empty(256 << 20, dtype=torch.uint8, device="cuda:0")
    load.start(0.02)
    load.window_begin()
    for seed in range(4):
        fill_(t, seed)
    torch.cuda.synchronize()
    load.window_end()
    st = load.stop()
    assert st["window_s"] > 0 and st["launches"] == native.load_plan(0.02, load.launch_s)[0]
    assert 0 <= st["window_launches"] <= st["launches_done"] <= st["launches"]
    assert (st["during_rate"] > 0) == (st["window_launches"] > 0)
    del load


@pytest.mark.parametrize("transport", ["ipc", "rccl"])
@pytest.mark.parametrize("spec", ["mfma", "hbm:64"])
def test_self_cell_quiet_then_loaded(exe, tmp_path, transport, spec):
    out, runs = launch(exe, 1, SELF + ["--transport", transport, "--load", spec], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len(runs) == 2
    kind, _, wgs = spec.partition(":")
    check_loaded(runs[0], runs[1], kind, int(wgs) if wgs else None)
    # The extended tables: the quiet run, then the loaded one with its ratio and the load's line.
    assert out.stdout.count("== [self ") == 2 and " load=%s:" % kind in out.stdout
    assert "under load, '" in out.stdout and "x quiet" in out.stdout
    assert "  load %s, " % kind in out.stdout and "during the windows" in out.stdout
    assert out.stdout.count("verification: OK") == 2


@pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")
def test_ranks_sharing_a_gpu_run_one_load(exe, tmp_path):
    out, runs = launch(exe, 2, ["--transport", "ipc", "--mode", "pair", "--dir", "uni", "--cells", "0-1", "--size", "16M",
                                "-n", "16", "--no-compat", "--load", "mfma:32"], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len(runs) == 2
    check_loaded(runs[0], runs[1], "mfma", 32)
    (ph,) = runs[1]["phases"]
    assert ph["load"]["ranks"] == [0]


def test_session_run_with_a_load(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    quiet = json.loads(sess.run(mode="self", bytes=16 << 20, iters=16, verify=True))
    loaded = json.loads(sess.run(mode="self", bytes=16 << 20, iters=16, verify=True, load="mfma"))
    assert "load" not in quiet and "load" not in quiet["phases"][0]
    assert loaded["load"]["kind"] == "mfma" and loaded["load"]["alone_rate"] > 0
    (ph,) = loaded["phases"]
    assert set(ph["load"]) == PHASE_LOAD_KEYS and ph["load"]["ranks"] == [0]
    assert ph["load"]["window_launches"] >= 1 and ph["load"]["during_rate"] > 0 and ph["mismatches"] == 0
    assert loaded["verify_coverage"] == quiet["verify_coverage"]
    with pytest.raises(RuntimeError, match="load"):
        sess.run(mode="self", bytes=1 << 20, iters=4, load="gemm")
    del sess
    host = native.Session(0, 1, transport="host")
    with pytest.raises(RuntimeError, match="no GPU to load"):
        host.run(mode="self", bytes=1 << 16, iters=2, load="mfma")
    del host


def test_corruption_under_load_still_fails_the_run(exe, tmp_path):
    out, runs = launch(exe, 1, ["--transport", "ipc", "--mode", "self", "--size", "8M", "-n", "8", "--no-compat",
                                "--load", "mfma"], tmp_path, env={"P2P_INJECT_FAULT": "corrupt@0"})
    assert out.returncode == 2, (out.returncode, out.stderr[-3000:])
    assert "VERIFICATION FAILED" in out.stderr
    assert len(runs) == 2 and runs[1]["phases"][0]["mismatches"] > 0 and "load" in runs[1]
