"""--verify-inline through the IPC transport on ONE MI355X: the pull engine's
copy kernel checks every timed delivery as it moves it, so coverage is 1.0
whatever number of receive generations the memory budget allows, and a
payload that is wrong at the source shows up in every delivery that carried
it, not only in the slot the check after timing still finds it in."""
import json
import os
import subprocess

import pytest

from conftest import MPIRUN, ROOT, ensure_built

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not os.path.exists(MPIRUN), reason="no mpirun")]

SUPPORTED = "--transport ipc --ipc-engine kernel"
PAIR = ["--mode", "pair", "--dir", "uni", "--cells", "0-1", "--size", "1M", "-n", "6"]


@pytest.fixture(scope="module")
def exe():
    ensure_built("gpu")
    return os.path.join(ROOT, "build", "p2p_matrix")


def launch(exe, nranks, args, tmp_path, env=None, engine="kernel"):
    """The run's CompletedProcess and its JSON run records."""
    js = tmp_path / "r.json"
    cmd = ([MPIRUN, "-n", str(nranks)] if nranks > 1 else []) + [
        exe, "--transport", "ipc", "--ipc-engine", engine, "--device", "0", "--no-compat", "--json", str(js),
        "--timeout", "60"] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, **(env or {})))
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l] if js.exists() else []
    return out, runs


def test_clean_one_rank(exe, tmp_path):
    out, runs = launch(exe, 1, ["--mode", "self", "--size", str((1 << 20) + 5), "-n", "6", "--verify-inline"], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "inline check: OK (0 mismatching words; 6 of 6 timed deliveries checked as they were copied)" in out.stdout
    (run,) = runs
    assert run["verify"] is True
    assert run["inline_coverage"] == 1.0 and run["inline_msgs"] == run["timed_msgs"] == 6
    assert run["inline_mismatches"] == 0 and run["inline_bad"] == []
    (ph,) = run["phases"]
    assert ph["inline_msgs"] == 6 and ph["inline_mismatches"] == 0 and ph["mismatches"] == 0


def test_off_leaves_the_records_alone(exe, tmp_path):
    out, runs = launch(exe, 1, ["--mode", "self", "--size", "1M", "-n", "3"], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "inline check" not in out.stdout
    (run,) = runs
    assert not [k for k in list(run) + list(run["phases"][0]) if k.startswith("inline")]


def test_clean_two_ranks_every_mode(exe, tmp_path):
    out, runs = launch(exe, 2, ["--mode", "all", "--sizes", "4K:16M:4", "-n", "6", "--verify-inline"], tmp_path)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len(runs) == 7 * 7
    for r in runs:
        assert r["inline_coverage"] == 1.0 and r["inline_mismatches"] == 0
        for ph in r["phases"]:
            assert ph["inline_msgs"] == ph["timed_msgs"] > 0 and ph["inline_mismatches"] == 0 and ph["mismatches"] == 0


def test_inline_covers_what_the_budget_cannot(exe, tmp_path):
    """Memory for two receive generations: the check after timing sees 2 of
    the 6 timed deliveries, the inline check all 6."""
    out, runs = launch(exe, 2, PAIR + ["--verify-inline"], tmp_path, env={"P2P_VERIFY_BUDGET": "5M"})
    assert out.returncode == 0, out.stderr[-3000:]
    (run,) = runs
    (ph,) = run["phases"]
    assert ph["generations"] == 2
    assert ph["timed_msgs"] == 6 and ph["verified_msgs"] == 2 and ph["inline_msgs"] == 6
    assert run["verify_coverage"] < 1 and run["inline_coverage"] == 1.0
    assert ph["mismatches"] == 0 and ph["inline_mismatches"] == 0


def test_fault_at_the_source_shows_in_every_delivery(exe, tmp_path):
    """corrupt-send@0 with two generations: timed iterations 0, 2 and 4 pull
    from the damaged generation-0 region.  The inline check names each of
    them; the check after timing finds the one slot that kept the last."""
    out, runs = launch(exe, 2, PAIR + ["--verify-inline"], tmp_path,
                       env={"P2P_VERIFY_BUDGET": "5M", "P2P_INJECT_FAULT": "corrupt-send@0"})
    assert out.returncode == 2, out.stderr[-3000:]
    assert "VERIFICATION FAILED" in out.stderr and "inline check: FAILED" in out.stdout
    (run,) = runs
    (ph,) = run["phases"]
    G = ph["generations"]
    assert G == 2
    bad = ph["inline_bad"]
    assert [b["iteration"] for b in bad] == [i for i in range(6) if i % G == 0]
    w = bad[0]["words"]
    assert 1 <= w <= 16  # whatever the 64 zeroed bytes differ in
    assert all((b["src"], b["dst"], b["words"]) == (0, 1, w) and b["first_bad"] < 64 for b in bad)
    assert ph["inline_mismatches"] == w * len(bad) == run["inline_mismatches"]
    assert ph["mismatches"] - ph["inline_mismatches"] == w  # the generation-0 slot, after timing
    assert run["inline_bad"] == [dict(b, label=ph["label"]) for b in bad]
    assert "iteration 4" in out.stderr


def test_existing_faults_keep_their_detector(exe, tmp_path):
    out, runs = launch(exe, 2, PAIR + ["--verify-inline"], tmp_path, env={"P2P_INJECT_FAULT": "skip-some@1"})
    assert out.returncode == 2, out.stderr[-3000:]
    (ph,) = runs[0]["phases"]
    # A dropped pull checks nothing in flight; the poison it left is found after timing.
    assert ph["inline_mismatches"] == 0 and ph["mismatches"] > 0
    out, runs = launch(exe, 2, PAIR + ["--verify-inline"], tmp_path, env={"P2P_INJECT_FAULT": "corrupt@1"})
    assert out.returncode == 2, out.stderr[-3000:]
    (ph,) = runs[0]["phases"]
    # Damage done after delivery: only the memory check can see it.
    assert ph["inline_mismatches"] == 0 and 1 <= ph["mismatches"] <= 16


@pytest.mark.parametrize("engine", ["push", "sdma"])
def test_other_engines_refuse(exe, tmp_path, engine):
    out, runs = launch(exe, 2, PAIR + ["--verify-inline"], tmp_path, engine=engine)
    assert out.returncode == 1, (out.returncode, out.stderr[-2000:])
    assert SUPPORTED in out.stderr and not runs


def test_session_run(native):
    sess = native.Session(0, 1, device=0, transport="ipc")
    run = json.loads(sess.run(mode="self", bytes=1 << 20, iters=4, verify=True, inline_check=True))
    assert run["inline_msgs"] == run["timed_msgs"] == 4 and run["inline_coverage"] == 1.0
    assert run["inline_mismatches"] == 0 and run["inline_bad"] == []
    (ph,) = run["phases"]
    assert ph["inline_msgs"] == 4 and ph["mismatches"] == 0
    plain = json.loads(sess.run(mode="self", bytes=1 << 20, iters=4, verify=True))
    assert "inline_msgs" not in plain and "inline_msgs" not in plain["phases"][0]
    with pytest.raises(RuntimeError, match="inline_check"):
        sess.run(mode="self", bytes=1 << 20, iters=4, verify=False, inline_check=True)
    del sess
    sdma = native.Session(0, 1, device=0, transport="ipc:sdma")
    with pytest.raises(RuntimeError, match="inline_check"):
        sdma.run(mode="self", bytes=1 << 20, iters=4, verify=True, inline_check=True)
    del sdma
