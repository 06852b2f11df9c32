"""Mismatch diagnosis on the CPU (csrc/diagnose.hpp): the C++ host
implementation against the PyTorch reference, the merge of granule records
into extents, and the whole path through p2p_matrix_host with injected faults
on both CPU transports.  tests/test_diagnose_gpu.py runs the same planted
damage through the gfx950 kernel."""
import json
import os
import subprocess

import pytest
import torch

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import given, settings, strategies as st  # noqa: E402

from test_nccl_p2p_amd.ops import GranuleRecord, reference_bytes, reference_diagnose  # noqa: E402

SEED = 0x1234_5678_9ABC_DEF0
OTHER_SEED = 0x0FED_CBA9_8765_4321
# The candidates every planted buffer is diagnosed with: another stream, and
# this one 4096 bytes further on and 4096 bytes earlier.
CANDS = [(OTHER_SEED, 0), (SEED, 4096), (SEED, -4096)]
SIZES = [0, 5, 16, 4096, 4096 * 3 + 7, 40 * 1024 + 7, 64 * 1024]
GRANULES = [4096, 8192]


def clean(nbytes, seed=SEED, extra=0):
    """The stream's first nbytes (+ extra) as a mutable uint8 tensor."""
    return reference_bytes(nbytes + extra, seed).clone()


def plant(nbytes, granule, seed=SEED):
    """A buffer of the stream `seed` with every kind of damage that fits:
    a zeroed range across the first granule boundary, one flipped bit, a
    range of OTHER_SEED's stream, ranges of the same stream from 4096 bytes
    further on / earlier, and a damaged partial last word.  At most 6 runs
    of damage, so no more than 8 extents.  Returns (uint8 tensor, what was
    planted: name -> (begin, end))."""
    stream = clean(nbytes, seed, extra=8192)
    other = reference_bytes(nbytes, OTHER_SEED)
    buf = stream[:nbytes].clone()
    planted = {}

    def put(name, begin, length, src):
        if begin >= 0 and begin + length <= nbytes - nbytes % 4:
            buf[begin:begin + length] = src
            planted[name] = (begin, begin + length)

    if nbytes >= 4:
        buf[1] ^= 0x08
        planted["bit"] = (0, 4)
    put("zero", granule - 40, 64, 0)
    put("other_seed", 1024, 256, other[1024:1024 + 256])
    put("further", 2048, 128, stream[2048 + 4096:2048 + 4096 + 128])
    put("earlier", 4096 + 512, 128, stream[512:512 + 128])
    if nbytes % 4:
        buf[nbytes - 1] ^= 0xFF
        planted["tail"] = (nbytes - nbytes % 4, nbytes)
    return buf, planted


def host_records(native, buf, seed, cands, granule):
    return [GranuleRecord(*r) for r in native.host_diagnose(bytes(buf.numpy().tobytes()), seed, cands, granule)]


# ------------------------------------------------- host against reference ----

@pytest.mark.parametrize("granule", GRANULES)
@pytest.mark.parametrize("nbytes", SIZES)
def test_host_matches_reference_on_planted_damage(native, nbytes, granule):
    buf, planted = plant(nbytes, granule)
    got = host_records(native, buf, SEED, CANDS, granule)
    want = reference_diagnose(buf, SEED, CANDS, granule)
    assert got == want
    total = lambda f: sum(getattr(r, f) for r in got)  # noqa: E731
    assert total("zero") == (16 if "zero" in planted else 0)
    assert total("cand0") == (64 if "other_seed" in planted else 0)
    assert total("cand1") == (32 if "further" in planted else 0)
    assert total("cand2") == (32 if "earlier" in planted else 0)
    assert total("other") == ("bit" in planted) + ("tail" in planted)
    if "bit" in planted and "tail" not in planted:
        assert total("flipped_bits") == 1
    if "zero" in planted:  # the zeroed range straddles the first granule boundary
        assert [r.index for r in got if r.zero] == [0, 1]
    assert host_records(native, clean(nbytes), SEED, CANDS, granule) == []


def test_partial_last_word_is_masked(native):
    """5 bytes: the second word has one byte.  A wrong byte past the end
    cannot be seen; a wrong last byte is one `other` word whose flipped bits
    are counted under the mask; a zero last byte is poison."""
    buf = clean(5)
    assert host_records(native, buf, SEED, [], 4096) == []
    buf[4] ^= 0x81
    want = [GranuleRecord(0, 4, 4, 0, 1, 2)]
    assert host_records(native, buf, SEED, [], 4096) == want == reference_diagnose(buf, SEED, [], 4096)
    if int(clean(5)[4]) != 0:
        buf[4] = 0
        want = [GranuleRecord(0, 4, 4, 1, 0, 0)]
        assert host_records(native, buf, SEED, [], 4096) == want == reference_diagnose(buf, SEED, [], 4096)
    # The partial word of a candidate matches under the same mask.
    buf = clean(5)
    buf[4] = reference_bytes(5, OTHER_SEED)[4]
    if int(buf[4]) not in (0, int(clean(5)[4])):
        assert host_records(native, buf, SEED, [(OTHER_SEED, 0)], 4096) == [GranuleRecord(0, 4, 4, 0, 0, 0, 1)]


def test_candidate_order_decides_ties(native):
    """A range that matches two candidates (the same one listed twice): the
    first in the list gets every word."""
    buf = clean(8192)
    buf[256:512] = reference_bytes(8192, OTHER_SEED)[256:512]
    cands = [(SEED ^ 1, 0), (OTHER_SEED, 0), (OTHER_SEED, 0)]
    got = host_records(native, buf, SEED, cands, 4096)
    assert got == reference_diagnose(buf, SEED, cands, 4096)
    assert got == [GranuleRecord(0, 256, 508, 0, 0, 0, 0, 64, 0)]


def test_negative_shifted_index_matches_nothing(native):
    """shift = -4096: the first 1024 words have no word to be compared with
    and fall through to `other`."""
    buf = clean(8192)
    buf[0:64] = reference_bytes(8192, OTHER_SEED)[0:64]
    got = host_records(native, buf, SEED, [(OTHER_SEED, -4096)], 4096)
    assert got == reference_diagnose(buf, SEED, [(OTHER_SEED, -4096)], 4096)
    assert (got[0].other, got[0].cand0) == (16, 0)


def test_bad_arguments_are_refused(native):
    with pytest.raises(ValueError):
        native.host_diagnose(b"\0" * 64, 1, [(2, 8)], 4096)       # shift not a multiple of 16
    with pytest.raises(ValueError):
        native.host_diagnose(b"\0" * 64, 1, [(2, 0)] * 7, 4096)   # more than 6 candidates
    with pytest.raises(ValueError):
        native.host_diagnose(b"\0" * 64, 1, [], 2048)             # granule below 4 KiB
    with pytest.raises(ValueError):
        native.host_diagnose(b"\0" * 64, 1, [], 12288)            # not a power of two
    assert native.MAX_DIAG_CANDIDATES == 6


def test_default_granule(native):
    g = native.diagnose_granule
    assert g(0) == g(1) == g(4096 * 65536) == 4096
    assert g(4096 * 65536 + 1) == 8192
    assert g(1 << 30) == 16384 and g((16 << 30) + 8192) == 512 * 1024


@st.composite
def damaged_buffers(draw, max_bytes=64 * 1024, granules=tuple(GRANULES)):
    nbytes = draw(st.integers(0, max_bytes))
    seed = draw(st.integers(0, 2**64 - 1))
    cands = draw(st.lists(st.tuples(st.integers(0, 2**64 - 1), st.integers(-512, 512).map(lambda s: 16 * s)),
                          max_size=6))
    if cands and draw(st.booleans()):
        cands[0] = (seed, cands[0][1] or 4096)  # the buffer's own stream, shifted
    buf = clean(nbytes, seed)
    if nbytes:
        for _ in range(draw(st.integers(0, 6))):
            begin = draw(st.integers(0, nbytes - 1))
            length = draw(st.integers(1, min(nbytes - begin, 9000)))
            kind = draw(st.integers(0, 2 + len(cands)))
            if kind == 0:
                buf[begin:begin + length] = 0
            elif kind == 1:
                buf[begin] ^= 1 << draw(st.integers(0, 7))
            elif kind == 2:
                buf[begin:begin + length] = draw(st.integers(1, 255))
            else:  # a copy of candidate kind - 3's stream at its shift, from the next word on
                cseed, shift = cands[kind - 3]
                begin = (begin + 3) // 4 * 4
                src = begin + shift
                if src >= 0 and begin < nbytes:
                    length = min(length, nbytes - begin)
                    buf[begin:begin + length] = reference_bytes(src + length, cseed)[src:src + length]
    return buf, seed, cands, draw(st.sampled_from(granules))


@settings(max_examples=60, deadline=None)
@given(damaged_buffers())
def test_host_matches_reference_on_random_damage(native, case):
    buf, seed, cands, granule = case
    assert host_records(native, buf, seed, cands, granule) == reference_diagnose(buf, seed, cands, granule)


# ------------------------------------------------------------------ extents --

def extents(native, buf, seed, cands, granule):
    recs = native.host_diagnose(bytes(buf.numpy().tobytes()), seed, cands, granule)
    return native.merge_extents(recs, buf.numel(), granule)


def test_extent_of_one_flipped_word(native):
    buf = clean(3 * 4096 + 7)
    buf[4096 + 101] ^= 0x40
    ext = extents(native, buf, SEED, CANDS, 4096)
    assert ext == [(4096 + 100, 4096 + 104, 0, 1, 1, 0, 0, 0, 0, 0, 0)]
    line = native.describe_extent(ext[0], buf.numel(), CANDS)
    assert line == "bytes [4196, 4200) of 12295: 1 word differs from every candidate in 1 bit"


def test_zero_run_across_three_granules_is_one_extent(native):
    buf = clean(5 * 4096)
    buf[4096 - 8:3 * 4096 + 12] = 0
    assert extents(native, buf, SEED, CANDS, 4096) == [(4096 - 8, 3 * 4096 + 12, (2 * 4096 + 20) // 4, 0, 0, 0, 0, 0, 0, 0, 0)]
    # ... also when the run ends in the partial last word, clipped to the buffer
    buf = clean(3 * 4096 + 7)
    buf[4096:] = 0
    assert extents(native, buf, SEED, CANDS, 4096) == [(4096, 3 * 4096 + 7, 2 * 1024 + 2, 0, 0, 0, 0, 0, 0, 0, 0)]


def test_adjacent_granules_with_different_classes_are_two_extents(native):
    buf = clean(4 * 4096)
    buf[4096:2 * 4096] = 0                                                   # granule 1: poison
    buf[2 * 4096:3 * 4096] = reference_bytes(4 * 4096, OTHER_SEED)[2 * 4096:3 * 4096]  # granule 2: candidate 0
    ext = extents(native, buf, SEED, CANDS, 4096)
    assert ext == [(4096, 2 * 4096, 1024, 0, 0, 0, 0, 0, 0, 0, 0), (2 * 4096, 3 * 4096, 0, 0, 0, 1024, 0, 0, 0, 0, 0)]
    assert native.describe_extent(ext[0], 4 * 4096, CANDS) == "bytes [4096, 8192) of 16384: 1024 words still poison (never written)"
    # Damaged granules that do not touch are separate extents of the same class.
    buf = clean(4 * 4096)
    buf[0:16] = 0
    buf[2 * 4096:2 * 4096 + 16] = 0
    assert [e[:3] for e in extents(native, buf, SEED, CANDS, 4096)] == [(0, 16, 4), (2 * 4096, 2 * 4096 + 16, 4)]


def test_nothing_damaged_gives_no_extents(native):
    assert extents(native, clean(3 * 4096 + 7), SEED, CANDS, 4096) == []
    assert extents(native, clean(0), SEED, CANDS, 4096) == []


def test_extent_text_names_what_a_candidate_stands_for(native):
    e = (16777216, 33554432, 0, 3, 3, 5, 6, 7, 0, 0, 0)
    cands = [(1, 0, 1, 2), (2, 16777216, 2), (3, 0, 3, 3)]  # (seed, shift, kind, value): generation 2, +16 MiB, rank 3
    line = native.describe_extent(e, 33554432, cands)
    assert line.startswith("bytes [16777216, 33554432) of 33554432:")
    assert "5 words match the sender's generation 2 (stale)" in line
    assert "6 words match the sender's stream 16777216 bytes further on (misplaced op)" in line
    assert "7 words match rank 3's payload (wrong sender)" in line
    assert "3 words differ from every candidate in 3 bits" in line
    z = native.describe_extent((16777216, 33554432, 4194304, 0, 0, 0, 0, 0, 0, 0, 0), 33554432, [])
    assert z == "bytes [16777216, 33554432) of 33554432: 4194304 words still poison (never written)"


# ------------------------------------------------------------ end to end ----

def run_host(host_build, mpirun, tmp_path, transport, fault=None, diagnose=4):
    js = tmp_path / ("%s_%s_%d.json" % (transport, (fault or "clean").replace("@", "_").replace(":", "_"), diagnose))
    cmd = [mpirun, "-n", "2", os.path.join(host_build, "p2p_matrix_host"), "--transport", transport, "--size", "64K",
           "-n", "3", "--verify", "--no-compat", "--json", str(js)]
    if diagnose:
        cmd += ["--diagnose", str(diagnose)]
    env = {k: v for k, v in os.environ.items() if k not in ("P2P_INJECT_FAULT", "P2P_DIAGNOSE")}
    if fault:
        env["P2P_INJECT_FAULT"] = fault
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env)
    runs = [json.loads(l) for l in js.read_text().splitlines() if '"type":"run"' in l]
    return out, runs, js.read_text()


def check_fault_run(out, runs, fault):
    """The assertions the CPU and the GPU end-to-end tests share."""
    assert out.returncode == 2, out.stderr[-3000:]
    err = out.stderr.splitlines()
    lines = [l for l in err if l.startswith("[p2p] diagnose ")]
    failed = [i for i, l in enumerate(err) if "VERIFICATION FAILED" in l]
    assert lines and len(failed) == 1 and err.index(lines[-1]) < failed[0], out.stderr[-3000:]
    found = [(ph, d) for r in runs for ph in r["phases"] for d in ph.get("diagnosis", [])]
    assert found and all(ph["mismatches"] > 0 for ph, _ in found)
    nbytes = runs[0]["bytes"]
    if fault.startswith("corrupt"):
        assert all("bytes [0, 64) of %d" % nbytes in l and "still poison" in l for l in lines), lines
        for _, d in found:
            (e,) = d["extents"]
            assert (e["begin"], e["end"], e["zero"], e["other"], sum(e["cand"])) == (0, 64, 16, 0, 0), d
            assert d["gen"] == 0
    elif fault.startswith("skip-some"):
        assert {d["gen"] for _, d in found} == {0, 2}  # -n 3: the even generations
        for _, d in found:
            (e,) = d["extents"]
            assert (e["begin"], e["end"], e["zero"], e["other"], sum(e["cand"])) == (0, nbytes, nbytes // 4, 0, 0), d
    elif fault.startswith("stale"):
        assert all("bytes [0, %d) of %d" % (nbytes, nbytes) in l and "generation 1 (stale)" in l for l in lines), lines
        for _, d in found:
            (e,) = d["extents"]
            assert (e["begin"], e["end"], e["zero"], e["other"], sum(e["cand"])) == (0, nbytes, 0, 0, nbytes // 4), d
            assert d["gen"] == 0


@pytest.mark.mpi
@pytest.mark.parametrize("fault", ["corrupt@1:1", "skip-some@1", "stale@1:1"])
@pytest.mark.parametrize("transport", ["host", "shm"])
def test_fault_is_diagnosed(host_build, mpirun, tmp_path, transport, fault):
    out, runs, _ = run_host(host_build, mpirun, tmp_path, transport, fault)
    check_fault_run(out, runs, fault)


@pytest.mark.mpi
@pytest.mark.parametrize("transport", ["host", "shm"])
def test_diagnosis_stays_off_unless_asked_for(host_build, mpirun, tmp_path, transport):
    out, runs, text = run_host(host_build, mpirun, tmp_path, transport, "corrupt@1:1", diagnose=0)
    assert out.returncode == 2 and "VERIFICATION FAILED" in out.stderr
    assert "diagnos" not in out.stderr and "diagnos" not in text and "diagnos" not in out.stdout


@pytest.mark.mpi
@pytest.mark.parametrize("transport", ["host", "shm"])
def test_clean_run_is_unaffected(host_build, mpirun, tmp_path, transport):
    out, runs, text = run_host(host_build, mpirun, tmp_path, transport)
    assert out.returncode == 0, out.stderr[-3000:]
    assert runs and "diagnosis" not in text and "[p2p] diagnose" not in out.stderr


@pytest.mark.mpi
def test_environment_sets_the_default(host_build, mpirun, tmp_path):
    js = tmp_path / "env.json"
    env = dict(os.environ, P2P_INJECT_FAULT="corrupt@1:1", P2P_DIAGNOSE="1")
    out = subprocess.run([mpirun, "-n", "2", os.path.join(host_build, "p2p_matrix_host"), "--transport", "shm", "--size",
                          "64K", "-n", "3", "--verify", "--no-compat", "-d", "uni", "--json", str(js)],
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 2 and out.stderr.count("[p2p] diagnose ") == 1, out.stderr[-2000:]


def test_help_lists_the_option(native):
    assert "--diagnose N" in native.usage() and "P2P_DIAGNOSE" in native.usage() and "stale" in native.usage()


def test_torch_is_only_the_reference():
    # reference_diagnose shares no code with the extension: pure torch ops.
    buf = clean(4096 + 5)
    buf[4096:] = 0
    assert reference_diagnose(buf, SEED, [], 4096) == [GranuleRecord(1, 4096, 4100, 2, 0, 0)]
    assert isinstance(buf, torch.Tensor)
