"""Tier T3: the gfx950 diagnosis kernel (csrc/diagnose.hip) against the
PyTorch reference, on the smallest shapes at which it can go wrong: tails,
more than one workgroup, granules smaller and larger than a workgroup's
32 KiB unit, the grid-stride loop and the 2^32-word seam of the PRNG key.
These tests use the GPU from the pytest process, like tests/test_kernels_gpu.py;
the file sorts with it, after tests/test_ipc_gpu.py, whose 8-rank runs share
the one GPU with any context this process holds.  The whole path through
p2p_matrix is in tests/test_diagnose_gpu.py."""
import pytest
import torch

hypothesis = pytest.importorskip("hypothesis")
from hypothesis import HealthCheck, given, settings, strategies as st  # noqa: E402

from test_diagnose import CANDS, OTHER_SEED, SEED, clean, damaged_buffers, plant  # noqa: E402
from test_nccl_p2p_amd.ops import diagnose, diagnose_records, fill_, reference_diagnose, verify  # noqa: E402

pytestmark = pytest.mark.gpu

GPU_SETTINGS = settings(max_examples=60, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])


@pytest.fixture(scope="module", autouse=True)
def gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)
    return native


def on_gpu(buf):
    """A 16-byte aligned device copy (torch aligns allocations; an empty
    tensor has no storage to misalign)."""
    return buf.cuda() if buf.numel() else torch.empty(0, dtype=torch.uint8, device="cuda")


# 12 KiB + 7 at 4 KiB: one workgroup, three records and a tail.  40 KiB + 7 at
# 8 KiB: two workgroups, the first with four records in its LDS table.
# 72 KiB + 7 at 64 KiB: three workgroups, the first two share record 0.
@pytest.mark.parametrize("nbytes,granule", [(12 * 1024 + 7, 4096), (40 * 1024 + 7, 8192), (72 * 1024 + 7, 65536)])
def test_kernel_matches_reference_on_planted_damage(nbytes, granule):
    buf, planted = plant(nbytes, granule)
    assert {"bit", "zero", "other_seed", "further", "earlier", "tail"} == set(planted)
    got = diagnose_records(on_gpu(buf), SEED, CANDS, granule)
    assert got == reference_diagnose(buf, SEED, CANDS, granule)
    assert diagnose_records(on_gpu(clean(nbytes)), SEED, CANDS, granule) == []
    assert diagnose(on_gpu(clean(nbytes)), SEED, CANDS, granule) == []


def test_grid_stride_loop_gives_the_same_records():
    buf, _ = plant(64 * 1024, 4096)
    buf[40 * 1024:40 * 1024 + 64] = 0          # damage in the second unit too
    dev = on_gpu(buf)
    want = reference_diagnose(buf, SEED, CANDS, 4096)
    assert diagnose_records(dev, SEED, CANDS, 4096) == want
    for max_grid in (1, 2):
        assert diagnose_records(dev, SEED, CANDS, 4096, max_grid=max_grid) == want, max_grid
    # One workgroup walks both units that share the 64 KiB granule's record.
    assert diagnose_records(dev, SEED, CANDS, 65536, max_grid=1) == reference_diagnose(buf, SEED, CANDS, 65536)


@pytest.mark.parametrize("nbytes", [0, 5, 16])
def test_degenerate_sizes(gpu, nbytes):
    buf, _ = plant(nbytes, 4096)
    assert diagnose_records(on_gpu(buf), SEED, CANDS, 4096) == reference_diagnose(buf, SEED, CANDS, 4096)
    assert diagnose_records(on_gpu(clean(nbytes)), SEED, CANDS, 4096) == []
    host = gpu.merge_extents(gpu.host_diagnose(buf.numpy().tobytes(), SEED, CANDS), nbytes)
    assert len(host) == (nbytes > 0) and diagnose(on_gpu(buf), SEED, CANDS) == host


def test_damage_only_in_the_partial_last_word():
    nbytes = 3 * 4096 + 7
    buf = clean(nbytes)
    buf[nbytes - 1] ^= 0x10
    got = diagnose_records(on_gpu(buf), SEED, CANDS, 4096)
    assert got == reference_diagnose(buf, SEED, CANDS, 4096)
    assert [(r.index, r.first_bad, r.last_bad, r.other, r.flipped_bits) for r in got] == [(3, nbytes - 3, nbytes - 3, 1, 1)]
    assert diagnose(on_gpu(buf), SEED, CANDS, 4096)[0][:2] == (nbytes - 3, nbytes)


def test_fully_damaged_buffers():
    nbytes = 1 << 20
    six = [(SEED + 1 + k, 0) for k in range(5)] + [(OTHER_SEED, 0)]  # the matching stream comes last
    zero = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    got = diagnose_records(zero, SEED, six, 4096)
    assert got == reference_diagnose(zero, SEED, six, 4096)
    assert sum(r.zero for r in got) == verify(zero, SEED).mismatches == nbytes // 4
    full = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fill_(full, OTHER_SEED)
    got = diagnose_records(full, SEED, six, 4096)
    assert got == reference_diagnose(full, SEED, six, 4096)
    assert sum(r.cand5 for r in got) == verify(full, SEED).mismatches
    assert sum(r.zero + r.other + r.cand0 + r.cand1 + r.cand2 + r.cand3 + r.cand4 for r in got) == 0
    (ext,) = diagnose(full, SEED, six)
    assert ext[:2] == (0, nbytes) and ext.cand5 == nbytes // 4


def test_shift_across_the_2_to_32_word_seam():
    """16 GiB + 8 KiB: words from 2^32 on take their key from the next region
    of the stream.  A range copied from 4096 bytes earlier straddles byte
    2^34, so behind the seam the candidate's word comes from the region
    before it; a zeroed range straddles the seam too."""
    seam = 1 << 34
    nbytes = seam + 8192
    try:
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:  # pragma: no cover
        pytest.skip("cannot allocate 16 GiB + 8 KiB on this GPU: %s" % e)
    fill_(buf, SEED)
    buf[seam - 2048:seam + 2048] = buf[seam - 2048 - 4096:seam + 2048 - 4096].clone()
    buf[seam - 64:seam + 64] = 0
    cands = [(SEED, -4096)]
    granule = 512 * 1024
    got = diagnose_records(buf, SEED, cands)
    start = seam - granule
    want = reference_diagnose(buf[start:], SEED, cands, granule, start=start)
    assert got == want
    assert [(r.index, r.zero, r.cand0, r.other) for r in got] == [(seam // granule - 1, 16, 496, 0),
                                                                  (seam // granule, 16, 496, 0)]
    assert diagnose(buf, SEED, cands) == [(seam - 2048, seam + 2048, 32, 0, 0, 992, 0, 0, 0, 0, 0)]
    del buf
    torch.cuda.empty_cache()


@GPU_SETTINGS
@given(damaged_buffers(max_bytes=256 * 1024, granules=(4096, 8192, 65536)), st.sampled_from([0, 1, 3]))
def test_kernel_matches_reference_on_random_damage(case, max_grid):
    buf, seed, cands, granule = case
    got = diagnose_records(on_gpu(buf), seed, cands, granule, max_grid=max_grid)
    assert got == reference_diagnose(buf, seed, cands, granule)
