"""Tier T3: the arrays behind the raw-pointer checks (csrc/device_checks.hpp:
one DeviceChecks per device, each array a DeviceMirror) when they grow, on one
GPU.  A call that needs more results, records or granules than the arrays
hold drains the stream it was given, frees them and allocates larger ones;
the calls before and after must still be right, and so must a blocking call
that grows the arrays while a launch-only call's work is still on the stream.

Every call runs on a torch stream of its own, never the default one, so the
stream passed in is the one that gets drained.  Every expected value comes
from PyTorch (reference_verify, reference_copy_check, reference_diagnose on
reference_words data), never from another kernel.

The arrays belong to the process and only grow, so of two tests that grow one
array only the first to run walks the growth; the launch-only tests come
first, since only they grow an array with work in flight.  A use after free
would not fail deterministically: these tests show that the path works, the
single owner of the arrays (DeviceMirror) is what makes it sound."""
import functools
import random

import pytest
import torch

from test_nccl_p2p_amd.ops.buffers import (reference_copy_check, reference_diagnose, reference_verify,
                                           reference_words)

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
SEED = 0xD1A6C0DE
WRONG_SEED = SEED ^ 0x5A5A
SIZES = [0, 15, 16, 4096 + 5, 65536 + 1]   # verify jobs: empty, tail only, one vector, ragged, > one 32 KiB pass
OP_BYTES = 4096 + 7                        # checked copy ops: one chunk and a tail
GUARD = 256
SMALL = 64 << 10                           # 16 granules of 4 KiB
LARGE = (256 << 20) + 4096                 # 65537 granules of 4 KiB: one past kMaxDiagRecords
GRANULE = 4096


@pytest.fixture(scope="module", autouse=True)
def _gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)


@pytest.fixture()
def side():
    """A stream of its own, behind everything the default stream prepared."""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    yield s.cuda_stream
    s.synchronize()


def stream_fill(buf, seed):
    """Writes stream `seed` into the uint8 tensor buf from reference_words,
    32 MiB at a time."""
    step = 32 << 20
    for off in range(0, buf.numel(), step):
        n = min(step, buf.numel() - off)
        w = reference_words(off // 4, (n + 3) // 4, seed, device="cuda")
        b = torch.stack([(w >> (8 * k)) & 0xFF for k in range(4)], dim=1).to(torch.uint8).reshape(-1)
        buf[off:off + n] = b[:n]
    return buf


@functools.lru_cache(maxsize=None)
def clean(nbytes):
    """The first nbytes of stream SEED; shared and never written.  Carved out
    of a larger buffer so that an empty one still has an address."""
    return stream_fill(torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")[:nbytes], SEED)


# --------------------------------------------------------- batched verify ----

@functools.lru_cache(maxsize=None)
def verify_want(nbytes, seed):
    return tuple(reference_verify(clean(nbytes), seed))


def verify_jobs(n, draw):
    """n jobs with sizes drawn from SIZES, every seventh against the wrong
    seed: ([(ptr, bytes, seed)], [the reference's tuple])."""
    rng = random.Random(draw)
    jobs, want = [], []
    for i in range(n):
        nbytes = rng.choice(SIZES)
        seed = WRONG_SEED if i % 7 == 6 else SEED
        jobs.append((clean(nbytes).data_ptr(), nbytes, seed))
        want.append(verify_want(nbytes, seed))
    return jobs, want


def test_launch_then_blocking_verify_many(native, side):
    jobs, _ = verify_jobs(2, draw=1)
    native.verify_many_launch(jobs, side)
    jobs, want = verify_jobs(70, draw=2)
    assert [tuple(r) for r in native.verify_many(jobs, side)] == want


def test_verify_many_across_growth_and_batch_seams(native, side):
    # 70 jobs: launches of 32, 32 and 6, and more results than 1 job's array doubled.
    for n in (1, 70, 3):
        jobs, want = verify_jobs(n, draw=10 + n)
        assert n < 70 or {b for _, b, _ in jobs} == set(SIZES)
        assert [tuple(r) for r in native.verify_many(jobs, side)] == want


# --------------------------------------------------------- inline records ----

@functools.lru_cache(maxsize=None)
def op_source(flip_at):
    """An op's source: stream SEED, with one byte flipped at flip_at (None:
    clean), and what the reference finds in it."""
    src = clean(OP_BYTES)
    if flip_at is not None:
        src = src.clone()
        src[flip_at] ^= 0x24
    return src, tuple(reference_copy_check(src, SEED, 0))


def checked_ops(n):
    """n ops with a record each, every fifth with one flipped byte, into
    destinations between 0xAB guards: (ops, arena, the arena due, the records due)."""
    pitch = (OP_BYTES + 15) // 16 * 16 + GUARD
    arena = torch.full((GUARD + n * pitch,), 0xAB, dtype=torch.uint8, device="cuda")
    due = arena.clone()
    ops, want = [], []
    for i in range(n):
        src, rec = op_source((i * 131) % OP_BYTES if i % 5 == 4 else None)
        off = GUARD + i * pitch
        ops.append((arena.data_ptr() + off, src.data_ptr(), OP_BYTES, SEED, 0, i))
        due[off:off + OP_BYTES] = src
        want.append(rec)
    return ops, arena, due, want


def run_checked(native, n, stream):
    ops, arena, due, want = checked_ops(n)
    torch.cuda.synchronize()
    got = [tuple(r) for r in native.copy_checked(ops, stream)]
    assert got == want
    assert sum(m for m, _ in want) == n // 5
    assert torch.equal(arena, due), "a guard or a destination holds something else than what was loaded"


def test_launch_then_blocking_copy_checked(native, side):
    ops, arena, due, _ = checked_ops(1)
    torch.cuda.synchronize()
    native.copy_checked_launch(ops, side)
    run_checked(native, 130, side)
    assert torch.equal(arena, due)


def test_copy_checked_records_across_growth(native, side):
    for n in (1, 130, 2):
        run_checked(native, n, side)


# -------------------------------------------------------------- diagnosis ----

def plant(buf, offsets):
    """One wrong word at each byte offset: the first zeroed (poison), the
    others with three bits flipped."""
    for k, off in enumerate(offsets):
        word = buf[off:off + 4]
        if k == 0:
            word.zero_()
        else:
            word[1] ^= 0x07
    return buf


@pytest.fixture(scope="module")
def small():
    """(buffer, records due): 64 KiB with one wrong word, at the default granule."""
    buf = plant(clean(SMALL).clone(), [5 * GRANULE + 260])
    return buf, [tuple(r) for r in reference_diagnose(buf, SEED, granule=GRANULE)]


@pytest.fixture(scope="module")
def large():
    """(buffer, records due): 256 MiB + 4 KiB with one wrong word in each of
    its first, a middle and its last granule.  The reference runs over those
    three granules; the rest is the stream itself."""
    buf = stream_fill(torch.empty(LARGE, dtype=torch.uint8, device="cuda"), SEED)
    granules = [0, 40000, LARGE // GRANULE - 1]
    plant(buf, [g * GRANULE + 4 * (17 + g % 900) for g in granules])
    want = []
    for g in granules:
        want += reference_diagnose(buf[g * GRANULE:(g + 1) * GRANULE], SEED, granule=GRANULE, start=g * GRANULE)
    assert [r.index for r in want] == granules
    assert [(r.zero, r.other, r.flipped_bits) for r in want] == [(1, 0, 0), (0, 1, 3), (0, 1, 3)]
    return buf, [tuple(r) for r in want]


def diagnose(native, case, granule, stream, launch_only=False):
    buf, want = case
    fn = native.diagnose_launch if launch_only else native.diagnose
    got = fn(buf.data_ptr(), buf.numel(), SEED, [], granule, stream)
    if not launch_only:
        assert [tuple(r) for r in got] == want


def test_launch_then_blocking_diagnose(native, side, small, large):
    assert native.diagnose_granule(SMALL) == GRANULE
    diagnose(native, small, 0, side, launch_only=True)
    diagnose(native, large, GRANULE, side)


def test_diagnose_across_growth(native, side, small, large):
    diagnose(native, small, 0, side)
    diagnose(native, large, GRANULE, side)
    diagnose(native, small, 0, side)
