"""The background-load kernels (csrc/load.hip) directly, on one MI355X.

Matrix-core load: every wave's stored tile is exactly the CPU product of the
operands rebuilt from the PRNG stream, whatever `reps` -- a wrong lane map, a
wave storing into another wave's tile or an unbalanced +A.B / -A.B pair shows
here.  HBM load: the workgroups' sums add up to passes x the buffer's word
sum.  Both: a cancel word set before the launch leaves `out` alone and `done`
where it was, and a row of launches counts `done` up and leaves the ticket
counter at 0."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import fill_
from test_nccl_p2p_amd.ops.load import load_hbm_, load_mfma_, reference_hbm_sum, reference_mfma_tiles

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes of 0xAB on either side of `out`
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def tiles(wgs, seed):
    return reference_mfma_tiles(wgs, seed)


def guarded(nbytes):
    """A 0xAB-filled byte buffer and the `nbytes` in its middle."""
    buf = torch.full((GUARD + nbytes + GUARD,), 0xAB, dtype=torch.uint8, device=DEV)
    return buf, buf[GUARD:GUARD + nbytes]


def guards_intact(buf):
    return bool((buf[:GUARD] == 0xAB).all()) and bool((buf[-GUARD:] == 0xAB).all())


class Ctl:
    """cancel and done in pinned host memory, the ticket counter on the device."""

    def __init__(self, native):
        self.words = native.HostWords(2)
        self.tickets = torch.zeros(1, dtype=torch.int64, device=DEV)

    def args(self, ordinal=0):
        return dict(cancel_ptr=self.words.ptr(0), done_ptr=self.words.ptr(1), tickets_ptr=self.tickets.data_ptr(),
                    ordinal=ordinal)

    def cancel(self, on):
        self.words.store(0, 1 if on else 0)

    @property
    def done(self):
        return self.words.load(1)


# reps 0, 1, 7: the final product alone, one pair, the remainder loop; 8 and 19: the 8-pair trips, then a remainder.
@pytest.mark.parametrize("wgs", [1, 3])
@pytest.mark.parametrize("reps", [0, 1, 7, 8, 19])
def test_mfma_tiles_are_exactly_a_times_b(native, wgs, reps):
    buf, mid = guarded(wgs * 4096 * 4)
    out = mid.view(torch.float32)
    load_mfma_(out, wgs, reps, 1234)
    torch.cuda.synchronize()
    got = out.cpu().reshape(wgs * 4, 64, 16)
    want = tiles(wgs, 1234)
    assert got.shape == want.shape
    bad = (got != want).nonzero()
    assert bad.numel() == 0, "first wrong (wave, lane, reg): %s of %d" % (bad[0].tolist(), len(bad))
    assert guards_intact(buf)


def test_mfma_seeds_give_different_tiles(native):
    _, mid = guarded(4096 * 4)
    out = mid.view(torch.float32)
    seen = []
    for seed in (1, 2, 2**40 + 1):
        load_mfma_(out, 1, 2, seed)
        torch.cuda.synchronize()
        seen.append(out.cpu().clone())
        assert torch.equal(seen[-1].reshape(4, 64, 16), tiles(1, seed))
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    # The waves of one workgroup are keyed apart too.
    assert not torch.equal(seen[0][:1024], seen[0][1024:2048])


@pytest.mark.parametrize("kind", ["mfma", "hbm"])
def test_cancel_before_the_launch_leaves_out_and_done_alone(native, kind):
    ctl = Ctl(native)
    wgs = 3
    buf, mid = guarded(wgs * 4096 * 4)
    data = fill_(torch.empty(1 << 16, dtype=torch.uint8, device=DEV), 9)
    ctl.cancel(True)
    for ordinal in range(2):
        if kind == "mfma":
            load_mfma_(mid.view(torch.float32), wgs, 3, 7, **ctl.args(ordinal))
        else:
            load_hbm_(data, 2, wgs, mid.view(torch.int64), **ctl.args(ordinal))
    torch.cuda.synchronize()
    assert bool((buf == 0xAB).all()), "a cancelled workgroup wrote to out"
    assert ctl.done == 0
    assert int(ctl.tickets.item()) == 0, "cancelled workgroups still take their tickets"
    # The same launch after the cancel is lifted runs and is counted.
    ctl.cancel(False)
    if kind == "mfma":
        load_mfma_(mid.view(torch.float32), wgs, 3, 7, **ctl.args(2))
    else:
        load_hbm_(data, 2, wgs, mid.view(torch.int64), **ctl.args(2))
    torch.cuda.synchronize()
    assert ctl.done == 3 and int(ctl.tickets.item()) == 0
    assert not bool((mid == 0xAB).all()) and guards_intact(buf)


def test_five_launches_in_a_row(native):
    ctl = Ctl(native)
    _, mid = guarded(5 * 4096 * 4)
    out = mid.view(torch.float32)
    for ordinal in range(5):
        load_mfma_(out, 5, 4, 3, **ctl.args(ordinal))
    torch.cuda.synchronize()
    assert ctl.done == 5
    assert int(ctl.tickets.item()) == 0
    assert torch.equal(out.cpu().reshape(20, 64, 16), tiles(5, 3))


def test_done_needs_a_ticket_counter(native):
    ctl = Ctl(native)
    _, mid = guarded(4096 * 4)
    with pytest.raises(ValueError, match="tickets_ptr"):
        native.load_mfma(1, 1, 1, mid.data_ptr(), 0, done_ptr=ctl.words.ptr(1))
    with pytest.raises(ValueError, match="wgs"):
        native.load_mfma(0, 1, 1, mid.data_ptr(), 0)
    with pytest.raises(ValueError, match="4096"):
        native.load_hbm(mid.data_ptr(), 4096 + 16, 1, 1, mid.data_ptr(), 0)


@functools.lru_cache(maxsize=None)
def hbm_buffer(nbytes):
    data = fill_(torch.empty(nbytes, dtype=torch.uint8, device=DEV), 0x5EED + nbytes)
    torch.cuda.synchronize()
    return data, reference_hbm_sum(data, 1)


# 4 KiB: one workgroup's single partial tile; 4 KiB x 257: an odd count of 4 KiB
# blocks, a partial last tile; 1 MiB: several grid-stride trips per workgroup.
@pytest.mark.parametrize("nbytes", [4096, 4096 * 257, 1 << 20])
@pytest.mark.parametrize("passes", [1, 3])
@pytest.mark.parametrize("wgs", [1, 5])
def test_hbm_sums_add_up(native, nbytes, passes, wgs):
    data, once = hbm_buffer(nbytes)
    buf, mid = guarded(wgs * 8)
    out = mid.view(torch.int64)
    load_hbm_(data, passes, wgs, out)
    torch.cuda.synchronize()
    total = sum(int(v) & (2**64 - 1) for v in out.cpu().tolist()) % 2**64
    assert total == (passes * once) % 2**64
    assert guards_intact(buf)
