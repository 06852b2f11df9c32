"""Payload fill / verification on device tensors.

Device side: the hand-written gfx950 kernels in ``csrc/kernels.hip`` (fill:
16 B/lane stores; verify: register- or LDS-DMA-staged loads with a fused
wave64-shuffle -> LDS -> one-atomic-per-block reduction).  Host side: a plain
PyTorch implementation of the same counter-based PRNG (``csrc/prng.hpp``) so
the kernels can be checked word for word.

The reference benchmark zero-fills its buffers and never reads them back
(/root/reference/p2p_matrix.cc:129-130); this is what replaces that.
"""

from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from .._native import require_native

M32 = 0xFFFFFFFF


def impl_number(name: str) -> int:
    """Verify kernel name -> the native impl number: auto, lds8 (alias lds),
    stride (alias reg); a variant round 5 removed raises ValueError saying so
    (csrc/app.cpp parse_verify_impl, shared with p2p_matrix --verify-impl)."""
    return require_native().parse_verify_impl(name)


class VerifyResult(NamedTuple):
    mismatches: int   # mismatching 32-bit words (tail: partial word counts once)
    checksum: int     # sum of received 32-bit words mod 2**64
    first_bad: int    # lowest mismatching byte offset, 2**64-1 if none

    @property
    def ok(self) -> bool:
        return self.mismatches == 0


def _check_tensor(t: torch.Tensor) -> int:
    if not t.is_cuda:
        raise ValueError("device kernels need a GPU tensor")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    if t.data_ptr() % 16:
        raise ValueError("tensor data must be 16-byte aligned (gfx950 dwordx4 accesses)")
    return t.numel() * t.element_size()


def _stream(stream: Optional[torch.cuda.Stream]) -> int:
    s = stream if stream is not None else torch.cuda.current_stream()
    return int(s.cuda_stream)


def fill_(t: torch.Tensor, seed: int, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Fills the bytes of ``t`` with PRNG stream ``seed`` (stream-ordered)."""
    nbytes = _check_tensor(t)
    require_native().fill(t.data_ptr(), nbytes, seed & (2**64 - 1), _stream(stream))
    return t


def verify(t: torch.Tensor, seed: int, impl: str = "auto", stream: Optional[torch.cuda.Stream] = None, *,
           max_grid: int = 0, lds_stages: int = 0) -> VerifyResult:
    """Compares ``t`` with PRNG stream ``seed`` on the device (blocking).
    ``max_grid`` > 0 caps the workgroup count and ``lds_stages`` 4 or 8 forces
    that LDS-staged kernel (0, 0: the production launch)."""
    nbytes = _check_tensor(t)
    r = require_native().verify(t.data_ptr(), nbytes, seed & (2**64 - 1), impl_number(impl), True, _stream(stream),
                                max_grid=max_grid, lds_stages=lds_stages)
    return VerifyResult(*r)


def checksum(t: torch.Tensor, impl: str = "auto", stream: Optional[torch.cuda.Stream] = None, *,
             max_grid: int = 0, lds_stages: int = 0) -> int:
    """Sum of the tensor's 32-bit words mod 2**64 (no PRNG compare);
    ``max_grid`` and ``lds_stages`` as in :func:`verify`."""
    nbytes = _check_tensor(t)
    return int(require_native().verify(t.data_ptr(), nbytes, 0, impl_number(impl), False, _stream(stream),
                                       max_grid=max_grid, lds_stages=lds_stages)[1])


# ---------------------------------------------------------------- reference --

def _fmix32(h: torch.Tensor) -> torch.Tensor:
    # int64 arithmetic; products wrap mod 2**64 and are masked back to 32 bits.
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _fmix32_int(h: int) -> int:
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def reference_words(start: int, count: int, seed: int, device="cpu") -> torch.Tensor:
    """Words [start, start+count) of the stream as int64 values in [0, 2**32)."""
    seed &= 2**64 - 1
    idx = torch.arange(start, start + count, dtype=torch.int64, device=device)
    hi = idx >> 32
    lo = idx & M32
    seed_lo = seed & M32
    seed_hi = seed >> 32
    inner = _fmix32((seed_hi + hi * 0x27D4EB2F + 0x165667B1) & M32)
    key = _fmix32(seed_lo ^ inner)
    return _fmix32(((lo * 0x9E3779B1) & M32) ^ key)


def reference_bytes(nbytes: int, seed: int, device="cpu") -> torch.Tensor:
    """The first ``nbytes`` of the stream as a uint8 tensor (little-endian words)."""
    nwords = (nbytes + 3) // 4
    w = reference_words(0, nwords, seed, device)
    b = torch.stack([(w >> (8 * k)) & 0xFF for k in range(4)], dim=1).to(torch.uint8).reshape(-1)
    return b[:nbytes]


def reference_verify(data: torch.Tensor, seed: int) -> VerifyResult:
    """PyTorch implementation of the verify kernel's contract on a uint8 tensor."""
    data = data.reshape(-1).to(torch.uint8)
    nbytes = data.numel()
    nwords = (nbytes + 3) // 4
    pad = nwords * 4 - nbytes
    d = torch.cat([data, torch.zeros(pad, dtype=torch.uint8, device=data.device)]).to(torch.int64).reshape(nwords, 4)
    got = d[:, 0] | (d[:, 1] << 8) | (d[:, 2] << 16) | (d[:, 3] << 24)
    want = reference_words(0, nwords, seed, data.device)
    if pad:
        mask = (1 << (8 * (4 - pad))) - 1
        want = want.clone()
        want[-1] &= mask
        got_cmp = got.clone()
        got_cmp[-1] &= mask
    else:
        got_cmp = got
    bad = (got_cmp != want).nonzero().reshape(-1)
    csum = int(got.sum().item()) % 2**64
    first = int(bad[0].item()) * 4 if bad.numel() else 2**64 - 1
    return VerifyResult(int(bad.numel()), csum, first)


# ------------------------------------------------------------- checked copy --

class CopyCheck(NamedTuple):
    """What the checked copy found in one op (csrc/kernels.hpp CopyCheck)."""
    mismatches: int   # mismatching 32-bit words (tail: partial word counts once)
    first_bad: int    # lowest mismatching stream byte (stream_offset + position), 2**64-1 if none

    @property
    def ok(self) -> bool:
        return self.mismatches == 0


def copy_checked_(dst: torch.Tensor, src: torch.Tensor, seed: int, *, stream_offset: int = 0, coherent: bool = False,
                  max_blocks: int = 0, stream: Optional[torch.cuda.Stream] = None) -> CopyCheck:
    """Copies ``src`` into ``dst`` with the gfx950 checked copy kernel, which
    compares every word it loads with bytes ``[stream_offset, stream_offset +
    nbytes)`` of PRNG stream ``seed`` on its way through (blocking).  ``dst``
    receives what was loaded whether or not it matched.  ``stream_offset`` is
    a multiple of 4096; ``coherent`` selects the cross-GPU access form."""
    nbytes = _check_tensor(src)
    if _check_tensor(dst) != nbytes:
        raise ValueError("copy_checked_: dst and src differ in size")
    r = require_native().copy_checked([(dst.data_ptr(), src.data_ptr(), nbytes, seed & (2**64 - 1), stream_offset, 0)],
                                      _stream(stream), coherent, max_blocks)
    return CopyCheck(*r[0])


def reference_copy_check(src: torch.Tensor, seed: int, stream_offset: int = 0) -> CopyCheck:
    """PyTorch implementation of the checked copy's contract on a uint8
    tensor holding stream bytes from ``stream_offset`` (a multiple of 4) on:
    wrong 32-bit words, the final partial word masked, and the first wrong
    stream byte.  Built on :func:`reference_words`."""
    assert stream_offset % 4 == 0
    data = src.reshape(-1).to(torch.uint8)
    nbytes = data.numel()
    nwords = (nbytes + 3) // 4
    if not nwords:
        return CopyCheck(0, 2**64 - 1)
    pad = nwords * 4 - nbytes
    d = torch.cat([data, torch.zeros(pad, dtype=torch.uint8, device=data.device)]).to(torch.int64).reshape(nwords, 4)
    mask = torch.full((nwords,), M32, dtype=torch.int64, device=data.device)
    if pad:
        mask[-1] = (1 << (8 * (4 - pad))) - 1
    got = (d[:, 0] | (d[:, 1] << 8) | (d[:, 2] << 16) | (d[:, 3] << 24)) & mask
    want = reference_words(stream_offset // 4, nwords, seed, data.device) & mask
    bad = (got != want).nonzero().reshape(-1)
    first = stream_offset + int(bad[0].item()) * 4 if bad.numel() else 2**64 - 1
    return CopyCheck(int(bad.numel()), first)


# ---------------------------------------------------------------- diagnosis --

class GranuleRecord(NamedTuple):
    """One damaged granule (csrc/diagnose.hpp DiagRecord)."""
    index: int         # granule number: bytes [index * granule, (index + 1) * granule)
    first_bad: int     # byte offset of its first damaged word
    last_bad: int      # byte offset of its last damaged word
    zero: int          # words still poison
    other: int         # words that match nothing
    flipped_bits: int  # popcount(got ^ expected) over the `other` words
    cand0: int = 0     # words that match candidate k
    cand1: int = 0
    cand2: int = 0
    cand3: int = 0
    cand4: int = 0
    cand5: int = 0


class Extent(NamedTuple):
    """A maximal run of consecutive damaged granules with the same classes."""
    begin: int         # byte offset of its first damaged word
    end: int           # byte offset after its last damaged word (clipped to the buffer)
    zero: int
    other: int
    flipped_bits: int
    cand0: int = 0
    cand1: int = 0
    cand2: int = 0
    cand3: int = 0
    cand4: int = 0
    cand5: int = 0


def _candidates(candidates):
    out = []
    for c in candidates:
        c = tuple(c)
        out.append((int(c[0]) & (2**64 - 1), int(c[1])) + tuple(int(x) for x in c[2:]))
    return out


def diagnose_records(t: torch.Tensor, seed: int, candidates=(), granule: int = 0,
                     stream: Optional[torch.cuda.Stream] = None, *, max_grid: int = 0):
    """The gfx950 diagnosis kernel on ``t`` (blocking): its damaged granules
    as :class:`GranuleRecord`.  ``candidates``: up to 6 ``(seed, shift)`` with
    ``shift`` a signed byte count, a multiple of 16."""
    nbytes = _check_tensor(t)
    recs = require_native().diagnose(t.data_ptr(), nbytes, seed & (2**64 - 1), _candidates(candidates), granule,
                                     _stream(stream), max_grid)
    return [GranuleRecord(*r) for r in recs]


def diagnose(t: torch.Tensor, seed: int, candidates=(), granule: int = 0,
             stream: Optional[torch.cuda.Stream] = None, *, max_grid: int = 0):
    """Where ``t`` differs from PRNG stream ``seed`` and what the wrong words
    hold instead, as :class:`Extent` (``_p2pcore.describe_extent`` gives the
    text of one)."""
    nbytes = _check_tensor(t)
    recs = diagnose_records(t, seed, candidates, granule, stream, max_grid=max_grid)
    return [Extent(*e) for e in require_native().merge_extents([tuple(r) for r in recs], nbytes, granule)]


def _popcount32(x: torch.Tensor) -> torch.Tensor:
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    return ((x * 0x01010101) & M32) >> 24


def reference_diagnose(data: torch.Tensor, seed: int, candidates=(), granule: int = 4096, start: int = 0):
    """PyTorch implementation of the diagnosis contract (csrc/diagnose.hpp) on
    a uint8 tensor, on top of :func:`reference_words`: the damaged granules as
    :class:`GranuleRecord`.  ``data`` may be the slice of a larger buffer that
    begins ``start`` bytes into it (a multiple of ``granule``) and runs to
    its end; indices and offsets are then those of the whole buffer."""
    assert granule >= 4096 and granule & (granule - 1) == 0 and start % granule == 0
    data = data.reshape(-1).to(torch.uint8)
    dev = data.device
    nbytes = data.numel()
    nwords = (nbytes + 3) // 4
    if not nwords:
        return []
    pad = nwords * 4 - nbytes
    d = torch.cat([data, torch.zeros(pad, dtype=torch.uint8, device=dev)]).to(torch.int64).reshape(nwords, 4)
    mask = torch.full((nwords,), M32, dtype=torch.int64, device=dev)
    if pad:
        mask[-1] = (1 << (8 * (4 - pad))) - 1
    got = (d[:, 0] | (d[:, 1] << 8) | (d[:, 2] << 16) | (d[:, 3] << 24)) & mask
    w0 = start // 4
    want = reference_words(w0, nwords, seed, dev) & mask
    bad = got != want
    zero = bad & (got == 0)
    left = bad & ~zero                      # wrong, not poison, no candidate matched yet
    classes = [zero]
    cands = _candidates(candidates)
    assert len(cands) <= 6
    for cseed, shift, *_ in cands:
        assert shift % 16 == 0
        first = w0 + shift // 4             # stream index the slice's word 0 is compared with
        skip = min(max(-first, 0), nwords)  # words whose shifted index is negative
        cw = torch.zeros(nwords, dtype=torch.int64, device=dev)
        if skip < nwords:
            cw[skip:] = reference_words(first + skip, nwords - skip, cseed, dev)
        valid = torch.arange(nwords, device=dev) >= skip
        hit = left & valid & (got == (cw & mask))
        classes.append(hit)
        left = left & ~hit
    classes += [torch.zeros_like(bad)] * (6 - len(cands))
    flipped = torch.where(left, _popcount32(got ^ want), torch.zeros_like(got))
    offs = start + 4 * torch.arange(nwords, dtype=torch.int64, device=dev)
    gran = (offs - start) // granule
    ngran = int(gran[-1].item()) + 1

    def per_granule(x):
        return torch.zeros(ngran, dtype=torch.int64, device=dev).index_add_(0, gran, x.to(torch.int64))

    sums = [per_granule(c) for c in classes] + [per_granule(left), per_granule(flipped)]
    big = torch.iinfo(torch.int64).max
    first_bad = torch.full((ngran,), big, dtype=torch.int64, device=dev).scatter_reduce_(
        0, gran[bad], offs[bad], "amin")
    last_bad = torch.full((ngran,), -1, dtype=torch.int64, device=dev).scatter_reduce_(
        0, gran[bad], offs[bad], "amax")
    rows = torch.stack(sums + [first_bad, last_bad], dim=1).cpu().tolist()  # one transfer
    out = []
    for g, c in enumerate(rows):
        if c[10] >= 0:
            out.append(GranuleRecord(start // granule + g, c[9], c[10], c[0], c[7], c[8], *c[1:7]))
    return out


def payload_seed(src: int, nbytes: int, salt: int = 0) -> int:
    """Seed of the payload rank ``src`` sends (csrc/prng.hpp payload_seed)."""
    s = 0x9E3779B97F4A7C15 ^ ((src & M32) << 40) ^ nbytes ^ ((salt * 0xD6E8FEB86659FD93) & (2**64 - 1))
    s &= 2**64 - 1
    return s ^ (s >> 29)
