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


# ------------------------------------------------------- receive-and-reduce --

REDUCE_DTYPES = ("u32", "f32", "bf16")


def reduce_(dst: torch.Tensor, srcs, dtype: str, *, coherent: bool = False, max_blocks: int = 0,
            stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """``dst`` = ``srcs[0] + srcs[1] + ...`` in that order with the gfx950
    reduce kernel (stream-ordered): the tensors' bytes are read as elements of
    ``dtype`` ('u32', 'f32' or 'bf16'; csrc/reduce_op.hpp).  More than 8
    sources take further launches with ``dst`` as their operand 0."""
    nbytes = _check_tensor(dst)
    if any(_check_tensor(s) != nbytes for s in srcs):
        raise ValueError("reduce_: dst and every source have one size")
    require_native().reduce(dst.data_ptr(), [s.data_ptr() for s in srcs], nbytes, dtype, _stream(stream), coherent,
                            max_blocks)
    return dst


def reference_operands(nbytes: int, seed: int, dtype: str, device="cpu") -> torch.Tensor:
    """The first ``nbytes`` (a multiple of 4) of operand stream ``seed`` as
    int64 words in [0, 2**32): :func:`reference_words` through the operand map
    of ``dtype``, which pins every float's exponent field into [64, 127]."""
    assert nbytes % 4 == 0 and dtype in REDUCE_DTYPES
    w = reference_words(0, nbytes // 4, seed, device)
    if dtype == "f32":
        w = (w & 0xBFFFFFFF) | 0x20000000
    elif dtype == "bf16":
        w = (w & 0xBFFFBFFF) | 0x20002000
    return w


def _words_to_f32(w: torch.Tensor) -> torch.Tensor:
    return torch.where(w >= 2**31, w - 2**32, w).to(torch.int32).view(torch.float32)


def _f32_to_words(f: torch.Tensor) -> torch.Tensor:
    return f.contiguous().view(torch.int32).to(torch.int64) & M32


def reference_reduce(operands, dtype: str) -> torch.Tensor:
    """The sum of ``operands`` (int64 word tensors as :func:`reference_operands`
    gives them) in order, as int64 words: u32 wraps mod 2**32; f32 is a chain
    of ``torch.float32`` adds on the CPU; bf16 widens both halves of a word to
    float32, chains the adds and rounds once with ``.to(torch.bfloat16)``."""
    assert dtype in REDUCE_DTYPES and len(operands) >= 1
    ops = [o.cpu() for o in operands]
    if dtype == "u32":
        acc = ops[0].clone()
        for o in ops[1:]:
            acc = (acc + o) & M32
        return acc
    if dtype == "f32":
        acc = _words_to_f32(ops[0]).clone()
        for o in ops[1:]:
            acc = acc + _words_to_f32(o)
        return _f32_to_words(acc)
    lo = _words_to_f32((ops[0] << 16) & M32).clone()
    hi = _words_to_f32(ops[0] & 0xFFFF0000).clone()
    for o in ops[1:]:
        lo = lo + _words_to_f32((o << 16) & M32)
        hi = hi + _words_to_f32(o & 0xFFFF0000)
    lo16 = lo.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    hi16 = hi.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    return lo16 | (hi16 << 16)


def gated_reduce_(dst: torch.Tensor, srcs, gates: torch.Tensor, row_elems: int, *, coherent: bool = False,
                  max_blocks: int = 0, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The expert combine with the gfx950 gated reduce kernel (stream-ordered;
    ``--reduce-gate``): the tensors' bytes are rows of ``row_elems`` bf16 (a
    multiple of 512), and row r of ``dst`` = the sum over the 1..8 ``srcs`` k, in
    that order, of gate k of entry r of ``gates`` times row r of source k, in
    float32, rounded once.  ``gates``: 16 bytes (8 bf16) per row, local memory
    (csrc/reduce_gate_op.hpp)."""
    nbytes = _check_tensor(dst)
    if any(_check_tensor(s) != nbytes for s in srcs):
        raise ValueError("gated_reduce_: dst and every source have one size")
    if row_elems <= 0 or nbytes % (2 * row_elems) or _check_tensor(gates) < nbytes // (2 * row_elems) * 16:
        raise ValueError("gated_reduce_: whole rows of row_elems bf16 and 16 bytes of gates per row")
    require_native().gated_reduce(dst.data_ptr(), [s.data_ptr() for s in srcs], nbytes, gates.data_ptr(), row_elems,
                                  _stream(stream), coherent, max_blocks)
    return dst


def reference_gates(rows: int, seed: int, device="cpu") -> torch.Tensor:
    """The gate table of ``rows`` entries from stream ``seed`` as int64 words, 4
    per row (gate k of a row: half ``k & 1`` of its word ``k // 2``): each
    half-word h of the PRNG word becomes the positive bf16
    ``((123 + ((h >> 7) & 3)) << 7) | (h & 0x7F)``, a value in [2**-4, 1)."""
    w = reference_words(0, 4 * rows, seed, device)
    halves = [(((123 + ((h >> 7) & 3)) << 7) | (h & 0x7F)) for h in (w & 0xFFFF, w >> 16)]
    return halves[0] | (halves[1] << 16)


def reference_gated_reduce(operands, gates: torch.Tensor, row_elems: int) -> torch.Tensor:
    """What :func:`gated_reduce_` leaves, as int64 words: ``operands`` are int64
    bf16 word tensors (:func:`reference_operands`), ``gates`` the table's words
    (:func:`reference_gates`).  Plain PyTorch on the CPU: every bf16 widened to
    ``torch.float32``, gate k's multiply, sequential float32 adds in operand
    order, one ``.to(torch.bfloat16)``."""
    assert 1 <= len(operands) <= 8 and row_elems % 512 == 0
    row_words = row_elems // 2
    table = gates.cpu().reshape(-1, 4)
    lo = hi = None
    for k, o in enumerate(o.cpu() for o in operands):
        g16 = (table[:, k // 2] >> (16 * (k & 1))) & 0xFFFF
        g = _words_to_f32(g16 << 16).repeat_interleave(row_words)
        p_lo = g * _words_to_f32((o << 16) & M32)
        p_hi = g * _words_to_f32(o & 0xFFFF0000)
        lo = p_lo if lo is None else lo + p_lo
        hi = p_hi if hi is None else hi + p_hi
    lo16 = lo.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    hi16 = hi.to(torch.bfloat16).view(torch.int16).to(torch.int64) & 0xFFFF
    return lo16 | (hi16 << 16)


def words_to_bytes(w: torch.Tensor) -> torch.Tensor:
    """int64 words in [0, 2**32) as a uint8 tensor (little-endian)."""
    return torch.stack([(w >> (8 * k)) & 0xFF for k in range(4)], dim=1).to(torch.uint8).reshape(-1)


# ------------------------------------------------------ block-scaled wire ----

# Per format: stored mantissa bits, exponent of the smallest normal, the
# maximum as (significand, exponent), the sign's bit and a block's element bytes.
WIRE_FORMATS = {"mxfp8": dict(mbits=3, emin=-6, top=1.75, emax=8, sign=7, block_bytes=32),
                "mxfp6": dict(mbits=3, emin=0, top=1.875, emax=2, sign=5, block_bytes=24),
                "mxfp4": dict(mbits=1, emin=0, top=1.5, emax=2, sign=3, block_bytes=16)}
WIRE_TILE_BLOCKS = 128


def wire_pack_(dst: torch.Tensor, src: torch.Tensor, fmt: str, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The bytes of ``src`` read as bf16 (a multiple of 64 bytes) -> their
    'mxfp8' / 'mxfp6' / 'mxfp4' wire image in ``dst`` with the gfx950 pack kernel."""
    nbytes = _check_tensor(src)
    nat = require_native()
    if _check_tensor(dst) < nat.wire_bytes(nbytes, fmt):
        raise ValueError("wire_pack_: dst holds less than wire_bytes() of src")
    nat.wire_pack(dst.data_ptr(), src.data_ptr(), nbytes, fmt, _stream(stream))
    return dst


def wire_unpack_(dst: torch.Tensor, src: torch.Tensor, fmt: str, *, coherent: bool = False, max_blocks: int = 0,
                 lanes: str = "auto", stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """The wire image in ``src`` -> the bytes of ``dst`` as bf16 with the
    gfx950 unpack kernel (the IPC pull engine's receive under ``--wire``)."""
    nbytes = _check_tensor(dst)
    nat = require_native()
    if _check_tensor(src) < nat.wire_bytes(nbytes, fmt):
        raise ValueError("wire_unpack_: src holds less than wire_bytes() of dst")
    nat.wire_unpack(dst.data_ptr(), src.data_ptr(), nbytes, fmt, _stream(stream), coherent, max_blocks, lanes)
    return dst


def reference_wire_operands(nbytes: int, seed: int, device="cpu") -> torch.Tensor:
    """The first ``nbytes`` (a multiple of 64) of bf16 operand stream ``seed``
    as int64 words: sign and mantissa of both halves of the PRNG word, the
    exponent field 64 + (block & 31) + the low 4 bits of the half's own."""
    assert nbytes % 64 == 0
    w = reference_words(0, nbytes // 4, seed, device)
    block = (torch.arange(nbytes // 4, dtype=torch.int64, device=w.device) >> 4) & 31

    def half(h):
        return (h & 0x807F) | ((64 + block + ((h >> 7) & 15)) << 7)

    return half(w & 0xFFFF) | (half(w >> 16) << 16)


def _pow2(k: torch.Tensor) -> torch.Tensor:
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), k.to(torch.float64))


def _wire_quantize(words: torch.Tensor, fmt: str):
    """Per block of 32 elements, in float64 (amax, the division by the scale
    and the grid are exact there): the scale bytes [blocks], the element codes
    [blocks, 32] and the values they stand for, scale applied."""
    f = WIRE_FORMATS[fmt]
    words = words.cpu()
    h = torch.stack([words & 0xFFFF, words >> 16], dim=1).reshape(-1, 32)
    x = _words_to_f32((h << 16) & M32).to(torch.float64)
    amax = x.abs().amax(dim=1)
    m, ex = torch.frexp(amax)  # amax = 2m x 2^(ex - 1), 2m in [1, 2)
    e = ex.to(torch.int64) - 1 - f["emax"] + (2 * m > f["top"]).to(torch.int64)  # the no-clip rule
    sb = torch.where(amax == 0, torch.full_like(e, 127), (e + 127).clamp(1, 254))
    scale = _pow2(sb - 127)[:, None]
    q = x.abs() / scale
    qe = torch.frexp(q)[1].to(torch.int64) - 1
    step = _pow2(qe.clamp(min=f["emin"]) - f["mbits"])  # the grid's spacing at q, subnormals included
    r = torch.round(q / step) * step  # ties to even
    re = torch.frexp(r)[1].to(torch.int64) - 1
    normal = ((re - f["emin"] + 1) << f["mbits"]) + ((r / _pow2(re) - 1) * 2 ** f["mbits"]).to(torch.int64)
    code = torch.where(r >= 2.0 ** f["emin"], normal, (r * 2.0 ** (f["mbits"] - f["emin"])).to(torch.int64))
    neg = torch.signbit(x)
    value = r * scale
    return sb, code | (neg.to(torch.int64) << f["sign"]), torch.where(neg, -value, value)


def reference_wire_pack(words: torch.Tensor, fmt: str) -> torch.Tensor:
    """The wire image (uint8) of the bf16 payload ``words`` (int64 words, 16
    per block): per tile of up to 128 blocks the element bytes (element j in
    bits bj.. of its block, little-endian) and the scale bytes, each section
    followed by zeros up to a multiple of 16."""
    sb, code, _ = _wire_quantize(words, fmt)
    if fmt == "mxfp6":  # four 6-bit codes share three bytes
        v = code[:, 0::4] | (code[:, 1::4] << 6) | (code[:, 2::4] << 12) | (code[:, 3::4] << 18)
        elems = torch.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], dim=2).reshape(-1, 24)
    else:
        elems = code if fmt == "mxfp8" else code[:, 0::2] | (code[:, 1::2] << 4)
    parts = []
    for t in range(0, sb.numel(), WIRE_TILE_BLOCKS):
        for section in (elems[t:t + WIRE_TILE_BLOCKS].reshape(-1), sb[t:t + WIRE_TILE_BLOCKS]):
            parts += [section, torch.zeros(-section.numel() % 16, dtype=torch.int64)]
    return torch.cat(parts).to(torch.uint8)


def reference_wire_roundtrip(words: torch.Tensor, fmt: str) -> torch.Tensor:
    """What the receiver holds (uint8, bf16 payload bytes): every element
    quantised under its block's scale and widened again, exactly."""
    value = _wire_quantize(words, fmt)[2].to(torch.float32).reshape(-1)
    bits = (value.view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    return torch.stack([bits & 0xFF, bits >> 8], dim=1).to(torch.uint8).reshape(-1)


def wire_reduce_(dst: torch.Tensor, srcs, fmt: str, *, coherent=False, max_blocks: int = 0,
                 lanes: str = "auto", stream: Optional[torch.cuda.Stream] = None, own_bf16: bool = False) -> torch.Tensor:
    """The bytes of ``dst`` as bf16 = the sum of the 1..8 'mxfp8' / 'mxfp6' /
    'mxfp4' wire images ``srcs`` in that order, dequantised and added in float32
    and rounded once, with the gfx950 wire-reduce kernel (the IPC pull engine's
    receive under ``--reduce-wire``; stream-ordered).  ``coherent``: True reads
    every image in the cross-GPU form, an int is a mask, bit k for source k.
    ``own_bf16``: ``srcs[0]`` is the receiver's own shard, the payload's bytes
    of bf16 in local memory, and enters the sum unquantised (``--reduce-own
    bf16``); bit 0 of the mask must be clear."""
    nbytes = _check_tensor(dst)
    nat = require_native()
    if any(_check_tensor(s) < (nbytes if own_bf16 and k == 0 else nat.wire_bytes(nbytes, fmt)) for k, s in enumerate(srcs)):
        raise ValueError("wire_reduce_: a source holds less than wire_bytes() of dst (own_bf16: the first less than dst)")
    nat.wire_reduce(dst.data_ptr(), [s.data_ptr() for s in srcs], nbytes, fmt, _stream(stream), coherent, max_blocks, lanes,
                    own_bf16)
    return dst


def reference_wire_reduce(operands, fmt: str, own_bf16: bool = False) -> torch.Tensor:
    """What :func:`wire_reduce_` leaves (uint8, bf16 payload bytes) for the
    images of ``operands`` (int64 bf16 word tensors, in order):
    :func:`reference_wire_roundtrip` of each (float64 quantisation) fed to
    :func:`reference_reduce` as bf16 (a ``torch.float32`` add chain on the CPU
    and one ``.to(torch.bfloat16)``).  ``own_bf16``: ``operands[0]`` is the
    own shard and enters unquantised."""
    widened = []
    for k, w in enumerate(operands):
        if own_bf16 and k == 0:
            widened.append(w.cpu())
            continue
        b = reference_wire_roundtrip(w, fmt).to(torch.int64).reshape(-1, 4)
        widened.append(b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24))
    return words_to_bytes(reference_reduce(widened, "bf16"))


def wire_reduce_packed_(dst: torch.Tensor, srcs, nbytes: int, fmt: str, *, coherent=False, max_blocks: int = 0,
                        lanes: str = "auto", stream: Optional[torch.cuda.Stream] = None, own_bf16: bool = False,
                        both: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``dst`` = the wire image (``wire_bytes(nbytes, fmt)`` bytes) of the bf16
    sum :func:`wire_reduce_` gives for the 1..8 'mxfp8' / 'mxfp6' / 'mxfp4' wire
    images ``srcs`` of ``nbytes`` of payload each, with the gfx950
    wire-reduce-pack kernel in one launch (the IPC pull engine's receive under
    ``--reduce-out wire``).  ``coherent`` and ``own_bf16`` as in
    :func:`wire_reduce_`.  ``both``: ``nbytes`` of bf16 that receive, in the same
    launch, what that image widens to (``--reduce-out both``)."""
    nat = require_native()
    image = nat.wire_bytes(nbytes, fmt)
    if _check_tensor(dst) < image or any(_check_tensor(s) < (nbytes if own_bf16 and k == 0 else image) for k, s in enumerate(srcs)):
        raise ValueError("wire_reduce_packed_: dst or a source holds less than wire_bytes() of the payload")
    if both is not None and _check_tensor(both) < nbytes:
        raise ValueError("wire_reduce_packed_: both holds less than the payload")
    nat.wire_reduce_packed(dst.data_ptr(), [s.data_ptr() for s in srcs], nbytes, fmt, _stream(stream), coherent, max_blocks, lanes,
                           own_bf16, both.data_ptr() if both is not None else 0)
    return dst


def reference_wire_reduce_packed(operands, fmt: str, own_bf16: bool = False) -> torch.Tensor:
    """What :func:`wire_reduce_packed_` leaves (uint8, the whole image):
    :func:`reference_wire_pack` of the :func:`reference_wire_reduce` result."""
    b = reference_wire_reduce(operands, fmt, own_bf16).to(torch.int64).reshape(-1, 4)
    return reference_wire_pack(b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24), fmt)


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
