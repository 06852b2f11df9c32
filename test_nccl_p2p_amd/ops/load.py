"""The background-load kernels (``--load``) on torch tensors, and the plain-PyTorch
references they are tested against.

``load_mfma_`` / ``load_hbm_`` launch the gfx950 kernels of csrc/load.hip;
``reference_mfma_tiles`` rebuilds every wave's A and B from the PRNG stream,
multiplies them on the CPU and lays the product out as the kernel stores it;
``reference_hbm_sum`` is the word sum the streaming kernel's workgroups add up to.
"""

from __future__ import annotations

from typing import Optional

import torch

from .._native import require_native
from .buffers import _check_tensor, _stream, reference_words

WAVES = 4            # per workgroup (256 threads)
TILE = 32 * 32       # floats a wave stores


def operand_values(words: torch.Tensor) -> torch.Tensor:
    """PRNG words -> operand elements ((w % 31) - 15) / 8: multiples of 1/8 in
    [-15/8, 15/8], exact in bf16, with products and 16-term sums exact in f32."""
    return ((words % 31) - 15).to(torch.float32) / 8.0


def reference_operands(wgs: int, seed: int):
    """A [waves, 32, 16] and B [waves, 16, 32] of every wave (wave g = workgroup * 4
    + wave): words [g * 1024, +512) of stream ``seed`` are A row-major, the next
    512 are B row-major."""
    n = wgs * WAVES
    v = operand_values(reference_words(0, n * 1024, seed)).reshape(n, 1024)
    return v[:, :512].reshape(n, 32, 16), v[:, 512:].reshape(n, 16, 32)


def reference_mfma_tiles(wgs: int, seed: int) -> torch.Tensor:
    """What ``load_mfma_`` stores for any ``reps``: [wgs * 4, 64 lanes, 16 regs] f32,
    each wave's A @ B in the C/D register layout of v_mfma_f32_32x32x16_bf16.

    The kernel's lane l fills element j of its fragments from A[l & 31][8 (l >> 5) + j]
    and B[8 (l >> 5) + j][l & 31] (the operand lane maps), so with those maps right the
    wave computes the plain product of the two row-major matrices; the result is read
    back through the C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) +
    4 (lane >> 5).  A wrong map on either side shows as a mismatch (A and B are random,
    so the product is not symmetric)."""
    a, b = reference_operands(wgs, seed)
    lane = torch.arange(64)
    c = a.double() @ b.double()                                # exact: multiples of 1/64, sums below 2**6
    reg = torch.arange(16)
    row = (reg[None, :] & 3) + 8 * (reg[None, :] >> 2) + 4 * (lane[:, None] >> 5)   # [64, 16]
    col = (lane & 31)[:, None].expand(64, 16)
    return c[:, row, col].to(torch.float32)


def reference_hbm_sum(data: torch.Tensor, passes: int) -> int:
    """``passes`` x the sum of the buffer's 32-bit words, mod 2**64."""
    w = data.detach().cpu().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (passes * int(w.sum().item())) % (1 << 64)


def load_mfma_(out: torch.Tensor, wgs: int, reps: int, seed: int, stream: Optional[torch.cuda.Stream] = None, *,
               cancel_ptr: int = 0, done_ptr: int = 0, tickets_ptr: int = 0, ordinal: int = 0) -> torch.Tensor:
    """Launches the matrix-core load (stream-ordered); ``out`` holds wgs * 4096 floats."""
    nbytes = _check_tensor(out)
    if out.dtype != torch.float32 or nbytes < wgs * WAVES * TILE * 4:
        raise ValueError("out must be float32 with at least wgs * 4096 elements")
    require_native().load_mfma(wgs, reps, seed & (2**64 - 1), out.data_ptr(), _stream(stream), cancel_ptr=cancel_ptr,
                               done_ptr=done_ptr, tickets_ptr=tickets_ptr, ordinal=ordinal)
    return out


def load_hbm_(data: torch.Tensor, passes: int, wgs: int, out: torch.Tensor,
              stream: Optional[torch.cuda.Stream] = None, *, cancel_ptr: int = 0, done_ptr: int = 0,
              tickets_ptr: int = 0, ordinal: int = 0) -> torch.Tensor:
    """Launches the HBM-streaming load over ``data`` (a multiple of 4 KiB); ``out`` holds
    ``wgs`` int64 sums."""
    nbytes = _check_tensor(data)
    if out.dtype != torch.int64 or _check_tensor(out) < wgs * 8:
        raise ValueError("out must be int64 with at least wgs elements")
    require_native().load_hbm(data.data_ptr(), nbytes, passes, wgs, out.data_ptr(), _stream(stream),
                              cancel_ptr=cancel_ptr, done_ptr=done_ptr, tickets_ptr=tickets_ptr, ordinal=ordinal)
    return out
