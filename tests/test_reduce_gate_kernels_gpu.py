"""The gfx950 gated reduce kernels on one GPU: bit-exact against the
plain-PyTorch reference, on operands and gates from the fills, between guards."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (gated_reduce_, reference_gated_reduce, reference_gates, reference_operands,
                                   words_to_bytes)

pytestmark = pytest.mark.gpu

ROWS = [1, 3, 4, 5, 13]  # H = 512: part of a block, block - 1 row, a block, block + 1 row; H = 1536: rows straddle blocks
GUARD = 256
GATE_SEED = 4242


@functools.lru_cache(maxsize=None)
def _ref_operand(nbytes, seed):
    return reference_operands(nbytes, seed, "bf16")


@functools.lru_cache(maxsize=None)
def _ref_sum(rows, h, k):
    ops = [_ref_operand(rows * 2 * h, 900 + i) for i in range(k)]
    return words_to_bytes(reference_gated_reduce(ops, reference_gates(rows, GATE_SEED), h))


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _guarded(nbytes):
    """A 0xAB-filled buffer and its 16-byte aligned payload view of nbytes."""
    whole = torch.full((2 * GUARD + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + nbytes:] == 0xAB).all())


def _inputs(native, rows, h, k):
    """k operand buffers and the gate table, from the device fills."""
    nbytes = rows * 2 * h
    srcs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(k)]
    for i, s in enumerate(srcs):
        native.fill_operand(s.data_ptr(), nbytes, 900 + i, "bf16", _stream())
    gates = torch.empty(16 * rows, dtype=torch.uint8, device="cuda")
    native.fill_gate(gates.data_ptr(), rows, GATE_SEED, _stream())
    return srcs, gates


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("h", [512, 1536])
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_gated_reduce_matches_reference(native, k, h, coherent):
    for rows in ROWS:
        nbytes = rows * 2 * h
        whole, dst = _guarded(nbytes)
        srcs, gates = _inputs(native, rows, h, k)
        gated_reduce_(dst, srcs, gates, h, coherent=coherent)
        assert torch.equal(dst.cpu(), _ref_sum(rows, h, k)), rows
        assert _guards_intact(whole, nbytes), rows


@pytest.mark.parametrize("rows,h,max_blocks", [(1025, 512, 0), (342, 1536, 2)], ids=["1MiB+row", "grid-stride"])
def test_gated_reduce_large_and_grid_stride(native, rows, h, max_blocks):
    nbytes = rows * 2 * h
    whole, dst = _guarded(nbytes)
    srcs, gates = _inputs(native, rows, h, 3)
    assert torch.equal(gates.cpu(), words_to_bytes(reference_gates(rows, GATE_SEED)))
    gated_reduce_(dst, srcs, gates, h, max_blocks=max_blocks)
    assert torch.equal(dst.cpu(), _ref_sum(rows, h, 3)) and _guards_intact(whole, nbytes)


def test_gated_reduce_many_one_launch(native):
    h, rows = 1536, [5, 13, 1]  # unequal sizes: the binary search for the op
    bufs = [_guarded(r * 2 * h) for r in rows]
    ins = [_inputs(native, r, h, 2) for r in rows]
    native.gated_reduce_many([(d.data_ptr(), [s.data_ptr() for s in ss], r * 2 * h, g.data_ptr())
                              for (_, d), (ss, g), r in zip(bufs, ins, rows)], h, _stream())
    for (whole, d), r in zip(bufs, rows):
        assert torch.equal(d.cpu(), _ref_sum(r, h, 2)) and _guards_intact(whole, r * 2 * h), r


def test_verify_gated_reduced_finds_a_flipped_bit_and_a_wrong_table(native):
    rows, h, k = 5, 1536, 3
    nbytes, seeds = rows * 2 * h, [900, 901, 902]
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    srcs, gates = _inputs(native, rows, h, k)
    gated_reduce_(dst, srcs, gates, h)
    bad, _, first = native.verify_gated_reduced(dst.data_ptr(), nbytes, seeds, GATE_SEED, h, _stream())
    assert (bad, first) == (0, 2**64 - 1)
    assert native.verify_gated_reduced(dst.data_ptr(), nbytes, seeds, GATE_SEED + 1, h, _stream())[0] > 0
    word, bit = 2 * 768 + 5, 19  # row 2, the high half
    dst[4 * word + bit // 8] ^= 1 << (bit % 8)
    bad, _, first = native.verify_gated_reduced(dst.data_ptr(), nbytes, seeds, GATE_SEED, h, _stream())
    assert (bad, first) == (1, 4 * word)


def test_gated_products_round_halfway_sums_to_even(native):
    """0.5 * 2 + 0.25 * 2^-6 = 1 + 2^-8 lies halfway between the bf16 values 1
    (even) and 1 + 2^-7; 0.5 * (2 + 2^-6) + 2^-8 halfway between 1 + 2^-7 (odd)
    and 1 + 2^-6 (even)."""
    rows, h = 5, 512
    a = torch.full((rows * h // 2,), 0x40014000, dtype=torch.int64)
    b = torch.full((rows * h // 2,), 0x3C803C80, dtype=torch.int64)
    gates = torch.tensor([0x3E803F00, 0, 0, 0] * rows, dtype=torch.int64)  # gate 0 = 0.5, gate 1 = 0.25
    want = reference_gated_reduce([a, b], gates, h)
    assert int(want[0]) == 0x3F823F80
    dst = torch.empty(rows * 2 * h, dtype=torch.uint8, device="cuda")
    gated_reduce_(dst, [words_to_bytes(a).cuda(), words_to_bytes(b).cuda()], words_to_bytes(gates).cuda(), h)
    assert torch.equal(dst.cpu(), words_to_bytes(want))
