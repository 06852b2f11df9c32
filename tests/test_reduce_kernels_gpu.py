"""The gfx950 receive-and-reduce kernels on one GPU: bit-exact against the
plain-PyTorch reference, on operands from the operand fill, between guards."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import reduce_, reference_operands, reference_reduce, words_to_bytes

pytestmark = pytest.mark.gpu

DTYPES = ["u32", "f32", "bf16"]
MIB4 = (1 << 20) + 4
SIZES = [4, 12, 16, 4092, 4096, 4100, 3 * 4096 + 12, MIB4]  # tails, one / several blocks, odd block counts
GUARD = 256


@functools.lru_cache(maxsize=None)
def _ref_operand(nbytes, seed, dtype):
    return reference_operands(nbytes, seed, dtype)


@functools.lru_cache(maxsize=None)
def _ref_sum(nbytes, k, dtype):
    return words_to_bytes(reference_reduce([_ref_operand(nbytes, 900 + i, dtype) for i in range(k)], dtype))


def _guarded(nbytes):
    """A 0xAB-filled buffer and its 16-byte aligned payload view of nbytes."""
    whole = torch.full((2 * GUARD + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + nbytes:] == 0xAB).all())


def _sources(native, nbytes, k, dtype):
    srcs = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(k)]
    for i, s in enumerate(srcs):
        native.fill_operand(s.data_ptr(), nbytes, 900 + i, dtype, int(torch.cuda.current_stream().cuda_stream))
    return srcs


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 9])  # 9: a second launch with dst as operand 0
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_matches_reference(native, dtype, k, coherent):
    for nbytes in SIZES:
        whole, dst = _guarded(nbytes)
        reduce_(dst, _sources(native, nbytes, k, dtype), dtype, coherent=coherent)
        assert torch.equal(dst.cpu(), _ref_sum(nbytes, k, dtype)), nbytes
        assert _guards_intact(whole, nbytes), nbytes


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_grid_stride_passes(native, dtype, coherent):
    whole, dst = _guarded(MIB4)
    reduce_(dst, _sources(native, MIB4, 3, dtype), dtype, coherent=coherent, max_blocks=2)
    assert torch.equal(dst.cpu(), _ref_sum(MIB4, 3, dtype)) and _guards_intact(whole, MIB4)


@pytest.mark.parametrize("sizes", [[4100, 3 * 4096 + 12, 16], [8192] * 4], ids=["search", "uniform"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_reduce_many_one_launch(native, dtype, sizes):
    bufs = [_guarded(n) for n in sizes]
    srcs = [_sources(native, n, 2, dtype) for n in sizes]
    native.reduce_many([(d.data_ptr(), [s.data_ptr() for s in ss], n) for (_, d), ss, n in zip(bufs, srcs, sizes)],
                       dtype, int(torch.cuda.current_stream().cuda_stream))
    for (whole, d), n in zip(bufs, sizes):
        assert torch.equal(d.cpu(), _ref_sum(n, 2, dtype)) and _guards_intact(whole, n), n


def test_bf16_rounds_halfway_sums_to_even(native):
    """1 + 2^-8 lies halfway between the bf16 values 1 (even) and 1 + 2^-7;
    (1 + 2^-7) + 2^-8 halfway between 1 + 2^-7 (odd) and 1 + 2^-6 (even)."""
    nwords = 1025  # a block and a tail word
    a = torch.full((nwords,), 0x3F813F80, dtype=torch.int64)
    b = torch.full((nwords,), 0x3B803B80, dtype=torch.int64)
    want = reference_reduce([a, b], "bf16")
    assert int(want[0]) == 0x3F823F80
    dst = torch.empty(4 * nwords, dtype=torch.uint8, device="cuda")
    reduce_(dst, [words_to_bytes(a).cuda(), words_to_bytes(b).cuda()], "bf16")
    assert torch.equal(dst.cpu(), words_to_bytes(want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fill_operand_matches_reference(native, dtype):
    nbytes = 3 * 4096 + 12
    (src,) = _sources(native, nbytes, 1, dtype)
    assert torch.equal(src.cpu(), words_to_bytes(_ref_operand(nbytes, 900, dtype)))


@pytest.mark.parametrize("dtype,word,bit", [("u32", 700, 31), ("f32", 1024, 0), ("bf16", 5, 3), ("bf16", 1024, 19)])
def test_verify_reduced_finds_one_flipped_bit(native, dtype, word, bit):
    nbytes, k = 4100, 3  # word 1024 is the tail
    seeds = [900 + i for i in range(k)]
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    reduce_(dst, _sources(native, nbytes, k, dtype), dtype)
    bad, _, first = native.verify_reduced(dst.data_ptr(), nbytes, seeds, dtype, int(torch.cuda.current_stream().cuda_stream))
    assert (bad, first) == (0, 2**64 - 1)
    dst[4 * word + bit // 8] ^= 1 << (bit % 8)
    bad, _, first = native.verify_reduced(dst.data_ptr(), nbytes, seeds, dtype, int(torch.cuda.current_stream().cuda_stream))
    assert (bad, first) == (1, 4 * word)
