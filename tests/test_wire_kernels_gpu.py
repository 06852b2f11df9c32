"""The gfx950 wire-format kernels on one GPU: pack, unpack, fill_packed and
verify_unpacked bit for bit against the float64 PyTorch reference, between guards."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_pack, reference_wire_roundtrip, wire_pack_,
                                   wire_unpack_, words_to_bytes)

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp8", "mxfp4"]
TILE = 8192
BIG = (1 << 20) + 64
# one block; two; a ragged tile one block short; exactly one tile; a one-block second tile; several tiles and a
# three-block one; many workgroups and a ragged end
SIZES = [64, 128, 4032, TILE, TILE + 64, 3 * TILE + 192, BIG]
GUARD = 256
SEED = 4242
forms = pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])


@functools.lru_cache(maxsize=None)
def _ref(nbytes, fmt, seed=SEED):
    """(payload bytes, wire image, unpacked payload bytes) of operand stream `seed`."""
    w = reference_wire_operands(nbytes, seed)
    return words_to_bytes(w), reference_wire_pack(w, fmt), reference_wire_roundtrip(w, fmt)


def _guarded(nbytes):
    """A 0xAB-filled buffer and its 16-byte aligned view of nbytes."""
    whole = torch.full((2 * GUARD + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + nbytes:] == 0xAB).all())


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_and_fill_packed_match_reference(native, fmt):
    for nbytes in SIZES:
        payload, image, _ = _ref(nbytes, fmt)
        whole, dst = _guarded(image.numel())
        wire_pack_(dst, payload.cuda(), fmt)
        assert torch.equal(dst.cpu(), image) and _guards_intact(whole, image.numel()), nbytes  # the zero padding too
        whole, dst = _guarded(image.numel())
        native.fill_packed(dst.data_ptr(), nbytes, SEED, fmt, _st())
        assert torch.equal(dst.cpu(), image) and _guards_intact(whole, image.numel()), nbytes


@forms
@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_matches_reference(native, fmt, lanes, coherent):
    for nbytes in SIZES:
        _, image, want = _ref(nbytes, fmt)
        whole, dst = _guarded(nbytes)
        wire_unpack_(dst, image.cuda(), fmt, coherent=coherent, lanes=lanes)
        assert torch.equal(dst.cpu(), want) and _guards_intact(whole, nbytes), nbytes


@forms
@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_grid_stride_passes(native, fmt, coherent):
    _, image, want = _ref(BIG, fmt)
    whole, dst = _guarded(BIG)
    wire_unpack_(dst, image.cuda(), fmt, coherent=coherent, max_blocks=2)
    assert torch.equal(dst.cpu(), want) and _guards_intact(whole, BIG)


@forms
@pytest.mark.parametrize("sizes", [[TILE + 64, 3 * TILE + 192, 64], [2 * TILE] * 4], ids=["search", "uniform"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_unpack_many_one_launch(native, fmt, sizes, coherent):
    bufs = [_guarded(n) for n in sizes]
    srcs = [_ref(n, fmt)[1].cuda() for n in sizes]
    native.wire_unpack_many([(d.data_ptr(), s.data_ptr(), n) for (_, d), s, n in zip(bufs, srcs, sizes)], fmt, _st(), coherent)
    for (whole, d), n in zip(bufs, sizes):
        assert torch.equal(d.cpu(), _ref(n, fmt)[2]) and _guards_intact(whole, n), n


# Directed blocks as bf16 bit patterns: (format, the 32 elements, the scale byte due, {element: code due}).  The
# blocks' first element is the amax; the others sit 0..15 binades below it.
def _block(first, rest):
    return [first] + (rest * 31)[:31]


DIRECTED = {
    # amax = 1.75 x 2^0 is e4m3's 448 under scale 2^-8; one ulp more needs 2^-7 (225 -> 224); 1.5 / 6 for e2m1
    "fp8-amax-at-max": ("mxfp8", _block(0x3FE0, [0x3F80]), 119, {0: 0x7E, 1: 0x78}),
    "fp8-amax-above-max": ("mxfp8", _block(0x3FE1, [0x3F80]), 120, {0: 0x76, 1: 0x70}),
    "fp4-amax-at-max": ("mxfp4", _block(0x3FC0, [0x3F80]), 125, {0: 7, 1: 6}),
    "fp4-amax-above-max": ("mxfp4", _block(0x3FC1, [0x3F80]), 126, {0: 5, 1: 4}),
    # halfway between two grid values: the lower neighbour even (stays), odd (goes up), negative too
    "fp8-ties": ("mxfp8", _block(0x3FE0, [0x3F88, 0x3F98, 0xBF98]), 119, {1: 0x78, 2: 0x7A, 3: 0xFA}),
    "fp4-ties": ("mxfp4", _block(0x3FC0, [0x3FA0, 0x3F60, 0x3F20, 0xBF20]), 125, {1: 6, 2: 6, 3: 4, 4: 12}),
    # 32 equal values
    "fp8-equal": ("mxfp8", [0x4049] * 32, 120, {0: 0x7D, 31: 0x7D}),
    "fp4-equal": ("mxfp4", [0x4049] * 32, 127, {0: 5, 31: 5}),
    # the format's subnormals, a tie at half the smallest step, and both zeros
    "fp8-subnormal": ("mxfp8", _block(0x3FE0, [0x3780, 0x3700, 0x36C0, 0x3680, 0xB680]), 119,
                      {1: 2, 2: 1, 3: 1, 4: 0, 5: 0x80}),
    "fp4-subnormal": ("mxfp4", _block(0x3FC0, [0x3E00, 0x3DC0, 0x3D80, 0xBD80]), 125, {1: 1, 2: 1, 3: 0, 4: 8}),
}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_blocks(native, name):
    fmt, block, scale, codes = DIRECTED[name]
    nblocks = 129  # one tile and one block: the full and the ragged tile both see it
    halves = torch.tensor(block, dtype=torch.int64)
    words = (halves[0::2] | (halves[1::2] << 16)).repeat(nblocks)
    image, want = reference_wire_pack(words, fmt), reference_wire_roundtrip(words, fmt)
    # The reference itself, pinned: the scale byte and a few codes of the first block.
    eb = 32 if fmt == "mxfp8" else 16
    assert int(image[128 * eb]) == scale and int(image[128 * eb + 128 + eb]) == scale
    for j, code in codes.items():
        got = int(image[j]) if fmt == "mxfp8" else (int(image[j // 2]) >> (4 * (j % 2))) & 15
        assert got == code, (j, hex(got), hex(code))
    nbytes = 64 * nblocks
    whole, packed = _guarded(image.numel())
    wire_pack_(packed, words_to_bytes(words).cuda(), fmt)
    assert torch.equal(packed.cpu(), image) and _guards_intact(whole, image.numel())
    for lanes in ("split", "contiguous"):
        whole, dst = _guarded(nbytes)
        wire_unpack_(dst, packed, fmt, lanes=lanes)
        assert torch.equal(dst.cpu(), want) and _guards_intact(whole, nbytes), lanes


@pytest.mark.parametrize("word,bit", [(700, 31), (2048 + 5, 3)], ids=["full-tile", "ragged-tile"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_verify_unpacked_finds_one_flipped_bit(native, fmt, word, bit):
    nbytes = TILE + 64
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wire_unpack_(dst, _ref(nbytes, fmt)[1].cuda(), fmt)
    assert native.verify_unpacked(dst.data_ptr(), nbytes, SEED, fmt, _st())[::2] == (0, 2**64 - 1)
    dst[4 * word + bit // 8] ^= 1 << (bit % 8)
    assert native.verify_unpacked(dst.data_ptr(), nbytes, SEED, fmt, _st())[::2] == (1, 4 * word)
