"""The gfx950 mxfp6 (e2m3) kernels on one GPU: pack, fill_packed, unpack, the
sum of images and the checks, bit for bit against the float64 PyTorch reference,
between guards."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_pack, reference_wire_reduce,
                                   reference_wire_roundtrip, wire_pack_, wire_reduce_, wire_unpack_, words_to_bytes)

pytestmark = pytest.mark.gpu

FMT = "mxfp6"
TILE = 8192
BIG = (1 << 20) + 64
# one block; two (an even ragged tile); 63 and 3 blocks (odd: the padded element section); a full tile; a one-block
# second tile; many workgroups and a ragged end
SIZES = [64, 128, 4032, TILE, TILE + 64, 3 * TILE + 192, BIG]
REDUCE_SIZES = [64, 4032, TILE + 64, 3 * TILE + 192]
GUARD = 256
SEED = 4242
forms = pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
both_lanes = pytest.mark.parametrize("lanes", ["split", "contiguous"])


@functools.lru_cache(maxsize=None)
def _ref(nbytes):
    """(payload bytes, wire image, unpacked payload bytes) of operand stream SEED."""
    w = reference_wire_operands(nbytes, SEED)
    return words_to_bytes(w), reference_wire_pack(w, FMT), reference_wire_roundtrip(w, FMT)


@functools.lru_cache(maxsize=None)
def _sum_ref(nbytes, fan_in):
    return reference_wire_reduce([reference_wire_operands(nbytes, SEED + k) for k in range(fan_in)], FMT)


def _guarded(nbytes):
    """A 0xAB-filled buffer and its 16-byte aligned view of nbytes."""
    whole = torch.full((2 * GUARD + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _is(whole, view, want):
    """The view holds `want` and the guards around it are intact."""
    n = view.numel()
    return torch.equal(view.cpu(), want) and bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + n:] == 0xAB).all())


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def test_pack_and_fill_packed_match_reference(native):
    for nbytes in SIZES:
        payload, image, _ = _ref(nbytes)
        assert image.numel() == native.wire_bytes(nbytes, FMT)
        whole, dst = _guarded(image.numel())
        wire_pack_(dst, payload.cuda(), FMT)
        assert _is(whole, dst, image), nbytes  # both zero paddings too
        whole, dst = _guarded(image.numel())
        native.fill_packed(dst.data_ptr(), nbytes, SEED, FMT, _st())
        assert _is(whole, dst, image), nbytes


@forms
@pytest.mark.parametrize("lanes,max_blocks", [("split", 0), ("contiguous", 0), ("auto", 2)])
def test_unpack_matches_reference(native, lanes, max_blocks, coherent):
    for nbytes in SIZES if not max_blocks else [BIG]:  # max_blocks: grid-stride passes
        whole, dst = _guarded(nbytes)
        wire_unpack_(dst, _ref(nbytes)[1].cuda(), FMT, coherent=coherent, lanes=lanes, max_blocks=max_blocks)
        assert _is(whole, dst, _ref(nbytes)[2]), nbytes


@forms
@pytest.mark.parametrize("sizes", [[TILE + 64, 3 * TILE + 192, 64], [2 * TILE] * 4], ids=["search", "uniform"])
def test_unpack_many_one_launch(native, sizes, coherent):
    bufs = [_guarded(n) for n in sizes]
    srcs = [_ref(n)[1].cuda() for n in sizes]
    native.wire_unpack_many([(d.data_ptr(), s.data_ptr(), n) for (_, d), s, n in zip(bufs, srcs, sizes)], FMT, _st(), coherent)
    for (whole, d), n in zip(bufs, sizes):
        assert _is(whole, d, _ref(n)[2]), n


# Directed blocks as bf16 bit patterns: (the 32 elements, the scale byte due, {element: code due}).  The first element
# is the amax; 1.875 x 2^0 is e2m3's 7.5 under scale 2^-2 (byte 125), where 1.0 is 4.0 = code 0x18.
def _block(first, rest):
    return [first] + (rest * 31)[:31]


DIRECTED = {
    "amax-at-max": (_block(0x3FF0, [0x3F80]), 125, {0: 0x1F, 1: 0x18}),
    "amax-above-max": (_block(0x3FF1, [0x3F80]), 126, {0: 0x17, 1: 0x10}),  # one ulp more: 3.766 -> 3.75 under 2^-1
    # halfway between two grid values: the lower neighbour even (stays), odd (goes up), negative too
    "ties": (_block(0x3FF0, [0x3F88, 0x3F98, 0xBF98]), 125, {1: 0x18, 2: 0x1A, 3: 0x3A}),
    "equal": ([0x4049] * 32, 126, {0: 0x1D, 31: 0x1D}),  # 3.14 / 0.5 = 6.28 -> 6.5
    # the subnormals (steps of 0.125: 2^-4, 2^-5, 1.5 x 2^-6 under 2^-2), a tie at half the smallest step, both zeros
    "subnormal": (_block(0x3FF0, [0x3D80, 0x3D00, 0x3CC0, 0x3C80, 0xBC80, 0x0000, 0x8000]), 125,
                  {1: 2, 2: 1, 3: 1, 4: 0, 5: 0x20, 6: 0, 7: 0x20}),
}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_blocks(native, name):
    block, scale, codes = DIRECTED[name]
    nblocks = 129  # one tile and one block: the full and the (odd) ragged tile both see it
    halves = torch.tensor(block, dtype=torch.int64)
    words = (halves[0::2] | (halves[1::2] << 16)).repeat(nblocks)
    image, want = reference_wire_pack(words, FMT), reference_wire_roundtrip(words, FMT)
    # The reference itself, pinned: the scale bytes (the second tile's behind 24 + 8 bytes) and a few codes.
    assert int(image[128 * 24]) == scale and int(image[3200 + 32]) == scale and image.numel() == 3200 + 48
    bits = sum(int(b) << (8 * i) for i, b in enumerate(image[:24].tolist()))
    assert {j: (bits >> (6 * j)) & 63 for j in codes} == codes
    whole, packed = _guarded(image.numel())
    wire_pack_(packed, words_to_bytes(words).cuda(), FMT)
    assert _is(whole, packed, image)
    for lanes in ("split", "contiguous"):
        whole, dst = _guarded(64 * nblocks)
        wire_unpack_(dst, packed, FMT, lanes=lanes)
        assert _is(whole, dst, want), lanes


def _sum(native, nbytes, fan_in, **kw):
    """The kernel's sum of the fill_packed images of streams SEED.. : (right and guards intact, dst)."""
    images = [torch.empty(native.wire_bytes(nbytes, FMT), dtype=torch.uint8, device="cuda") for _ in range(fan_in)]
    for k, im in enumerate(images):
        native.fill_packed(im.data_ptr(), nbytes, SEED + k, FMT, _st())
    whole, dst = _guarded(nbytes)
    wire_reduce_(dst, images, FMT, **kw)
    return _is(whole, dst, _sum_ref(nbytes, fan_in)), dst


# mixed: sources 0, 2, 5 and 7 (as far as the op has them) are read in the cross-GPU form, the others as local images
@pytest.mark.parametrize("coherent", [False, True, 0xA5], ids=["local", "coherent", "mixed"])
@both_lanes
@pytest.mark.parametrize("fan_in", [1, 2, 3, 8])
def test_sum_matches_reference(native, fan_in, lanes, coherent):
    if coherent not in (False, True):
        coherent &= (1 << fan_in) - 1
    for nbytes in REDUCE_SIZES:
        assert _sum(native, nbytes, fan_in, lanes=lanes, coherent=coherent)[0], nbytes


def test_sum_grid_stride_passes(native):
    assert _sum(native, 5 * TILE + 192, 3, max_blocks=2)[0]


# (per operand: code, scale byte), the bf16 bits due.  1.0 is code 0x08 under scale byte 127, 2^-8 the same code
# under 119, 1.5 x 2^-7 is 0x0C under 120; the sign is bit 5.
DIRECTED_SUMS = {
    "tie-even-stays": ([(0x08, 127), (0x08, 119)], 0x3F80),          # 1 + 2^-8
    "tie-odd-goes-up": ([(0x08, 127), (0x0C, 120)], 0x3F82),         # 1 + 1.5 x 2^-7; truncation: 0x3F81
    "rounds-once": ([(0x08, 127), (0x08, 119), (0x08, 119)], 0x3F81),  # a rounding per add: 0x3F80
    "cancel-plus-minus-zero": ([(0x08, 127), (0x28, 127), (0x20, 127)], 0x0000),
    "minus-zeros": ([(0x20, 127), (0x20, 127)], 0x8000),
    "one-operand-passes": ([(0x2C, 120)], 0xBC40),                   # -1.5 x 2^-7
}


@both_lanes
@pytest.mark.parametrize("name", sorted(DIRECTED_SUMS))
def test_directed_sums(native, name, lanes):
    operands, bits = DIRECTED_SUMS[name]
    images = []
    for c, sb in operands:  # one block: 32 equal codes in 24 bytes, 8 zeros, the scale byte, zeros up to 16
        v = c | c << 6 | c << 12 | c << 18
        images.append(torch.tensor([v & 0xFF, (v >> 8) & 0xFF, v >> 16] * 8 + [0] * 8 + [sb] + [0] * 15, dtype=torch.uint8).cuda())
    dst = torch.empty(64, dtype=torch.uint8, device="cuda")
    wire_reduce_(dst, images, FMT, lanes=lanes)
    assert dst.cpu().view(torch.int16).tolist() == [bits - (bits >> 15 << 16)] * 32


@pytest.mark.parametrize("word,bit", [(700, 31), (2048 + 5, 3)], ids=["full-tile", "ragged-tile"])
def test_verify_finds_one_flipped_bit(native, word, bit):
    nbytes, seeds = TILE + 64, [SEED + k for k in range(3)]
    dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    wire_unpack_(dst, _ref(nbytes)[1].cuda(), FMT)
    for buf, check in ((dst, lambda p: native.verify_unpacked(p, nbytes, SEED, FMT, _st())),
                       (_sum(native, nbytes, 3)[1], lambda p: native.verify_wire_reduced(p, nbytes, seeds, FMT, _st()))):
        assert check(buf.data_ptr())[::2] == (0, 2**64 - 1)
        buf[4 * word + bit // 8] ^= 1 << (bit % 8)
        assert check(buf.data_ptr())[::2] == (1, 4 * word)
