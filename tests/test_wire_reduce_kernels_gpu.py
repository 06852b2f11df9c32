"""The gfx950 wire-reduce kernel on one GPU: the bf16 sum of 1..8 MXFP8 / MXFP4
images bit for bit against the float64 / float32 PyTorch reference, between
guards, and the check of such a sum."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import reference_wire_operands, reference_wire_reduce, wire_reduce_

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp8", "mxfp4"]
TILE = 8192
# one block; 63 blocks (the split mapping's second unit wholly outside); one tile; a one-block second tile; several
# tiles and a three-block one
SIZES = [64, 4032, TILE, TILE + 64, 3 * TILE + 192]
GUARD = 256
SEED = 7100  # operand k is stream SEED + k


@functools.lru_cache(maxsize=None)
def _want(nbytes, fmt, fan_in):
    return reference_wire_reduce([reference_wire_operands(nbytes, SEED + k) for k in range(fan_in)], fmt)


def _guarded(nbytes):
    """A 0xAB-filled buffer and its 16-byte aligned view of nbytes."""
    whole = torch.full((2 * GUARD + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    return whole, whole[GUARD:GUARD + nbytes]


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def _sum(native, nbytes, fmt, fan_in, **kw):
    """The kernel's sum of the fill_packed images of streams SEED.. : (equals the reference, guards intact, dst)."""
    images = [torch.empty(native.wire_bytes(nbytes, fmt), dtype=torch.uint8, device="cuda") for _ in range(fan_in)]
    for k, im in enumerate(images):
        native.fill_packed(im.data_ptr(), nbytes, SEED + k, fmt, _st())
    whole, dst = _guarded(nbytes)
    wire_reduce_(dst, images, fmt, **kw)
    intact = bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + nbytes:] == 0xAB).all())
    return torch.equal(dst.cpu(), _want(nbytes, fmt, fan_in)), intact, dst


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_sum_matches_reference(native, fmt, lanes, coherent):
    for nbytes, fan_in in [(n, 8) for n in SIZES] + [(TILE + 64, k) for k in (1, 2, 3)]:
        assert _sum(native, nbytes, fmt, fan_in, lanes=lanes, coherent=coherent)[:2] == (True, True), (nbytes, fan_in)


@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_stride_passes(native, fmt):
    assert _sum(native, 5 * TILE + 192, fmt, 3, max_blocks=2)[:2] == (True, True)


# (per operand: mxfp8 code, mxfp4 code, scale byte), the bf16 bits due.  1.0 is 0x38 / 0x2 under scale byte 127,
# 2^-8 the same codes under 119, 1.5 x 2^-7 is 0x3C / 0x3 under 120; the sign is bit 7 / bit 3.
DIRECTED = {
    "tie-even-stays": ([(0x38, 0x2, 127), (0x38, 0x2, 119)], 0x3F80),          # 1 + 2^-8
    "tie-odd-goes-up": ([(0x38, 0x2, 127), (0x3C, 0x3, 120)], 0x3F82),         # 1 + 1.5 x 2^-7; truncation: 0x3F81
    "rounds-once": ([(0x38, 0x2, 127), (0x38, 0x2, 119), (0x38, 0x2, 119)], 0x3F81),  # a rounding per add: 0x3F80
    "cancel-plus-minus-zero": ([(0x38, 0x2, 127), (0xB8, 0xA, 127), (0x80, 0x8, 127)], 0x0000),
    "minus-zeros": ([(0x80, 0x8, 127), (0x80, 0x8, 127)], 0x8000),
}


@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_sums(native, name, fmt, lanes):
    operands, bits = DIRECTED[name]
    images = []
    for c8, c4, sb in operands:  # one block: its element bytes, the scale byte, zeros up to 16
        elems = [c8] * 32 if fmt == "mxfp8" else [c4 | c4 << 4] * 16
        images.append(torch.tensor(elems + [sb] + [0] * (-(len(elems) + 1) % 16), dtype=torch.uint8).cuda())
    dst = torch.empty(64, dtype=torch.uint8, device="cuda")
    wire_reduce_(dst, images, fmt, lanes=lanes)
    assert dst.cpu().view(torch.int16).tolist() == [bits - (bits >> 15 << 16)] * 32


@pytest.mark.parametrize("word,bit", [(700, 31), (2048 + 5, 3)], ids=["full-tile", "ragged-tile"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_verify_wire_reduced_finds_one_flipped_bit(native, fmt, word, bit):
    nbytes, seeds = TILE + 64, [SEED + k for k in range(3)]
    dst = _sum(native, nbytes, fmt, 3)[2]
    assert native.verify_wire_reduced(dst.data_ptr(), nbytes, seeds, fmt, _st())[::2] == (0, 2**64 - 1)
    dst[4 * word + bit // 8] ^= 1 << (bit % 8)
    assert native.verify_wire_reduced(dst.data_ptr(), nbytes, seeds, fmt, _st())[::2] == (1, 4 * word)
