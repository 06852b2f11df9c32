"""The gfx950 wire-reduce-pack kernel on one GPU: the wire image of the sum of
1..8 MXFP8 / MXFP4 images, padding included, byte for byte against the float64
/ float32 PyTorch reference between guards, and the check of such an image."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_reduce, reference_wire_reduce_packed,
                                   reference_wire_roundtrip, wire_reduce_packed_, wire_unpack_)

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp8", "mxfp4"]
TILE = 8192
# one block; 63 blocks (the split mapping's second unit wholly outside); one tile; a one-block second tile; several
# tiles and a three-block one
SIZES = [64, 4032, TILE, TILE + 64, 3 * TILE + 192]
GUARD = 256
SEED = 7300  # operand k is stream SEED + k


@functools.lru_cache(maxsize=None)
def _operands(nbytes, fan_in):
    return [reference_wire_operands(nbytes, SEED + k) for k in range(fan_in)]


@functools.lru_cache(maxsize=None)
def _want(nbytes, fmt, fan_in):
    return reference_wire_reduce_packed(_operands(nbytes, fan_in), fmt)


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def _packed_sum(native, images, nbytes, fmt, **kw):
    """The kernel's image of the sum of `images` between 0xAB guards: (image, guards intact)."""
    size = native.wire_bytes(nbytes, fmt)
    whole = torch.full((2 * GUARD + size,), 0xAB, dtype=torch.uint8, device="cuda")
    dst = wire_reduce_packed_(whole[GUARD:GUARD + size], images, nbytes, fmt, **kw)
    return dst, bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + size:] == 0xAB).all())


def _of_streams(native, nbytes, fmt, fan_in, **kw):
    images = [torch.empty(native.wire_bytes(nbytes, fmt), dtype=torch.uint8, device="cuda") for _ in range(fan_in)]
    for k, im in enumerate(images):
        native.fill_packed(im.data_ptr(), nbytes, SEED + k, fmt, _st())
    return _packed_sum(native, images, nbytes, fmt, **kw)


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_image_matches_reference(native, fmt, lanes, coherent):
    for nbytes, fan_in in [(n, 8) for n in SIZES] + [(TILE + 64, k) for k in (1, 2, 3)]:
        dst, intact = _of_streams(native, nbytes, fmt, fan_in, lanes=lanes, coherent=coherent)
        assert torch.equal(dst.cpu(), _want(nbytes, fmt, fan_in)) and intact, (nbytes, fan_in)


@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_stride_passes(native, fmt):
    dst, intact = _of_streams(native, 5 * TILE + 192, fmt, 3, max_blocks=2)
    assert torch.equal(dst.cpu(), _want(5 * TILE + 192, fmt, 3)) and intact


@pytest.mark.parametrize("fmt", FORMATS)
def test_next_hop_can_unpack_the_image(native, fmt):
    nbytes = TILE + 64
    image = _of_streams(native, nbytes, fmt, 3)[0]
    got = wire_unpack_(torch.empty(nbytes, dtype=torch.uint8, device="cuda"), image, fmt)
    b = reference_wire_reduce(_operands(nbytes, 3), fmt).to(torch.int64).reshape(-1, 4)
    assert torch.equal(got.cpu(), reference_wire_roundtrip(b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24), fmt))


# One block.  An operand is (code of element 0, code of the odd elements, code of the other even ones, scale byte);
# the image due is given the same way.  e4m3: 0x38 = 1.0, 0x3E = 1.75, 0x18 = 2^-4, 0x01 = 2^-9, 0x3C = 1.5; e2m1:
# 0x2 = 1.0, 0x3 = 1.5, 0x4 = 2.0, 0x1 = 0.5; the sign is bit 7 / bit 3.
DIRECTED = {
    # amax 1.75 / 1.5 is the largest significand: the scale is 2^(E - 8) / 2^(E - 2) and the code is the format's maximum
    ("amax-at-top", "mxfp8"): ([(0x3E, 0x3E, 0x3E, 127)], (119, 0x7E, 0x7E, 0x7E)),
    ("amax-at-top", "mxfp4"): ([(0x3, 0x3, 0x3, 127)], (125, 0x7, 0x7, 0x7)),
    # + 2^-7, one bf16 ulp: the scale byte steps; 225 / 128 -> 224 / 128 = 1.75 x 2^7, 3.016 -> 3
    ("amax-one-ulp-above", "mxfp8"): ([(0x3E, 0x3E, 0x3E, 127), (0x38, 0x38, 0x38, 120)], (120, 0x76, 0x76, 0x76)),
    ("amax-one-ulp-above", "mxfp4"): ([(0x3, 0x3, 0x3, 127), (0x2, 0x2, 0x2, 120)], (126, 0x5, 0x5, 0x5)),
    ("cancels-to-plus-zero", "mxfp8"): ([(0x38, 0x38, 0x38, 127), (0xB8, 0xB8, 0xB8, 127)], (127, 0, 0, 0)),
    ("cancels-to-plus-zero", "mxfp4"): ([(0x2, 0x2, 0x2, 127), (0xA, 0xA, 0xA, 127)], (127, 0, 0, 0)),
    ("minus-zeros", "mxfp8"): ([(0x80, 0x80, 0x80, 127)] * 2, (127, 0x80, 0x80, 0x80)),
    ("minus-zeros", "mxfp4"): ([(0x8, 0x8, 0x8, 127)] * 2, (127, 0x8, 0x8, 0x8)),
    # element 0 sums to 1.0 and sets the scale (2^-8 / 2^-2); the odd elements (3 x 2^-17 / 2^-3) land on a subnormal
    # of the format, the even ones (-2^-20 / -2^-5) below half its smallest step: -0
    ("large-and-subnormals", "mxfp8"): ([(0x38, 0x00, 0x00, 127), (0x00, 0x3C, 0x98, 111)], (119, 0x78, 0x03, 0x80)),
    ("large-and-subnormals", "mxfp4"): ([(0x2, 0x0, 0x0, 127), (0x0, 0x4, 0x9, 123)], (125, 0x6, 0x1, 0x8)),
    # 1 + 2^-4 + 2^-9 (1 + 2^-2 + 2^-9) beside 1.75 (1.5): the bf16 rounding drops the 2^-9, the quantiser sees the tie
    # between 1.0 and 1.125 (1.5) and goes to even, 1.0; quantising the f32 sum would give 0x79 / 0x7
    ("rounds-to-bf16-first", "mxfp8"): ([(0x3E, 0x38, 0x38, 127), (0x00, 0x18, 0x18, 127), (0x00, 0x01, 0x01, 127)],
                                        (119, 0x7E, 0x78, 0x78)),
    ("rounds-to-bf16-first", "mxfp4"): ([(0x3, 0x2, 0x2, 127), (0x0, 0x2, 0x2, 125), (0x0, 0x2, 0x2, 118)], (125, 0x7, 0x6, 0x6)),
}


def _block(fmt, first, odd, even, sb):
    """The image of one block: element bytes, the scale byte, zeros up to a multiple of 16."""
    codes = [first if j == 0 else odd if j % 2 else even for j in range(32)]
    elems = codes if fmt == "mxfp8" else [codes[j] | codes[j + 1] << 4 for j in range(0, 32, 2)]
    return torch.tensor(elems + [sb] + [0] * (-(len(elems) + 1) % 16), dtype=torch.uint8)


@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("name,fmt", sorted(DIRECTED))
def test_directed_images(native, name, fmt, lanes):
    operands, (sb, first, odd, even) = DIRECTED[name, fmt]
    dst, intact = _packed_sum(native, [_block(fmt, *op).cuda() for op in operands], 64, fmt, lanes=lanes)
    assert dst.cpu().tolist() == _block(fmt, first, odd, even, sb).tolist() and intact


@pytest.mark.parametrize("where", ["full-tile-word", "ragged-tile-word", "scale-byte"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_verify_finds_one_flipped_bit(native, fmt, where):
    nbytes, seeds = TILE + 64, [SEED + k for k in range(3)]
    tile = native.wire_bytes(TILE, fmt)  # the second tile's offset; its scale bytes are the last 128 of the first
    at, named = {"full-tile-word": (401, 400), "ragged-tile-word": (tile + 14, tile + 12), "scale-byte": (tile - 51,) * 2}[where]
    image = _of_streams(native, nbytes, fmt, 3)[0].clone()
    assert native.verify_wire_reduced_packed(image.data_ptr(), nbytes, seeds, fmt, _st())[::2] == (0, 2**64 - 1)
    image[at] ^= 0x10
    assert native.verify_wire_reduced_packed(image.data_ptr(), nbytes, seeds, fmt, _st())[::2] == (1, named)
