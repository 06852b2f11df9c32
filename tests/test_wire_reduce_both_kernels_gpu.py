"""The gfx950 wire-reduce-pack kernels with both outputs (`both`) on one GPU: the
wire image of the sum and the bf16 it widens to, from one launch, against the
float64 / float32 PyTorch reference between guards; mxfp6's image alone; the
checks of both outputs."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (reference_wire_operands, reference_wire_reduce, reference_wire_reduce_packed,
                                   reference_wire_roundtrip, wire_reduce_packed_)

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp8", "mxfp6", "mxfp4"]
TILE = 8192
# one block; 63 blocks; one tile; a one-block second tile; several tiles and a three-block one
SIZES = [64, 4032, TILE, TILE + 64, 3 * TILE + 192]
WAVE6 = 2 * TILE + 65 * 64  # mxfp6: one block past a wave boundary of the workgroup's second tile
GUARD = 256
SEED = 7700  # operand k is stream SEED + k


def _words(b):
    b = b.to(torch.int64).reshape(-1, 4)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


@functools.lru_cache(maxsize=None)
def _want(nbytes, fmt, fan_in, own):
    """(image, bf16): the reference's packed sum and the round trip of its bf16 sum."""
    ops = tuple(reference_wire_operands(nbytes, SEED + k) for k in range(fan_in))
    return (reference_wire_reduce_packed(ops, fmt, own_bf16=own),
            reference_wire_roundtrip(_words(reference_wire_reduce(ops, fmt, own_bf16=own)), fmt))


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def _run(native, srcs, nbytes, fmt, both=True, **kw):
    """The kernel's outputs, each between 0xAB guards: (image, bf16 or None, guards intact)."""
    size = native.wire_bytes(nbytes, fmt)
    whole = torch.full((4 * GUARD + size + nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    image, bf16 = whole[GUARD:GUARD + size], whole[3 * GUARD + size:3 * GUARD + size + nbytes]
    wire_reduce_packed_(image, srcs, nbytes, fmt, both=bf16 if both else None, **kw)
    used = torch.zeros_like(whole, dtype=torch.bool)
    used[GUARD:GUARD + size] = True
    used[3 * GUARD + size:3 * GUARD + size + nbytes] = both
    return image, bf16 if both else None, bool((whole[~used] == 0xAB).all())


def _of_streams(native, nbytes, fmt, fan_in, own=False, **kw):
    srcs = []
    for k in range(fan_in):
        srcs.append(torch.empty(nbytes if own and k == 0 else native.wire_bytes(nbytes, fmt), dtype=torch.uint8, device="cuda"))
        if own and k == 0:
            native.fill_wire_operand(srcs[0].data_ptr(), nbytes, SEED, _st())
        else:
            native.fill_packed(srcs[k].data_ptr(), nbytes, SEED + k, fmt, _st())
    return _run(native, srcs, nbytes, fmt, own_bf16=own, **kw)


@pytest.mark.parametrize("own", [False, True], ids=["images", "own-bf16"])
@pytest.mark.parametrize("coherent", [False, True], ids=["local", "coherent"])
@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_both_outputs_match_reference(native, fmt, lanes, coherent, own):
    sizes = SIZES + [WAVE6] if fmt == "mxfp6" else SIZES
    for nbytes, fan_in in [(n, 8) for n in sizes] + [(TILE + 64, k) for k in (1, 2, 3)]:
        mask = ((1 << fan_in) - 1 - own) if coherent else 0  # a bf16 own shard (bit 0) is local
        image, bf16, intact = _of_streams(native, nbytes, fmt, fan_in, own, lanes=lanes, coherent=mask)
        want_image, want_bf16 = _want(nbytes, fmt, fan_in, own)
        assert torch.equal(image.cpu(), want_image) and torch.equal(bf16.cpu(), want_bf16) and intact, (nbytes, fan_in)


@pytest.mark.parametrize("lanes", ["split", "contiguous"])
def test_mxfp6_image_alone(native, lanes):
    for nbytes in SIZES + [WAVE6]:
        image, _, intact = _of_streams(native, nbytes, "mxfp6", 8, both=False, lanes=lanes)
        assert torch.equal(image.cpu(), _want(nbytes, "mxfp6", 8, False)[0]) and intact, nbytes


@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_stride_passes(native, fmt):
    image, bf16, intact = _of_streams(native, 5 * TILE + 192, fmt, 3, max_blocks=2)
    want_image, want_bf16 = _want(5 * TILE + 192, fmt, 3, False)
    assert torch.equal(image.cpu(), want_image) and torch.equal(bf16.cpu(), want_bf16) and intact


# One mxfp6 block.  An operand is (code of element 0, code of the odd elements, code of the other even ones, scale
# byte); the image due is (scale byte, the three codes).  e2m3: 0x08 = 1.0, 0x0C = 1.5, 0x0F = 1.875, 0x18 = 4.0,
# 0x1F = 7.5, 0x01 = 0.125 and 0x03 = 0.375 (subnormals); the sign is bit 5.
DIRECTED = {
    # amax 1.875 is the largest significand: the scale is 2^(E - 2) and the code the format's maximum
    "amax-at-top": ([(0x0F, 0x0F, 0x0F, 127)], (125, 0x1F, 0x1F, 0x1F)),
    # + 2^-7, one bf16 ulp: the scale byte steps; 241 / 128 under 2^-1 is 3.766 -> 3.75
    "amax-one-ulp-above": ([(0x0F, 0x0F, 0x0F, 127), (0x08, 0x08, 0x08, 120)], (126, 0x17, 0x17, 0x17)),
    "cancels-to-plus-zero": ([(0x08, 0x08, 0x08, 127), (0x28, 0x28, 0x28, 127)], (127, 0, 0, 0)),
    "minus-zeros": ([(0x20, 0x20, 0x20, 127)] * 2, (127, 0x20, 0x20, 0x20)),
    # element 0 sums to 1.0 and sets the scale 2^-2; the odd elements (1.5 x 2^-4) land on the subnormal 0.375, the
    # even ones (-2^-7) below half the smallest step 2^-5: -0
    "large-and-subnormals": ([(0x08, 0x00, 0x00, 127), (0x00, 0x0C, 0x21, 123)], (125, 0x18, 0x03, 0x20)),
    # 1 + 2^-4 + 2^-9 beside 1.875: the bf16 rounding drops the 2^-9, the quantiser sees the tie between 4.0 and 4.5
    # and goes to even, 4.0; quantising the f32 sum would give 0x19
    "rounds-to-bf16-first": ([(0x0F, 0x08, 0x08, 127), (0x00, 0x08, 0x08, 123), (0x00, 0x08, 0x08, 118)], (125, 0x1F, 0x18, 0x18)),
}


def _codes(first, odd, even):
    return torch.tensor([first if j == 0 else odd if j % 2 else even for j in range(32)], dtype=torch.int64)


def _block6(first, odd, even, sb):
    """The image of one block: 24 element bytes, zeros up to 32, the scale byte, zeros up to 48."""
    c = _codes(first, odd, even)
    v = c[0::4] | (c[1::4] << 6) | (c[2::4] << 12) | (c[3::4] << 18)
    elems = torch.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], dim=1).reshape(-1).tolist()
    return torch.tensor(elems + [0] * 8 + [sb] + [0] * 15, dtype=torch.uint8)


def _bf16_words(first, odd, even, sb):
    """The block's values as bf16 words (exact: a 4-bit significand times a power of two)."""
    c = _codes(first, odd, even)
    e, m = (c >> 3) & 3, (c & 7).to(torch.float64)
    mag = torch.where(e == 0, m / 8, (1 + m / 8) * 2.0 ** (e - 1).to(torch.float64)) * 2.0 ** (sb - 127)
    bits = (torch.where((c & 0x20) != 0, -mag, mag).to(torch.float32).view(torch.int32).to(torch.int64) >> 16) & 0xFFFF
    return bits[0::2] | (bits[1::2] << 16)


@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_mxfp6_blocks(native, name, lanes):
    operands, (sb, first, odd, even) = DIRECTED[name]
    due = _block6(first, odd, even, sb)
    words = [_bf16_words(*op) for op in operands]
    assert torch.equal(reference_wire_reduce_packed(words, "mxfp6"), due)
    image, bf16, intact = _run(native, [_block6(*op).cuda() for op in operands], 64, "mxfp6", lanes=lanes)
    assert image.cpu().tolist() == due.tolist() and intact
    assert torch.equal(bf16.cpu(), reference_wire_roundtrip(_words(reference_wire_reduce(words, "mxfp6")), "mxfp6"))


TILE6 = 3200  # a full mxfp6 tile; its scale bytes are its last 128
# (which output, the byte to damage, the offset the check names): the roundtrip check counts 32-bit words, the mxfp6
# image check 6-byte groups of 8 codes and scale bytes
FLIPS = {"bf16-full-tile-word": (1203, 1200), "bf16-ragged-tile-word": (TILE + 14, TILE + 12),
         "image-full-tile-word": (401, 396), "image-ragged-tile-word": (TILE6 + 14, TILE6 + 12), "image-scale-byte": (TILE6 - 51,) * 2}


@pytest.mark.parametrize("where", sorted(FLIPS))
def test_checks_find_one_flipped_bit(native, where):
    nbytes, seeds, (at, named) = TILE + 64, [SEED + k for k in range(3)], FLIPS[where]
    image, bf16, _ = _of_streams(native, nbytes, "mxfp6", 3)
    if where.startswith("bf16"):
        def check():
            return native.verify_wire_reduced(bf16.data_ptr(), nbytes, seeds, "mxfp6", _st(), roundtrip=True)[::2]
    else:
        def check():
            return native.verify_wire_reduced_packed(image.data_ptr(), nbytes, seeds, "mxfp6", _st())[::2]
    assert check() == (0, 2**64 - 1)
    (bf16 if where.startswith("bf16") else image)[at] ^= 0x10
    assert check() == (1, named)
