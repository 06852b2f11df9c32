"""The gfx950 wire-reduce kernels with a bf16 own shard (own_bf16) on one GPU:
operand 0 unquantised, operands 1..K-1 wire images, bit for bit against the
float64 / float32 PyTorch reference between guards, in both output forms."""
import functools

import pytest
import torch

from test_nccl_p2p_amd.ops import (reduce_, reference_wire_operands, reference_wire_reduce, reference_wire_reduce_packed,
                                   wire_reduce_, wire_reduce_packed_, wire_unpack_, words_to_bytes)

pytestmark = pytest.mark.gpu

FORMATS = ["mxfp8", "mxfp6", "mxfp4"]
PACKED = ["mxfp8", "mxfp4"]
TILE = 8192
# one block; 63 blocks (ragged inside one wave); a tile and one block (mxfp6: the workgroup's second tile at a single
# lane); one block past a wave boundary of the second mxfp6 tile; several tiles and a three-block one
SIZES = [64, 4032, TILE + 64, 2 * TILE + 65 * 64, 3 * TILE + 192]
CASES = [(n, 8) for n in SIZES] + [(TILE + 64, k) for k in (1, 2, 3)]
GUARD = 256
SEED = 7500  # operand k is stream SEED + k


@functools.lru_cache(maxsize=None)
def _operands(nbytes, fan_in):
    return [reference_wire_operands(nbytes, SEED + k) for k in range(fan_in)]


@functools.lru_cache(maxsize=None)
def _want(nbytes, fmt, fan_in, packed):
    ref = reference_wire_reduce_packed if packed else reference_wire_reduce
    return ref(_operands(nbytes, fan_in), fmt, own_bf16=True)


def _st():
    return int(torch.cuda.current_stream().cuda_stream)


def _sources(native, nbytes, fmt, fan_in):
    """The own shard (fill_wire_operand of stream SEED) and the images of streams SEED + 1.. ."""
    own = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    native.fill_wire_operand(own.data_ptr(), nbytes, SEED, _st())
    images = [torch.empty(native.wire_bytes(nbytes, fmt), dtype=torch.uint8, device="cuda") for _ in range(fan_in - 1)]
    for k, im in enumerate(images):
        native.fill_packed(im.data_ptr(), nbytes, SEED + 1 + k, fmt, _st())
    return [own] + images


def _sum(native, srcs, nbytes, fmt, packed, **kw):
    """The fused kernel's output between 0xAB guards: (dst, guards intact)."""
    size = native.wire_bytes(nbytes, fmt) if packed else nbytes
    whole = torch.full((2 * GUARD + size,), 0xAB, dtype=torch.uint8, device="cuda")
    dst = whole[GUARD:GUARD + size]
    if packed:
        wire_reduce_packed_(dst, srcs, nbytes, fmt, own_bf16=True, **kw)
    else:
        wire_reduce_(dst, srcs, fmt, own_bf16=True, **kw)
    return dst, bool((whole[:GUARD] == 0xAB).all()) and bool((whole[GUARD + size:] == 0xAB).all())


@pytest.mark.parametrize("coherent", [False, True], ids=["local", "peers-coherent"])
@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt,packed", [(f, False) for f in FORMATS] + [(f, True) for f in PACKED])
def test_sum_matches_reference(native, fmt, packed, lanes, coherent):
    for nbytes, fan_in in CASES:
        mask = ((1 << fan_in) - 2) if coherent else 0  # sources 1..K-1; bit 0, the own shard, stays clear
        dst, intact = _sum(native, _sources(native, nbytes, fmt, fan_in), nbytes, fmt, packed, lanes=lanes, coherent=mask)
        assert torch.equal(dst.cpu(), _want(nbytes, fmt, fan_in, packed)) and intact, (nbytes, fan_in)


@pytest.mark.parametrize("fmt,packed", [(f, False) for f in FORMATS] + [(f, True) for f in PACKED])
def test_grid_stride_passes(native, fmt, packed):
    nbytes = 8 * TILE + 192  # 9 tiles over 2 workgroups
    dst, intact = _sum(native, _sources(native, nbytes, fmt, 3), nbytes, fmt, packed, max_blocks=2)
    assert torch.equal(dst.cpu(), _want(nbytes, fmt, 3, packed)) and intact


def test_a_coherent_own_shard_is_refused(native):
    srcs = _sources(native, 64, "mxfp8", 2)
    with pytest.raises(Exception, match="own shard"):
        wire_reduce_(torch.empty(64, dtype=torch.uint8, device="cuda"), srcs, "mxfp8", own_bf16=True, coherent=3)


# own bf16 bits, per incoming operand (mxfp8 code, mxfp6 code, mxfp4 code, scale byte), the bf16 bits due.  1.0 is
# 0x38 / 0x08 / 0x2 under scale byte 127, 2^-8 and 2^-10 the same codes under 119 and 117; the sign is the top code bit.
DIRECTED = {
    "tie-even-stays": (0x3F80, [(0x38, 0x08, 0x2, 119)], 0x3F80),        # 1 + 2^-8: half way, the lower neighbour is even
    "tie-odd-goes-up": (0x3F81, [(0x38, 0x08, 0x2, 119)], 0x3F82),       # (1 + 2^-7) + 2^-8: the lower neighbour is odd
    "below-half-ulp": (0x3F81, [(0x38, 0x08, 0x2, 117)] * 2, 0x3F81),    # + 2^-10 twice: the own value stays
    "cancels-to-plus-zero": (0x3F80, [(0xB8, 0x28, 0xA, 127)], 0x0000),  # 1 + (-1)
}


@pytest.mark.parametrize("lanes", ["split", "contiguous"])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_sums(native, name, fmt, lanes):
    own_bits, incoming, bits = DIRECTED[name]
    srcs = [torch.tensor([own_bits & 0xFF, own_bits >> 8] * 32, dtype=torch.uint8).cuda()]
    for c8, c6, c4, sb in incoming:  # one block: its element bytes, zeros up to 16, the scale byte, zeros up to 16
        v = c6 | c6 << 6 | c6 << 12 | c6 << 18
        elems = {"mxfp8": [c8] * 32, "mxfp6": [v & 0xFF, (v >> 8) & 0xFF, v >> 16] * 8, "mxfp4": [c4 | c4 << 4] * 16}[fmt]
        elems += [0] * (-len(elems) % 16)
        srcs.append(torch.tensor(elems + [sb] + [0] * 15, dtype=torch.uint8).cuda())
    dst = torch.empty(64, dtype=torch.uint8, device="cuda")
    wire_reduce_(dst, srcs, fmt, lanes=lanes, own_bf16=True)
    assert dst.cpu().view(torch.int16).tolist() == [bits - (bits >> 15 << 16)] * 32


@pytest.mark.parametrize("fmt", FORMATS)
def test_two_step_path_agrees(native, fmt):
    """The second oracle: unpack the incoming images to bf16 scratch, then the bf16 reduce kernel over own + scratch."""
    nbytes = 3 * TILE + 192
    srcs = _sources(native, nbytes, fmt, 3)
    scratch = [wire_unpack_(torch.empty(nbytes, dtype=torch.uint8, device="cuda"), im, fmt) for im in srcs[1:]]
    two_step = reduce_(torch.empty(nbytes, dtype=torch.uint8, device="cuda"), [srcs[0]] + scratch, "bf16")
    assert torch.equal(_sum(native, srcs, nbytes, fmt, False)[0], two_step)


@pytest.mark.parametrize("fmt,packed", [(f, False) for f in FORMATS] + [(f, True) for f in PACKED])
def test_verify_names_one_flipped_bit(native, fmt, packed):
    nbytes, seeds = TILE + 64, [SEED + k for k in range(3)]
    dst = _sum(native, _sources(native, nbytes, fmt, 3), nbytes, fmt, packed)[0]
    check = native.verify_wire_reduced_packed if packed else native.verify_wire_reduced
    assert check(dst.data_ptr(), nbytes, seeds, fmt, _st(), own_bf16=True)[::2] == (0, 2**64 - 1)
    assert check(dst.data_ptr(), nbytes, seeds, fmt, _st())[0] > 0  # the all-image sum is another one
    dst[4 * 300 + 3] ^= 0x80
    assert check(dst.data_ptr(), nbytes, seeds, fmt, _st(), own_bf16=True)[::2] == (1, 4 * 300)


def test_fill_wire_operand_is_the_operand_stream(native):
    nbytes = TILE + 64
    own = _sources(native, nbytes, "mxfp8", 1)[0]
    assert torch.equal(own.cpu(), words_to_bytes(_operands(nbytes, 1)[0]))
