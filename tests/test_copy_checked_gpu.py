"""Tier T3: the checked copy kernel (multi_copy_checked_kernel) on one GPU,
in its plain and its cross-GPU (coherent) form on local memory.  It must move
exactly what the plain copy moves -- what it loaded, matched or not -- and
report, per record, the wrong 32-bit words and the first wrong stream byte.

Every expected value comes from PyTorch: reference_copy_check /
reference_words for the findings, torch's own copy for the bytes; never from
another kernel.  The destination sits between 0xAB guard regions that are
compared too.  Nothing depends on the CU count: grids are set with max_blocks
or the result does not depend on the grid.

Notation: U = 4096, one workgroup's chunk; G = max_blocks."""
import functools
import itertools

import pytest
import torch

from test_nccl_p2p_amd.ops import copy_checked_, reference_bytes, reference_copy_check
from test_nccl_p2p_amd.ops.buffers import reference_words

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
SEED = 0xC0FFEE5
WRONG_SEED = SEED + 1
U = 4096
GUARD = 256
RAGGED = 3 * U + 1024 + 16 * 37 + 5

FORMS = [pytest.param(False, id="plain"), pytest.param(True, id="coherent")]


@pytest.fixture(scope="module", autouse=True)
def _gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def stream_bytes(offset, nbytes, seed):
    """Bytes [offset, offset + nbytes) of stream `seed` on the GPU (offset a
    multiple of 4), from reference_words."""
    assert offset % 4 == 0
    w = reference_words(offset // 4, (nbytes + 3) // 4, seed, device="cuda")
    b = torch.stack([(w >> (8 * k)) & 0xFF for k in range(4)], dim=1).to(torch.uint8).reshape(-1)
    return b[:nbytes].contiguous()


@functools.lru_cache(maxsize=None)
def clean(nbytes, seed=SEED, offset=0):
    """A source holding that part of the stream; shared and never written.
    Carved out of a larger buffer so that an empty one still has an address."""
    buf = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    buf[:nbytes] = stream_bytes(offset, nbytes, seed)
    return buf[:nbytes]


def flipped(src, offsets, bit=0x24):
    out = torch.empty(src.numel() + 16, dtype=torch.uint8, device="cuda")[:src.numel()]
    out.copy_(src)
    for off in offsets:
        out[off] ^= bit
    return out


def run_group(native, specs, coherent, max_blocks=0, launches=1):
    """specs: [(src, seed, stream_offset, record)].  Launches the group into
    destinations laid out between guards, checks that every destination equals
    its source and that nothing else was written, and returns the records."""
    total = GUARD + sum((s.numel() + 15) // 16 * 16 + GUARD for s, *_ in specs)
    arena = torch.full((total,), 0xAB, dtype=torch.uint8, device="cuda")
    want = arena.clone()
    ops, off = [], GUARD
    for src, seed, so, rec in specs:
        n = src.numel()
        ops.append((arena.data_ptr() + off, src.data_ptr(), n, seed, so, rec))
        want[off:off + n] = src
        off += (n + 15) // 16 * 16 + GUARD
    got = native.copy_checked(ops, stream(), coherent, max_blocks, accumulate_launches=launches)
    assert torch.equal(arena, want), "the copy moved something other than what it loaded"
    return [tuple(g) for g in got]


def expected(specs):
    """Per distinct record, ascending: the sum of the ops' wrong words and the
    lowest of their first wrong stream bytes (reference_copy_check)."""
    out = {}
    for src, seed, so, rec in specs:
        r = reference_copy_check(src, seed, so)
        m, f = out.get(rec, (0, NONE))
        out[rec] = (m + r.mismatches, min(f, r.first_bad))
    return [out[k] for k in sorted(out)]


# ------------------------------------------------------------------ sizes ----

@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, U - 16, U, U + 16, 2 * U + 5, RAGGED])
@pytest.mark.parametrize("coherent", FORMS)
def test_sizes_clean_and_wrong_seed(native, coherent, nbytes):
    src = clean(nbytes)
    assert run_group(native, [(src, SEED, 0, 0)], coherent) == [(0, NONE)]
    want = expected([(src, WRONG_SEED, 0, 0)])
    assert (want[0][0] > 0) == (nbytes > 0)
    assert run_group(native, [(src, WRONG_SEED, 0, 0)], coherent) == want


@pytest.mark.parametrize("coherent", FORMS)
def test_tensor_entry_point(coherent):
    src = flipped(clean(RAGGED), [U + 3])
    dst = torch.zeros_like(src)
    r = copy_checked_(dst, src, SEED, coherent=coherent)
    assert r == reference_copy_check(src, SEED) == (1, U)
    assert not r.ok and torch.equal(dst, src)


# ------------------------------------------------------------------ flips ----

NVEC = RAGGED // 16
SINGLE_FLIPS = {
    "word0": 1,
    "vec0-word2": 9,
    "last-full-vector": (NVEC - 1) * 16 + 13,
    "tail-partial-word": NVEC * 16 + 4,
    "before-chunk-seam": U - 1,
    "after-chunk-seam": U,
}


@pytest.mark.parametrize("where", list(SINGLE_FLIPS))
@pytest.mark.parametrize("coherent", FORMS)
def test_one_flipped_byte(native, coherent, where):
    off = SINGLE_FLIPS[where]
    spec = [(flipped(clean(RAGGED), [off]), SEED, 0, 0)]
    want = expected(spec)
    assert want == [(1, off // 4 * 4)]
    assert run_group(native, spec, coherent) == want


@pytest.mark.parametrize("coherent", FORMS)
def test_every_subset_of_a_vectors_words(native, coherent):
    vec = 300  # lane 44 of the second chunk
    for r in range(1, 5):
        for words in itertools.combinations(range(4), r):
            spec = [(flipped(clean(RAGGED), [vec * 16 + 4 * w + 2 for w in words]), SEED, 0, 0)]
            want = expected(spec)
            assert want == [(len(words), vec * 16 + 4 * words[0])]
            assert run_group(native, spec, coherent) == want, words


@pytest.mark.parametrize("coherent", FORMS)
def test_all_flips_at_once(native, coherent):
    spec = [(flipped(clean(RAGGED), list(SINGLE_FLIPS.values())), SEED, 0, 0)]
    want = expected(spec)
    assert want == [(6, 0)]
    assert run_group(native, spec, coherent) == want


# ------------------------------------------------------------ grid-stride ----

@pytest.mark.parametrize("size_index", range(4))
@pytest.mark.parametrize("G", [1, 2, 3])
@pytest.mark.parametrize("coherent", FORMS)
def test_grid_stride(native, coherent, G, size_index):
    """G workgroups walk one to three passes: ends exactly on a pass, one
    vector into the next, one vector short of two, and a ragged third pass;
    then a flip in the last pass (and in the tail where there is one)."""
    P = G * U
    nbytes = [P, P + 16, 2 * P - 16, 2 * P + 1024 + 16 * 37 + 5][size_index]
    src = clean(nbytes)
    assert run_group(native, [(src, SEED, 0, 0)], coherent, max_blocks=G) == [(0, NONE)]
    last_pass = (nbytes - 1) // P * P
    flips = sorted({last_pass + 7, nbytes - 1})
    spec = [(flipped(src, flips), SEED, 0, 0)]
    want = expected(spec)
    assert want == [(len({f // 4 for f in flips}), last_pass + 4)]
    assert run_group(native, spec, coherent, max_blocks=G) == want
    assert run_group(native, [(src, WRONG_SEED, 0, 0)], coherent, max_blocks=G) == expected([(src, WRONG_SEED, 0, 0)])


# -------------------------------------------------------------------- ops ----

@pytest.mark.parametrize("G", [0, 5])
@pytest.mark.parametrize("coherent", FORMS)
def test_three_unequal_ops(native, coherent, G):
    """Unequal block counts: the binary-search lookup (under a cap too).  Each
    op its own seed and record; flips in the middle one only."""
    sizes = [U + 16, 3 * U + 5, 2 * U]
    spec = [(clean(n, SEED + i), SEED + i, 0, i) for i, n in enumerate(sizes)]
    assert run_group(native, spec, coherent, max_blocks=G) == [(0, NONE)] * 3
    spec[1] = (flipped(spec[1][0], [2 * U + 33, 3 * U + 4]), SEED + 1, 0, 1)
    want = expected(spec)
    assert want == [(0, NONE), (2, 2 * U + 32), (0, NONE)]
    assert run_group(native, spec, coherent, max_blocks=G) == want


@pytest.mark.parametrize("coherent", FORMS)
def test_four_equal_ops(native, coherent):
    """Equal block counts: the one-division lookup."""
    spec = [(clean(2 * U, SEED + i), SEED + i, 0, i) for i in range(4)]
    assert run_group(native, spec, coherent) == [(0, NONE)] * 4
    spec[2] = (flipped(spec[2][0], [U + 5]), SEED + 2, 0, 2)
    spec[3] = (spec[3][0], SEED, 0, 3)  # the whole op against another op's stream
    want = expected(spec)
    assert want[:3] == [(0, NONE), (0, NONE), (1, U + 4)] and want[3][0] > 2000
    assert run_group(native, spec, coherent) == want


@pytest.mark.parametrize("coherent", FORMS)
def test_35_ops_more_than_one_launch(native, coherent):
    """35 ops, one record each, go out as launches of 32 and 3: flips in ops
    0, 31, 32 and 34 show up in those records and in no other."""
    spec = [(clean(U + 16 * i + (i % 7), SEED + i), SEED + i, 0, i) for i in range(35)]
    for i in (0, 31, 32, 34):
        spec[i] = (flipped(spec[i][0], [spec[i][0].numel() - 1]), SEED + i, 0, i)
    want = expected(spec)
    assert [i for i, w in enumerate(want) if w[0]] == [0, 31, 32, 34]
    assert run_group(native, spec, coherent) == want


@pytest.mark.parametrize("coherent", FORMS)
def test_two_ops_on_one_record(native, coherent):
    """Two pieces of one message (the second from stream byte 2U on) share a
    record: it holds the sum of their wrong words and the lower first byte,
    in stream bytes."""
    a = flipped(clean(2 * U), [U + 9])
    b = flipped(clean(2 * U + 5, SEED, 2 * U), [3, 2 * U + 4])
    spec = [(b, SEED, 2 * U, 0), (a, SEED, 0, 0)]
    want = expected(spec)
    assert want == [(3, U + 8)]
    assert run_group(native, spec, coherent) == want
    assert run_group(native, [(b, SEED, 2 * U, 0)], coherent) == [(2, 2 * U)]


@pytest.mark.parametrize("coherent", FORMS)
def test_records_accumulate_until_reset(native, coherent):
    spec = [(flipped(clean(RAGGED), [5, U + 1, RAGGED - 1]), SEED, 0, 0)]
    once = expected(spec)
    assert once == [(3, 4)]
    assert run_group(native, spec, coherent, launches=2) == [(6, 4)]
    assert run_group(native, spec, coherent) == once  # a new call resets first


# --------------------------------------------------------------- key seam ----

SEAM = 2**34  # stream byte of word 2**32, where the PRNG key changes


@pytest.mark.parametrize("coherent", FORMS)
def test_key_seam(native, coherent):
    """3U + 5 bytes of the stream from 2**34 - U on: the key changes one chunk
    in.  Clean, then a flip either side of the seam; first_bad is in stream
    bytes."""
    so, n = SEAM - U, 3 * U + 5
    src = clean(n, SEED, so)
    lo = reference_words(SEAM // 4 - 2, 4, SEED)
    assert not torch.equal(lo[2:], reference_words(0, 2, SEED))  # the stream does not simply wrap there
    assert run_group(native, [(src, SEED, so, 0)], coherent) == [(0, NONE)]
    for off, first in ((U - 1, SEAM - 4), (U, SEAM)):
        spec = [(flipped(src, [off]), SEED, so, 0)]
        want = expected(spec)
        assert want == [(1, first)]
        assert run_group(native, spec, coherent) == want
    # The same bytes against the stream one key span later: every word is wrong.
    wrong = expected([(src, SEED, so + SEAM, 0)])
    assert wrong == [((n + 3) // 4, so + SEAM)]
    assert run_group(native, [(src, SEED, so + SEAM, 0)], coherent) == wrong


# ------------------------------------------------------------ offset rule ----

def test_unaligned_stream_offset_is_an_error_not_a_launch(native):
    src = clean(U)
    dst = torch.full((U,), 0xAB, dtype=torch.uint8, device="cuda")
    for so in (16, 2048, U + 4):
        with pytest.raises(ValueError, match="4096"):
            native.copy_checked([(dst.data_ptr(), src.data_ptr(), U, SEED, so, 0)], stream())
        with pytest.raises(ValueError, match="4096"):
            native.copy_checked_launch([(dst.data_ptr(), src.data_ptr(), U, SEED, so, 0)], stream())
    torch.cuda.synchronize()
    assert torch.all(dst == 0xAB)


def test_launch_only_entry_point_moves_the_bytes(native):
    src = clean(RAGGED)
    dst = torch.full((RAGGED + GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    native.copy_checked_launch([(dst.data_ptr(), src.data_ptr(), RAGGED, SEED, 0, 0)], stream())
    torch.cuda.synchronize()
    assert torch.equal(dst[:RAGGED], src) and torch.all(dst[RAGGED:] == 0xAB)


# --------------------------------------------------------------- property ----

try:
    from hypothesis import HealthCheck, given, settings, strategies as st
except ImportError:  # the example-based tests above still run
    def test_random_groups_match_reference():
        pytest.importorskip("hypothesis")
else:
    @st.composite
    def op_groups(draw):
        """1..40 ops of 0..48 KiB at any 4 KiB-aligned stream offset (some
        across the key seam), a few records shared between them, up to 3
        corrupt bytes each, either form, a full grid or a cap."""
        n = draw(st.integers(1, 40))
        ops = []
        for _ in range(n):
            nbytes = draw(st.integers(0, 48 << 10))
            so = draw(st.one_of(st.integers(0, 1 << 24), st.integers((SEAM >> 12) - 12, (SEAM >> 12) + 1))) << 12
            flips = draw(st.lists(st.integers(0, max(nbytes - 1, 0)), max_size=3, unique=True)) if nbytes else []
            ops.append((nbytes, draw(st.integers(0, (1 << 64) - 1)), so, draw(st.integers(0, 5)), flips,
                        draw(st.booleans())))
        return ops, draw(st.booleans()), draw(st.sampled_from([0, 0, 1, 3, 7]))

    @settings(max_examples=40, deadline=None, suppress_health_check=[HealthCheck.function_scoped_fixture])
    @given(op_groups())
    def test_random_groups_match_reference(native, group):
        ops, coherent, G = group
        spec = []
        for nbytes, seed, so, rec, flips, wrong_seed in ops:
            src = flipped(stream_bytes(so, nbytes, seed), flips, bit=0x5A)
            spec.append((src, seed ^ 1 if wrong_seed else seed, so, rec))
        assert run_group(native, spec, coherent, max_blocks=G) == expected(spec)
