"""Tier T3, the loops and dispatches the other kernel tests never re-enter:
the verify kernels' grid-stride passes (a capped grid on small buffers), the
LDS-staged kernel's ragged last chunk after its pipeline has wrapped, both
LDS templates at any size, the copy kernel's grid-stride loops and the
proportional block split under a grid cap, the 4 GiB seams of fill and copy,
empty and sub-vector buffers, and every subset of bad words in one vector.

Every expected value comes from the PyTorch reference of the same operation
(reference_bytes / reference_words / reference_verify, torch's copy_), never
from another kernel; the payloads are integers, so every comparison is exact.
Nothing here depends on the CU count: the grids are set with max_grid /
max_blocks, or the result does not depend on the grid.

Notation: U = bytes one workgroup consumes per pass (stride 16 KiB; lds8 with
4 stages 16 KiB, with 8 stages 32 KiB), G = max_grid, P = G * U."""
import functools
import itertools

import pytest
import torch

from test_nccl_p2p_amd.ops import checksum, reference_bytes, reference_verify, verify
from test_nccl_p2p_amd.ops.buffers import reference_words

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
SEED = 0x5EED5
WRONG_SEED = SEED + 1
GIB = 1 << 30

# (id, impl, lds_stages, U)
KERNELS = [
    pytest.param("stride", 0, 16 << 10, id="stride"),
    pytest.param("lds8", 4, 16 << 10, id="lds4"),
    pytest.param("lds8", 8, 32 << 10, id="lds8"),
]
GRIDS = [1, 2, 3]


@pytest.fixture(scope="module", autouse=True)
def _gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def ragged_size(P):
    """Two full passes, then a last wave chunk of one full 1 KiB stage, 37
    vectors of the next stage and a 5-byte tail."""
    return 2 * P + 1024 + 16 * 37 + 5


def pass_sizes(P, U):
    return [P, P + 16, 2 * P - 16, ragged_size(P), 4 * P + U // 4 + 16]


@functools.lru_cache(maxsize=None)
def clean(nbytes):
    """(buffer holding stream SEED, its reference result, the reference result
    against WRONG_SEED); shared by the tests and never written."""
    buf = reference_bytes(nbytes, SEED, device="cuda")
    return buf, reference_verify(buf, SEED), reference_verify(buf, WRONG_SEED)


# ------------------------------------------------- 1. multi-pass verify ----

@pytest.mark.parametrize("size_index", range(5))
@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("check", [True, False], ids=["verify", "checksum"])
@pytest.mark.parametrize("impl,stages,U", KERNELS)
def test_multi_pass_verify(impl, stages, U, check, G, size_index):
    """A grid of G workgroups walks buffers of one to five passes: ends exactly
    on a pass, one vector into the next, one vector short of two, a ragged
    third pass, and one vector into a later wave's chunk."""
    nbytes = pass_sizes(G * U, U)[size_index]
    buf, ref, ref_wrong = clean(nbytes)
    assert ref.mismatches == 0 and ref.first_bad == NONE
    if not check:
        assert checksum(buf, impl=impl, max_grid=G, lds_stages=stages) == ref.checksum
        return
    r = verify(buf, SEED, impl=impl, max_grid=G, lds_stages=stages)
    assert r == (0, ref.checksum, NONE)
    wrong = verify(buf, WRONG_SEED, impl=impl, max_grid=G, lds_stages=stages)
    assert ref_wrong.mismatches > 0
    assert wrong == ref_wrong


# --------------------------------------------------- 2. stale-slot probe ----

@pytest.mark.parametrize("G", GRIDS)
@pytest.mark.parametrize("impl,stages,U", KERNELS)
def test_ragged_last_chunk_after_wrap(impl, stages, U, G):
    """The last chunk fills one stage and 37 lanes of the next, in slots that
    still hold the chunk of the pass before.  Bad bytes in the last full
    vector, in the tail, in word 2 of vector 0 and, one pass earlier, at a
    stage and lane the last chunk does not fill: a masked-out lane that is
    counted is one mismatch too many, one that is summed a wrong checksum."""
    P = G * U
    nbytes = ragged_size(P)
    nvec = nbytes // 16
    buf = clean(nbytes)[0].clone()
    flips = [(nvec - 1) * 16 + 13, nvec * 16 + 2, 8 + 1, 2 * P - P + 2 * 1024 + 16 * 50 + 6]
    for off in flips:
        buf[off] ^= 0x24
    ref = reference_verify(buf, SEED)
    assert ref.mismatches == 4 and ref.first_bad == 8
    assert verify(buf, SEED, impl=impl, max_grid=G, lds_stages=stages) == ref
    assert checksum(buf, impl=impl, max_grid=G, lds_stages=stages) == ref.checksum


# ------------------------------------------------ 3. production dispatch ----

def test_geometry_dispatch(native):
    """What a production launch picks, without launching anything large: 4
    stages (16 KiB of LDS) below 2 GiB, 8 (32 KiB) from there; lds_stages
    overrides either way; max_grid caps the grid."""
    below, at = 2 * GIB - 16, 2 * GIB
    assert native.verify_geometry(below, 1)[1:] == (256, 16 << 10)
    assert native.verify_geometry(at, 1)[1:] == (256, 32 << 10)
    assert native.verify_geometry(at, 0)[2] == 32 << 10  # auto = lds8
    for nbytes in (below, at):
        assert native.verify_geometry(nbytes, 1, lds_stages=4)[2] == 16 << 10
        assert native.verify_geometry(nbytes, 1, lds_stages=8)[2] == 32 << 10
        assert native.verify_geometry(nbytes, 2)[2] == 0
        assert native.verify_geometry(nbytes, 2, lds_stages=8)[2] == 0
        for impl, stages in ((1, 0), (1, 4), (1, 8), (2, 0)):
            assert 1 <= native.verify_geometry(nbytes, impl, max_grid=5, lds_stages=stages)[0] <= 5
    # Small buffers: one workgroup per U bytes up to the cap.
    for impl, stages, U in ((2, 0, 16 << 10), (1, 4, 16 << 10), (1, 8, 32 << 10)):
        for G in GRIDS:
            assert native.verify_geometry(4 * G * U, impl, max_grid=G, lds_stages=stages)[0] == G
        assert native.verify_geometry(2 * U + 16, impl, max_grid=8, lds_stages=stages)[0] == 3
        assert native.verify_geometry(0, impl, max_grid=8, lds_stages=stages)[0] == 1
    buf = clean(4096)[0]
    for bad in (1, 5, 16, -4):
        with pytest.raises(ValueError, match="lds_stages"):
            native.verify_geometry(4096, 1, lds_stages=bad)
        with pytest.raises(ValueError, match="lds_stages"):
            native.verify(buf.data_ptr(), 4096, SEED, 1, True, stream(), lds_stages=bad)
        with pytest.raises(ValueError, match="lds_stages"):
            native.verify_launch(buf.data_ptr(), 4096, SEED, 1, True, stream(), lds_stages=bad)
        with pytest.raises(ValueError, match="lds_stages"):
            verify(buf, SEED, impl="lds8", lds_stages=bad)


# ---------------------------------------------------- 4. per-vector words ----

@pytest.mark.parametrize("impl,stages,U", KERNELS)
def test_every_subset_of_bad_words_in_one_vector(impl, stages, U):
    """One byte flipped in each word of a subset of a vector's four words:
    the count is the subset's size and first_bad its lowest word."""
    nbytes = 4096 + 7
    vec = 64 + 6  # second wave of the register kernel, second stage of the LDS kernels
    base = clean(nbytes)[0]
    for k in range(1, 5):
        for subset in itertools.combinations(range(4), k):
            buf = base.clone()
            for w in subset:
                buf[vec * 16 + 4 * w + (w + 1) % 4] ^= 0x81
            ref = reference_verify(buf, SEED)
            assert (ref.mismatches, ref.first_bad) == (len(subset), vec * 16 + 4 * subset[0])
            r = verify(buf, SEED, impl=impl, lds_stages=stages)
            assert r == ref, (subset, r, ref)


# ----------------------------------------------- 5. tiny and empty buffers ----

@pytest.mark.parametrize("impl", ["lds8", "stride"])
@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 5, 15, 17, 31])
def test_tiny_buffers_and_the_byte_past_the_end(impl, nbytes):
    """Below one vector only the tail runs (0 bytes: nothing does).  The last
    byte inside the buffer counts; the byte just past it does not, neither in
    the masked compare nor in the checksum."""
    store = torch.full((nbytes + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    store[:nbytes] = reference_bytes(nbytes, SEED, device="cuda")
    buf = store[:nbytes]
    ref = reference_verify(buf, SEED) if nbytes else (0, 0, NONE)
    assert tuple(ref)[::2] == (0, NONE)
    assert verify(buf, SEED, impl=impl) == tuple(ref)
    assert checksum(buf, impl=impl) == ref[1]
    if nbytes:
        store[nbytes - 1] ^= 0x08
        bad = reference_verify(buf, SEED)
        assert (bad.mismatches, bad.first_bad) == (1, (nbytes - 1) // 4 * 4)
        assert verify(buf, SEED, impl=impl) == bad
        assert checksum(buf, impl=impl) == bad.checksum
        store[nbytes - 1] ^= 0x08
    store[nbytes] = 0x54  # first guard byte; the buffer itself is intact again
    assert verify(buf, SEED, impl=impl) == tuple(ref)
    assert checksum(buf, impl=impl) == ref[1]


# ------------------------------------------------ 6. copy under a grid cap ----

SRC_BYTES = 256 << 10
RAGGED_COPY = 4096 * 5 + 1008 + 3  # six 4 KiB passes of one block, the last with 63 vectors, then a 3-byte tail


@functools.lru_cache(maxsize=None)
def copy_source():
    g = torch.Generator(device="cuda").manual_seed(7)
    return torch.randint(0, 256, (SRC_BYTES,), dtype=torch.uint8, device="cuda", generator=g)


def check_copy(native, sizes, coherent, max_blocks, single=False):
    """Copies ops of `sizes` into one 0xAB arena, 64 guard bytes before and
    after each destination, and compares the whole arena with the one torch's
    own copies give."""
    src = copy_source()
    offs, off = [], 64
    for n in sizes:
        offs.append(off)
        off = (off + n + 15) // 16 * 16 + 64
    dst = torch.full((off,), 0xAB, dtype=torch.uint8, device="cuda")
    want = dst.clone()
    ops = []
    for i, (n, o) in enumerate(zip(sizes, offs)):
        so = (i * 1237) % ((SRC_BYTES - n) // 16 + 1) * 16
        want[o:o + n].copy_(src[so:so + n])
        ops.append((dst.data_ptr() + o, src.data_ptr() + so, n))
    if single:
        (d, s, n), = ops
        native.copy(d, s, n, stream(), max_blocks=max_blocks, coherent=coherent)
    else:
        native.copy_many(ops, stream(), coherent, max_blocks=max_blocks)
    torch.cuda.synchronize()
    assert torch.equal(dst, want)


@pytest.mark.parametrize("coherent", [False, True], ids=["plain", "coherent"])
@pytest.mark.parametrize("max_blocks", [1, 2, 3])
@pytest.mark.parametrize("nbytes", [16, RAGGED_COPY, 4096 * 7])
def test_copy_under_grid_cap(native, nbytes, max_blocks, coherent):
    """One op on 1 to 3 workgroups: up to seven grid-stride passes, passes
    that end before, on and after the op's last block."""
    check_copy(native, [nbytes], coherent, max_blocks, single=True)


@pytest.mark.parametrize("coherent", [False, True], ids=["plain", "coherent"])
@pytest.mark.parametrize("max_blocks", [2, 0], ids=["cap2", "uncapped"])
def test_copy_many_one_block_per_op(native, max_blocks, coherent):
    """Three ops under a cap of 2: each keeps one block, so op 0 takes six
    passes.  Uncapped, the same ops are the control (one pass each)."""
    check_copy(native, [RAGGED_COPY, 16, 8192], coherent, max_blocks)


@pytest.mark.parametrize("coherent", [False, True], ids=["plain", "coherent"])
def test_copy_many_proportional_shares(native, coherent):
    """40 ops under a cap of 7: two launches (32 + 8 ops).  In the first, two
    40-block ops among 30 one-block ops get 40 * 7 / 110 = 2 blocks each; in
    the second a 40-block op gets 40 * 7 / 59 = 4 and a 13-block op with a
    ragged end 13 * 7 / 59 = 1; every other op, the empty ones included, 1."""
    small = [0, 16, 4099, 1008 + 3, 48, 4096, 1000, 3]
    sizes = [small[i % len(small)] for i in range(40)]
    sizes[3] = sizes[17] = sizes[33] = 4096 * 40
    sizes[36] = 4096 * 12 + 1008 + 3
    check_copy(native, sizes, coherent, 7)


# ----------------------------------------------------- 7. the 4 GiB seams ----

BIG = 4 * GIB + (12 << 10) + 1008 + 5
BIG_SEED = 0xB16
SLICE_WORDS = 1 << 26


class Big:
    """`ref`: BIG bytes of stream BIG_SEED from the PyTorch reference, built in
    slices of 2**26 words, with its checksum; never written.  `work`: BIG
    bytes plus a 64-byte guard for the kernels to write."""

    def __init__(self):
        assert BIG % 4 == 1  # the last word is one byte: masked in the compare, alone in the checksum
        nwords = (BIG + 3) // 4
        store = torch.empty(nwords * 4, dtype=torch.uint8, device="cuda")
        words = store.view(torch.int32)
        total = 0
        for start in range(0, nwords, SLICE_WORDS):
            count = min(SLICE_WORDS, nwords - start)
            w = reference_words(start, count, BIG_SEED, device="cuda")
            if start + count == nwords:
                total += int(w[:-1].sum().item()) + (int(w[-1].item()) & ((1 << (8 * (BIG % 4))) - 1))
            else:
                total += int(w.sum().item())
            words[start:start + count] = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32)
            del w
        self.ref = store[:BIG]
        self.checksum = total % 2**64
        self.work = torch.empty(BIG + 64, dtype=torch.uint8, device="cuda")

    def word(self, t, index):
        """32-bit word `index` of tensor t (bytes past its end read as 0)."""
        b = t[4 * index:4 * index + 4].tolist()
        return sum(v << (8 * k) for k, v in enumerate(b))


@pytest.fixture(scope="module")
def big():
    b = Big()
    yield b
    del b.ref, b.work
    torch.cuda.empty_cache()


def equal_sliced(a, b, step=GIB):
    """torch.equal in pieces (its temporaries stay at one piece's size)."""
    assert a.numel() == b.numel()
    return all(torch.equal(a[i:i + step], b[i:i + step]) for i in range(0, a.numel(), step))


def all_guard(t, step=GIB):
    return all(bool(torch.all(t[i:i + step] == 0xAB)) for i in range(0, t.numel(), step))


def test_big_reference_is_the_stream(big):
    """The sliced reference buffer against reference_bytes / reference_words
    at its start, across the 4 GiB seam and at its masked end."""
    assert torch.equal(big.ref[:4099], reference_bytes(4099, BIG_SEED, device="cuda"))
    w0 = GIB - 8
    got = big.ref[4 * w0:4 * (w0 + 16)].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, reference_words(w0, 16, BIG_SEED, device="cuda"))
    last = int(reference_words(BIG // 4, 1, BIG_SEED).item())
    assert big.word(big.ref, BIG // 4) == last & 0xFF


@pytest.mark.parametrize("nbytes", [4 * GIB + 16 + 5, BIG], ids=["4GiB+21", "full"])
def test_fill_across_4gib(native, big, nbytes):
    """launch_fill's second grid (begin = 4 GiB): a single vector plus tail,
    and 12 KiB + 63 vectors plus tail."""
    big.work.fill_(0xAB)
    native.fill(big.work.data_ptr(), nbytes, BIG_SEED, stream())
    torch.cuda.synchronize()
    assert equal_sliced(big.work[:nbytes], big.ref[:nbytes])
    # The last whole words and the partial one once more, straight from reference_words.
    nwords = nbytes // 4
    got = big.work[4 * (nwords - 8):4 * nwords].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert torch.equal(got, reference_words(nwords - 8, 8, BIG_SEED, device="cuda"))
    last = int(reference_words(nwords, 1, BIG_SEED).item())
    assert big.work[4 * nwords:nbytes].tolist() == [(last >> (8 * k)) & 0xFF for k in range(nbytes % 4)]
    assert all_guard(big.work[nbytes:]), "fill wrote past the end"


@pytest.mark.parametrize("check", [True, False], ids=["verify", "checksum"])
@pytest.mark.parametrize("impl", ["stride", "lds8"])
def test_verify_across_4gib(native, big, impl, check):
    """Both kernels over 4 GiB and a ragged rest (lds8 takes its 8-stage
    template by itself here): the sliced reference's checksum on the clean
    buffer, then a bad byte just past 4 GiB and one in the masked last word."""
    if impl == "lds8":
        assert native.verify_geometry(BIG, 1)[2] == 32 << 10
    work = big.work[:BIG]
    work.copy_(big.ref)
    if check:
        assert verify(work, BIG_SEED, impl=impl) == (0, big.checksum, NONE)
    else:
        assert checksum(work, impl=impl) == big.checksum
    flips = [4 * GIB + 100, BIG - 1]
    want_sum = big.checksum
    for off in flips:
        want_sum -= big.word(work, off // 4)
        work[off] ^= 0x10
        want_sum += big.word(work, off // 4)
    want_sum %= 2**64
    if check:
        assert verify(work, BIG_SEED, impl=impl) == (2, want_sum, (4 * GIB + 100) // 4 * 4)
    else:
        assert checksum(work, impl=impl) == want_sum


@pytest.mark.parametrize("coherent", [False, True], ids=["plain", "coherent"])
@pytest.mark.parametrize("nbytes", [4 * GIB + 5, BIG], ids=["4GiB+5", "full"])
def test_copy_across_4gib(native, big, nbytes, coherent):
    """launch_multi_copy cuts an op above 4 GiB into pieces: a second piece
    that is a tail only (no vector), and one of 12 KiB + 63 vectors + tail."""
    big.work.fill_(0xAB)
    native.copy(big.work.data_ptr(), big.ref.data_ptr(), nbytes, stream(), coherent=coherent)
    torch.cuda.synchronize()
    assert equal_sliced(big.work[:nbytes], big.ref[:nbytes])
    assert all_guard(big.work[nbytes:]), "copy wrote past the end"


@pytest.mark.parametrize("coherent", [False, True], ids=["plain", "coherent"])
def test_copy_many_across_4gib(native, big, coherent):
    """The pieces of a split op packed into launches with a small op behind
    them."""
    big.work.fill_(0xAB)
    small = torch.full((4099 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    src_off = 4 * GIB - 2048
    native.copy_many([(big.work.data_ptr(), big.ref.data_ptr(), BIG),
                      (small.data_ptr(), big.ref.data_ptr() + src_off, 4099)], stream(), coherent)
    torch.cuda.synchronize()
    assert equal_sliced(big.work[:BIG], big.ref)
    assert all_guard(big.work[BIG:]), "copy wrote past the end"
    assert torch.equal(small[:4099], big.ref[src_off:src_off + 4099])
    assert bool(torch.all(small[4099:] == 0xAB)), "copy wrote past the end"
