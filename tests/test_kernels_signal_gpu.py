"""The two one-wave kernels of csrc/pingpong.hip, driven directly on one GPU:
pingpong_kernel (the device-initiated ping-pong and the ring token chain) and
signal_kernel (the push engine's ready / done rendezvous and the StreamGate).

Every expected value comes from a plain Python model of the protocol (Wave,
run_waves, model_signal below), never from another kernel run.  The model is
integers and bytes, so every comparison is exact.

All memory a kernel may write lies between 0xAB guard bytes, and each test
compares the whole arena with the model's, guards included.  The arena is once
a torch uint8 tensor (plain hipMalloc, the transports' fallback) and once a
native.signal_page (what the transports use); flags the host writes while a
kernel runs, and every flag a kernel may be left waiting on, are lines of
native.HostWords.  Slots are laid out as in production: flag at offset 0,
payload at offset 256; signal flags on 128-byte lines.

Sections: A one wave against a pre-set inbox (nothing spins), B two waves of
one workgroup handing off for real, C signal kernels with nothing left
waiting, D signal kernels the host releases, E deadlines.  Every wait in D and
E is bounded twice: by the kernel's own deadline and by the host storing the
awaited value whatever the test saw.

Nothing here depends on the CU count, on a second GPU or on a second process.
"""
import struct
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 0xAB
GUARD64 = 0xABABABABABABABAB
HEADER = 256  # payload offset in a slot (transport_ipc.cpp kPingHeader)
LINE = 128    # one signal flag per line (transport_ipc.cpp kSyncLine)
HOST = 1 << 48  # model addresses from here on are HostWords lines, 64 bytes apart
SPARE_STAMPS = 4  # guard entries behind stamps[iters]
MAX_SIGNALS = 16

MEMORY = ["tensor", "page"]
PING_POINTERS = ("out_flag", "out_payload", "in_flag", "in_payload", "stamps", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def hz(native):
    rate = native.wall_clock_hz()
    assert rate > 0
    return rate


def null_stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------- memory and model ----

class Layout:
    """Named regions of an arena, each 256-byte aligned with at least 256
    guard bytes on either side."""

    def __init__(self):
        self.regions = []
        self.size = 256

    def add(self, name, nbytes):
        off = (self.size + 255) // 256 * 256
        self.regions.append((name, off, nbytes))
        self.size = off + nbytes + 256
        return off

    def where(self, off):
        for name, start, nbytes in self.regions:
            if start <= off < start + nbytes:
                return "%s + %d" % (name, off - start)
        return "guard"


class Mem:
    """What the model reads and writes: the arena's bytes and the first 8
    bytes of each HostWords line.  Addresses are arena offsets, or HOST +
    64 * line."""

    def __init__(self, layout, nwords=0):
        self.layout = layout
        self.img = bytearray([GUARD]) * ((layout.size + 255) // 256 * 256)
        self.words = [0] * nwords

    @staticmethod
    def word(line):
        return HOST + 64 * line

    def get64(self, addr):
        if addr >= HOST:
            return self.words[(addr - HOST) // 64]
        return struct.unpack_from("<Q", self.img, addr)[0]

    def put64(self, addr, v):
        if addr >= HOST:
            self.words[(addr - HOST) // 64] = v
        else:
            struct.pack_into("<Q", self.img, addr, v)

    def get32(self, addr):
        if addr >= HOST:
            return self.words[(addr - HOST) // 64] & 0xFFFFFFFF
        return struct.unpack_from("<I", self.img, addr)[0]

    def put32(self, addr, v):
        if addr >= HOST:
            i = (addr - HOST) // 64
            self.words[i] = (self.words[i] & ~0xFFFFFFFF) | v
        else:
            struct.pack_into("<I", self.img, addr, v)


class Device:
    """The device's copy of a Mem as it stands now: the arena in memory of one
    kind, the words in HostWords."""

    def __init__(self, native, kind, mem):
        self.native = native
        self.n = len(mem.img)
        self.stage = torch.frombuffer(bytearray(mem.img), dtype=torch.uint8).cuda()
        self.page = None
        if kind == "page":
            self.page = native.signal_page(self.n)
            assert self.page.bytes == self.n and self.page.ptr % 256 == 0
            native.copy(self.page.ptr, self.stage.data_ptr(), self.n, null_stream())
        self.base = self.page.ptr if self.page else self.stage.data_ptr()
        self.hw = native.HostWords(len(mem.words)) if mem.words else None
        for i, v in enumerate(mem.words):
            self.hw.store(i, v)
        torch.cuda.synchronize()

    def ptr(self, addr):
        if addr >= HOST:
            return self.hw.ptr((addr - HOST) // 64)
        assert 0 <= addr < self.n
        return self.base + addr

    def store(self, addr, v):
        assert addr >= HOST
        self.hw.store((addr - HOST) // 64, v)

    def read(self):
        """(arena bytes, words) once everything launched has finished."""
        torch.cuda.synchronize()
        back = self.stage
        if self.page:
            back = torch.empty_like(self.stage)
            self.native.copy(back.data_ptr(), self.page.ptr, self.n, null_stream())
            torch.cuda.synchronize()
        words = [self.hw.load(i) for i in range(len(self.hw))] if self.hw else []
        return bytearray(back.cpu().numpy().tobytes()), words


def assert_same(got, mem):
    """The arena byte for byte, and the words, against the model's."""
    img, words = got
    if bytes(img) != bytes(mem.img):
        diff = [i for i in range(len(mem.img)) if img[i] != mem.img[i]]
        pytest.fail("%d bytes differ from the model, the first at %d (%s): 0x%02x, the model says 0x%02x; u64 there "
                    "0x%x, the model 0x%x" % (len(diff), diff[0], mem.layout.where(diff[0]), img[diff[0]],
                                              mem.img[diff[0]],
                                              struct.unpack_from("<Q", img, diff[0] // 8 * 8)[0],
                                              struct.unpack_from("<Q", mem.img, diff[0] // 8 * 8)[0]))
    assert words == mem.words


class Wave:
    """One wave of pingpong_kernel on a Mem.  Stamps are counted, not written
    (their values are the device's clock): `stamped` entries, from 0."""

    def __init__(self, mem, role):
        self.mem, self.r = mem, role
        self.i = 0
        self.sent = False
        self.done = False
        self.stamped = 1 if role["leader"] else 0

    def send(self, seq):
        r = self.r
        for off in range(0, r["bytes"], 8):
            self.mem.put64(r["out_payload"] + off, seq)
        self.mem.put64(r["out_flag"], seq)

    def check(self, want):
        # Lane 0 reads the first vector, lane 1 the last; each counts its own.
        r = self.r
        bad = 0
        for off in (0, r["bytes"] - 16):
            x = self.mem.get64(r["in_payload"] + off)
            y = self.mem.get64(r["in_payload"] + off + 8)
            bad += x != want or y != want
        self.mem.put32(r["status"] + 4, self.mem.get32(r["status"] + 4) + bad)

    def step(self):
        """Runs until the wave is done or must wait; True if it got anywhere."""
        r = self.r
        moved = False
        while not self.done:
            if self.i == r["iters"]:
                self.done = True
                break
            seq, want = r["base"] + self.i + 1, r["in_base"] + self.i + 1
            if r["leader"] and not self.sent:
                self.send(seq)
                self.sent = moved = True
            if self.mem.get64(r["in_flag"]) < want:
                break
            self.check(want)
            if r["leader"]:
                self.stamped += 1
            else:
                self.send(seq)
            self.i += 1
            self.sent = False
            moved = True
        return moved

    def expire(self):
        self.mem.put32(self.r["status"], self.mem.get32(self.r["status"]) | 1)
        self.done = True


def run_waves(mem, roles):
    """The waves of one launch to their end; a wave nobody will ever answer
    leaves at its deadline.  Returns the stamp count of each."""
    waves = [Wave(mem, r) for r in roles]
    while not all(w.done for w in waves):
        if not any([w.step() for w in waves]):
            for w in waves:
                if not w.done:
                    w.expire()
    return [w.stamped for w in waves]


def model_signal(mem, posts, waits, status):
    """signal_kernel with nobody else writing: posts, then every wait either
    holds already or runs into the deadline."""
    for flag, value in posts:
        mem.put64(flag, value)
    expired = any(mem.get64(flag) < value for flag, value in waits)
    if expired:
        mem.put32(status, mem.get32(status) | 1)
    return expired


def ping_memory(nbytes, iters, nwords=0):
    lay = Layout()
    slots = [lay.add("slot 0", HEADER + nbytes), lay.add("slot 1", HEADER + nbytes)]
    stamps = lay.add("stamps", 8 * (iters + 1 + SPARE_STAMPS))
    status = lay.add("status", 8)
    mem = Mem(lay, nwords)
    mem.put32(status, 0)
    mem.put32(status + 4, 0)
    return mem, slots, stamps, status


def ping_role(slots, stamps, status, nbytes, iters, leader, base, in_base, ticks, out=0):
    """Writes slot `out`, reads the other one."""
    return {"out_flag": slots[out], "out_payload": slots[out] + HEADER,
            "in_flag": slots[1 - out], "in_payload": slots[1 - out] + HEADER,
            "bytes": nbytes, "base": base, "in_base": in_base, "iters": iters, "leader": leader,
            "stamps": stamps, "status": status, "timeout_ticks": ticks}


def fill_payload(mem, slot, nbytes, value):
    for off in range(0, nbytes, 8):
        mem.put64(slot + HEADER + off, value)


def on_device(dev, role):
    return {k: dev.ptr(v) if k in PING_POINTERS else v for k, v in role.items()}


def take_stamps(img, stamps, iters, written):
    """The stamps the kernel wrote: exactly `written` entries, non-decreasing,
    the rest still guard.  Puts the guard back so the arena can be compared
    with the model, which has no clock."""
    total = iters + 1 + SPARE_STAMPS
    vals = list(struct.unpack_from("<%dQ" % total, img, stamps))
    assert vals[written:] == [GUARD64] * (total - written), "a stamp past entry %d was written" % (written - 1)
    got = vals[:written]
    assert GUARD64 not in got, "a stamp that is due was not written"
    assert got == sorted(got), "stamps decrease: %r" % (got,)
    struct.pack_into("<%dQ" % total, img, stamps, *([GUARD64] * total))
    return got


# ------------------------------- A. one wave against a pre-set inbox ----

ROLES = [pytest.param(1, id="leader"), pytest.param(0, id="follower")]
BASES = [pytest.param(0, 0, id="zero"), pytest.param(100, 5000, id="ring"),
         pytest.param(2**40 + 3, 2**33 + 1, id="above32")]


def run_one_wave(native, kind, mem, role, stamps):
    dev = Device(native, kind, mem)
    stamped, = run_waves(mem, [role])
    native.pingpong(on_device(dev, role), None, null_stream())
    img, words = dev.read()
    take_stamps(img, stamps, role["iters"], stamped)
    assert_same((img, words), mem)
    return mem


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("base,in_base", BASES)
@pytest.mark.parametrize("nbytes", [16, 32, 1024, 1040, 4112])
@pytest.mark.parametrize("iters", [1, 2, 7])
@pytest.mark.parametrize("leader", ROLES)
def test_one_wave_against_a_preset_inbox(native, hz, leader, iters, nbytes, base, in_base, kind):
    """The inbox flag is in_base + iters exactly (the >= boundary on the last
    iteration) and every inbox vector is (P, P) with P = in_base + iters, so
    only the last iteration finds its payload: both checking lanes count each
    of the others.  The wave never spins.  Its out slot carries base + iters
    in the flag and in every u64 of the payload and is otherwise untouched;
    the inbox is unchanged; a leader stamps entries 0..iters and no more, a
    follower none."""
    mem, slots, stamps, status = ping_memory(nbytes, iters)
    role = ping_role(slots, stamps, status, nbytes, iters, leader, base, in_base, int(2 * hz))
    p = in_base + iters
    mem.put64(slots[1], p)
    fill_payload(mem, slots[1], nbytes, p)
    inbox = bytes(mem.img[slots[1] - 256:slots[1] + HEADER + nbytes + 256])
    run_one_wave(native, kind, mem, role, stamps)
    # What the model must have come to, spelled out.
    assert mem.get32(status) == 0
    assert mem.get64(slots[0]) == base + iters
    assert all(mem.get64(slots[0] + HEADER + off) == base + iters for off in range(0, nbytes, 8))
    assert bytes(mem.img[slots[1] - 256:slots[1] + HEADER + nbytes + 256]) == inbox
    if nbytes > 16:
        assert mem.get32(status + 4) == 2 * (iters - 1)


CORRUPTIONS = [
    pytest.param(("first.y",), 1, id="first-y"),
    pytest.param(("last.x",), 1, id="last-x"),
    pytest.param(("first.y", "last.x"), 2, id="both"),
    pytest.param(("middle",), 0, id="middle"),
]


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("nbytes", [48, 1040])
@pytest.mark.parametrize("where,count", CORRUPTIONS)
@pytest.mark.parametrize("leader", ROLES)
def test_check_reads_both_halves_of_both_end_vectors(native, hz, leader, where, count, nbytes, kind):
    """The contract of ping_check: after the acquire, lane 0 compares both u64
    of the first 16 bytes of the payload with the awaited sequence number and
    lane 1 both u64 of the last 16 bytes, and each counts its vector once in
    status[1].  Only the two ends are looked at: a wrong middle vector goes
    unnoticed (the payload between the ends is covered by the byte-for-byte
    comparisons of what ping_send wrote, in the other tests)."""
    base, in_base = 7, 2**33 + 1
    mem, slots, stamps, status = ping_memory(nbytes, 1)
    role = ping_role(slots, stamps, status, nbytes, 1, leader, base, in_base, int(2 * hz))
    want = in_base + 1
    mem.put64(slots[1], want)
    fill_payload(mem, slots[1], nbytes, want)
    payload = slots[1] + HEADER
    wrong = {"first.y": payload + 8, "last.x": payload + nbytes - 16, "middle": payload + 16 + 8}
    for w in where:
        mem.put64(wrong[w], want ^ (1 << 32))
    run_one_wave(native, kind, mem, role, stamps)
    assert (mem.get32(status), mem.get32(status + 4)) == (0, count)


# -------------------------- B. two waves, one workgroup, real hand-offs ----

def pair_memory(nbytes, iters, a_base, b_base, ticks):
    """The two roles as device_pingpong builds them (b: a's mirror image, same
    stamps and status), and slots as earlier launches left them: flag and
    payload at the writer's base."""
    mem, slots, stamps, status = ping_memory(nbytes, iters)
    a = ping_role(slots, stamps, status, nbytes, iters, 1, a_base, b_base, ticks, out=0)
    b = ping_role(slots, stamps, status, nbytes, iters, 0, b_base, a_base, ticks, out=1)
    for slot, base in ((slots[0], a_base), (slots[1], b_base)):
        mem.put64(slot, base)
        fill_payload(mem, slot, nbytes, base)
    return mem, a, b, slots, stamps, status


def launch_pair(native, hz, dev, mem, a, b, stamps):
    """One launch of both waves, compared with the model; returns the stamps."""
    stamped = run_waves(mem, [a, b])
    assert stamped == [a["iters"] + 1, 0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    native.pingpong(on_device(dev, a), on_device(dev, b), null_stream())
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    img, words = dev.read()
    got = take_stamps(img, stamps, a["iters"], stamped[0])
    assert_same((img, words), mem)
    # A kernel cannot have run longer than the host waited for it: this pins
    # the tick unit from above without a measured constant.
    kernel_s = (got[-1] - got[0]) / hz
    assert 0 < kernel_s <= host_s, "%d ticks at %g Hz are %.6f s, the host waited %.6f s" % (
        got[-1] - got[0], hz, kernel_s, host_s)
    return got


def assert_pair_finished(mem, a, b, slots, status, nbytes):
    assert (mem.get32(status), mem.get32(status + 4)) == (0, 0)
    for slot, r in ((slots[0], a), (slots[1], b)):
        final = r["base"] + r["iters"]
        assert mem.get64(slot) == final
        assert all(mem.get64(slot + HEADER + off) == final for off in range(0, nbytes, 8))


PAIR_BASES = [pytest.param(0, 0, id="pingpong"), pytest.param(100, 5000, id="ring")]


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("a_base,b_base", PAIR_BASES)
@pytest.mark.parametrize("nbytes", [16, 1040, 65536])
@pytest.mark.parametrize("iters", [1, 2, 200])
def test_two_waves_hand_off(native, hz, iters, nbytes, a_base, b_base, kind):
    """The self ping-pong: leader and follower as two waves of one workgroup,
    mirrored as device_pingpong mirrors them, and the ring form (each wave
    counts what it writes from its own base and what it awaits from the
    other's).  No deadline, no early payload; both flags and every payload
    u64 at the final sequence numbers; guards intact; stamps in order and no
    longer apart than the host waited."""
    mem, a, b, slots, stamps, status = pair_memory(nbytes, iters, a_base, b_base, int(2 * hz))
    dev = Device(native, kind, mem)
    launch_pair(native, hz, dev, mem, a, b, stamps)
    assert_pair_finished(mem, a, b, slots, status, nbytes)


@pytest.mark.parametrize("kind", MEMORY)
def test_two_waves_hand_off_above_32_bits(native, hz, kind):
    mem, a, b, slots, stamps, status = pair_memory(1040, 2, 2**40 + 3, 2**33 + 1, int(2 * hz))
    dev = Device(native, kind, mem)
    launch_pair(native, hz, dev, mem, a, b, stamps)
    assert_pair_finished(mem, a, b, slots, status, 1040)


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("nbytes", [16, 1040, 65536])
@pytest.mark.parametrize("iters", [1, 2, 200])
def test_flags_are_monotonic_across_launches(native, hz, iters, nbytes, kind):
    """Two launches in a row on the same slots with nothing reset between
    them; the second counts on from where the first stopped."""
    mem, a, b, slots, stamps, status = pair_memory(nbytes, iters, 0, 0, int(2 * hz))
    dev = Device(native, kind, mem)
    launch_pair(native, hz, dev, mem, a, b, stamps)
    for r in (a, b):
        r["base"] += iters
        r["in_base"] += iters
    launch_pair(native, hz, dev, mem, a, b, stamps)
    assert_pair_finished(mem, a, b, slots, status, nbytes)
    assert mem.get64(slots[0]) == 2 * iters


# --------------------------------- C. signal kernel, nothing left waiting ----

def signal_memory(status_in_host, preset=0, nwords=0):
    """16 flag lines, a trap line and a status line in the arena; the status
    word optionally in a HostWords line (the last one) instead."""
    lay = Layout()
    flags = lay.add("flag lines", LINE * MAX_SIGNALS)
    lines = [flags + LINE * i for i in range(MAX_SIGNALS)]
    trap = lay.add("trap line", LINE)
    status = lay.add("status", LINE)
    mem = Mem(lay, nwords + (1 if status_in_host else 0))
    if status_in_host:
        status = Mem.word(nwords)
    mem.put32(status, preset)
    return mem, lines, trap, status


def launch_signal(native, dev, posts, waits, status, ticks, release_first, trap, stream=None):
    native.signal([(dev.ptr(f), v) for f, v in posts], [(dev.ptr(f), v) for f, v in waits], dev.ptr(status), ticks,
                  bool(release_first), null_stream() if stream is None else stream, dev.ptr(trap))


STATUS_HOME = [pytest.param(False, id="status-device"), pytest.param(True, id="status-host")]
RELEASE_FIRST = [pytest.param(0, id="plain"), pytest.param(1, id="release-first")]


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("release_first", RELEASE_FIRST)
@pytest.mark.parametrize("status_in_host", STATUS_HOME)
@pytest.mark.parametrize("nposts", [0, 1, 2, 15, 16])
def test_signal_posts(native, hz, nposts, status_in_host, release_first, kind):
    """Lane i stores value i to flag i for i < nposts and nothing else: every
    other line, the trap line (where the entries past nposts point) and the
    status stay as they were."""
    mem, lines, trap, status = signal_memory(status_in_host)
    posts = [(lines[i], 2**40 + i) for i in range(nposts)]
    dev = Device(native, kind, mem)
    assert not model_signal(mem, posts, [], status)
    launch_signal(native, dev, posts, [], status, int(0.2 * hz), release_first, trap)
    assert_same(dev.read(), mem)
    assert [mem.get64(lines[i]) for i in range(nposts)] == [2**40 + i for i in range(nposts)]
    assert mem.get64(trap) == GUARD64 and mem.get32(status) == 0


def satisfied_pair(i):
    """(flag, value) of a wait that holds: equal; far above; and a pair whose
    low 32 bits alone say the opposite."""
    return [(2**40 + i, 2**40 + i), (2**33, 2**32 + 7), (2**63 + i, 5)][i % 3]


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("release_first", RELEASE_FIRST)
@pytest.mark.parametrize("status_in_host", STATUS_HOME)
@pytest.mark.parametrize("preset", [0, 2])
@pytest.mark.parametrize("nwaits,first", [(0, 0), (1, 0), (1, 1), (16, 0), (16, 1)])
def test_signal_waits_already_satisfied(native, hz, nwaits, first, preset, status_in_host, release_first, kind):
    """Waits whose flags already hold (flag == value among them, and flag =
    2**33 against value = 2**32 + 7, which a 32-bit compare would wait on)
    pass at once and write nothing: the status stays what it was, 0 or 2."""
    mem, lines, trap, status = signal_memory(status_in_host, preset)
    waits = []
    for i in range(nwaits):
        flag, value = satisfied_pair(i + first)
        mem.put64(lines[i], flag)
        waits.append((lines[i], value))
    dev = Device(native, kind, mem)
    assert not model_signal(mem, [], waits, status)
    launch_signal(native, dev, [], waits, status, int(0.2 * hz), release_first, trap)
    assert_same(dev.read(), mem)
    assert mem.get32(status) == preset


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("release_first", RELEASE_FIRST)
def test_signal_posts_before_it_waits(native, hz, release_first, kind):
    """One launch posts F = v and waits for F >= v: it passes only because the
    posts come first."""
    mem, lines, trap, status = signal_memory(False)
    v = 2**40 + 9
    mem.put64(lines[3], v - 1)
    dev = Device(native, kind, mem)
    assert not model_signal(mem, [(lines[3], v)], [(lines[3], v)], status)
    launch_signal(native, dev, [(lines[3], v)], [(lines[3], v)], status, int(0.2 * hz), release_first, trap)
    assert_same(dev.read(), mem)
    assert mem.get32(status) == 0


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("release_first", RELEASE_FIRST)
@pytest.mark.parametrize("status_in_host", STATUS_HOME)
def test_signal_chain_in_stream_order(native, hz, status_in_host, release_first, kind):
    """Three launches on one stream: post F; wait F and post G; wait F and G."""
    mem, lines, trap, status = signal_memory(status_in_host)
    f, g = lines[0], lines[9]
    vf, vg = 2**40 + 1, 2**32 + 2
    mem.put64(f, 0)
    mem.put64(g, vg - 1)
    dev = Device(native, kind, mem)
    chain = [([(f, vf)], []), ([(g, vg)], [(f, vf)]), ([], [(f, vf), (g, vg)])]
    for posts, waits in chain:
        assert not model_signal(mem, posts, waits, status)
        launch_signal(native, dev, posts, waits, status, int(0.2 * hz), release_first, trap)
    assert_same(dev.read(), mem)
    assert (mem.get64(f), mem.get64(g), mem.get32(status)) == (vf, vg, 0)


# ------------------------------- D. signal kernel, released by the host ----

def sixteen_waits(mem, lines, k, flag_k, value_k):
    """16 waits that hold except lane k's, whose flag is HostWords line 0."""
    waits = []
    for i in range(MAX_SIGNALS):
        if i == k:
            mem.put64(Mem.word(0), flag_k)
            waits.append((Mem.word(0), value_k))
        else:
            flag, value = satisfied_pair(i)
            mem.put64(lines[i], flag)
            waits.append((lines[i], value))
    return waits


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("k,first,value", [(0, 0, 2**40 + 2), (5, 0, 2**40 + 2), (15, 0, 2**40 + 2),
                                           (5, 2**32 + 5, 2**33 + 1)],
                         ids=["lane0", "lane5", "lane15", "lane5-above32"])
def test_signal_waits_for_the_host(native, hz, k, first, value, kind):
    """15 waits hold, lane k's does not: the kernel stays until the host
    stores the value itself (value - 1 does not do; nor does a flag whose low
    32 bits alone are past the value's), then leaves with status 0."""
    mem, lines, trap, status = signal_memory(False, nwords=1)
    waits = sixteen_waits(mem, lines, k, first, value)
    dev = Device(native, kind, mem)
    side = torch.cuda.Stream()
    launch_signal(native, dev, [], waits, status, int(5 * hz), 0, trap, side.cuda_stream)
    try:
        time.sleep(0.05)
        assert not side.query(), "the kernel left although lane %d's flag is not there" % k
        dev.store(Mem.word(0), value - 1)
        time.sleep(0.05)
        assert not side.query(), "the kernel left on value - 1"
    finally:
        dev.store(Mem.word(0), value)  # whatever happened: nothing stays waiting
        side.synchronize()
    mem.put64(Mem.word(0), value)
    assert not model_signal(mem, [], waits, status)
    assert_same(dev.read(), mem)
    assert mem.get32(status) == 0


# --------------------------------------------------------- E. deadlines ----

DEADLINE_S = 0.05
BACKSTOP_S = 5.0


def run_to_deadline(dev, launch, release):
    """Launches on a side stream and waits for the kernel to leave by itself.
    A safety cap, not a measurement: 5 s after the launch, and in any case once
    the stream is seen done, the host stores every awaited value (release), so
    even broken deadline code ends; the test fails if that is what ended it.
    Returns the host's time from just before the launch until it saw the
    stream done, which the kernel's own time cannot exceed."""
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    launch(side.cuda_stream)
    try:
        while True:
            done = side.query()
            elapsed = time.perf_counter() - t0
            if done or elapsed > BACKSTOP_S:
                break
            time.sleep(0.0005)
    finally:
        for addr, value in release:
            dev.store(addr, value)
        side.synchronize()
    assert done, "the kernel was still waiting %.1f s after a %.2f s deadline" % (BACKSTOP_S, DEADLINE_S)
    print("deadline: left after %.4f s, %.3f x the %.2f s asked for" % (elapsed, elapsed / DEADLINE_S, DEADLINE_S))
    assert elapsed >= DEADLINE_S, "the kernel left %.4f s after its launch, before its %.2f s deadline" % (
        elapsed, DEADLINE_S)
    return elapsed


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("status_in_host", STATUS_HOME)
@pytest.mark.parametrize("preset", [0, 2])
@pytest.mark.parametrize("k,first,value", [(0, 2**40, 2**40 + 1), (15, 2**40, 2**40 + 1), (15, 2**32 + 5, 2**33 + 1)],
                         ids=["lane0", "lane15", "lane15-above32"])
def test_signal_deadline(native, hz, k, first, value, preset, status_in_host, kind):
    """16 waits on HostWords flags, lane k's short of its value (once only in
    the high 32 bits): the kernel leaves at its deadline, not before, ORs bit
    0 into the status, and its own posts were made all the same."""
    mem, lines, trap, status = signal_memory(status_in_host, preset, nwords=MAX_SIGNALS)
    waits = []
    for i in range(MAX_SIGNALS):
        flag, want = (first, value) if i == k else satisfied_pair(i)
        mem.put64(Mem.word(i), flag)
        waits.append((Mem.word(i), want))
    posts = [(lines[i], 2**40 + i) for i in (0, 7, 15)]
    dev = Device(native, kind, mem)
    assert model_signal(mem, posts, waits, status)
    run_to_deadline(dev, lambda s: launch_signal(native, dev, posts, waits, status, int(DEADLINE_S * hz), 0, trap, s),
                    [(Mem.word(k), value)])
    mem.put64(Mem.word(k), value)  # the release above
    assert_same(dev.read(), mem)
    assert mem.get32(status) == preset | 1


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("leader,behind", [(1, -1), (0, 0), (0, 2**40 + 1 - (2**32 + 5))],
                         ids=["leader", "follower", "follower-above32"])
def test_pingpong_deadline(native, hz, leader, behind, kind):
    """A wave whose partner stops answering.  The leader of three iterations
    gets one reply (inbox flag in_base + 1): it leaves at its deadline with
    status[0] = 1, having sent message 2 (out flag base + 2) and stamped
    entries 0 and 1 only.  The follower finds its inbox at in_base, or at
    2**32 + 5, below in_base in the high 32 bits only: it leaves at its
    deadline having sent and stamped nothing."""
    iters, nbytes, base, in_base = 3, 1040, 2**33 + 5, 2**40 + 1
    mem, slots, stamps, status = ping_memory(nbytes, iters, nwords=1)
    role = ping_role(slots, stamps, status, nbytes, iters, leader, base, in_base, int(DEADLINE_S * hz))
    role["in_flag"] = Mem.word(0)
    arrived = in_base - behind
    mem.put64(Mem.word(0), arrived)
    fill_payload(mem, slots[1], nbytes, arrived)
    untouched = bytes(mem.img)
    dev = Device(native, kind, mem)
    stamped, = run_waves(mem, [role])
    run_to_deadline(dev, lambda s: native.pingpong(on_device(dev, role), None, s), [(Mem.word(0), in_base + iters)])
    mem.put64(Mem.word(0), in_base + iters)  # the release above
    img, words = dev.read()
    take_stamps(img, stamps, iters, stamped)
    assert_same((img, words), mem)
    assert (mem.get32(status), mem.get32(status + 4)) == (1, 0)
    if leader:
        assert stamped == 2 and mem.get64(slots[0]) == base + 2
    else:
        assert stamped == 0
        expected = bytearray(untouched)
        struct.pack_into("<I", expected, status, 1)
        assert bytes(mem.img) == bytes(expected)
