"""The device-initiated stream kernel of csrc/stream.hip, driven directly on one
GPU through native.stream, in the style of tests/test_kernels_signal_gpu.py
(whose arena, model memory and byte-for-byte comparison it reuses).

A channel is a credit-flow ring: the sender writes message i (vector j = the
two 64-bit words {seq, j}, seq = base + i + 1) into slot i % depth and
publishes tail = seq; the receiver waits for tail, compares the slot and hands
the credit back as head = seq; the sender reuses a slot only once head says
its last message was consumed, and leaves only when head == base + iters.

Every expected byte comes from a Python model of that protocol (StreamWave,
run_stream below), never from another kernel run.  Everything a kernel may
write lies between 0xAB guards and is compared whole; the stamp regions hold
the device's clock, so they are checked on their own (how many entries, their
order, the causal order between sender and receiver) and masked out of the
byte compare.  Each case runs once on a torch tensor (plain hipMalloc) and
once on a native.signal_page (what the transport uses).

Sections: A a receiver against a pre-written ring (nothing spins), B a sender
with every credit granted in advance, C senders and receivers in one launch so
that credits really flow, D deadlines.  Every wait in D is bounded twice: by
the kernel's own 20 ms deadline and by the host storing the awaited flag
afterwards whatever the test saw.
"""
import struct
import time

import numpy as np
import pytest
import torch

from test_kernels_signal_gpu import GUARD64, Device, Layout, Mem, assert_same, null_stream

pytestmark = pytest.mark.gpu

HEADER = 256  # tail, then the ring on its own lines (stream_layout.hpp kHeader)
LINE = 128    # one head per line (stream_layout.hpp kCreditLine)
SPARE_STAMPS = 4  # guard entries behind the last stamp a role may write
MEMORY = ["tensor", "page"]
STREAM_POINTERS = ("out_flag", "in_flag", "ring", "stamps", "status")


@pytest.fixture(scope="module", autouse=True)
def _gpu(native):
    assert torch.cuda.is_available(), "GPU tier needs a GPU"
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def hz(native):
    rate = native.wall_clock_hz()
    assert rate > 0
    return rate


# ------------------------------------------------------------- the model ----

def message(seq, nbytes):
    """The bytes of the message with sequence number seq."""
    v = np.empty((nbytes // 16, 2), dtype="<u8")
    v[:, 0] = seq
    v[:, 1] = np.arange(nbytes // 16, dtype="<u8")
    return v.tobytes()


def checked_vectors(nbytes, check_all):
    nvec = nbytes // 16
    if check_all:
        return list(range(nvec))
    return [0] if nvec == 1 else [0, nvec - 1]


class StreamWave:
    """One role of stream_kernel on a Mem.  Stamps are counted, not written."""

    def __init__(self, mem, role):
        self.mem, self.r = mem, role
        self.i = 0
        self.done = False
        self.stamped = 1 if role["sender"] else 0  # stamps[0]
        self.idx = np.array(checked_vectors(role["bytes"], role["check_all"]), dtype="<u8")

    def slot(self, i):
        return self.r["ring"] + (i % self.r["depth"]) * self.r["bytes"]

    def step(self):
        """Runs until the wave is done or must wait; True if it got anywhere."""
        r, mem = self.r, self.mem
        moved = False
        while not self.done:
            seq = r["base"] + self.i + 1
            if r["sender"]:
                if self.i == r["iters"]:
                    if mem.get64(r["in_flag"]) < r["base"] + r["iters"]:
                        break
                    self.stamped += 1  # stamps[iters + 1]
                    self.done = True
                    return True
                if self.i >= r["depth"] and mem.get64(r["in_flag"]) < seq - r["depth"]:
                    break
                at = self.slot(self.i)
                mem.img[at:at + r["bytes"]] = message(seq, r["bytes"])
                mem.put64(r["out_flag"], seq)
                self.stamped += 1  # stamps[i + 1]
            else:
                if self.i == r["iters"]:
                    self.done = True
                    return moved
                if mem.get64(r["in_flag"]) < seq:
                    break
                self.stamped += 1  # stamps[i]
                at = self.slot(self.i)
                got = np.frombuffer(bytes(mem.img[at:at + r["bytes"]]), dtype="<u8").reshape(-1, 2)
                bad = int(np.count_nonzero((got[self.idx, 0] != np.uint64(seq)) | (got[self.idx, 1] != self.idx)))
                mem.put32(r["status"] + 4, mem.get32(r["status"] + 4) + bad)
                mem.put64(r["out_flag"], seq)
            self.i += 1
            moved = True
        return moved

    def expire(self):
        self.mem.put32(self.r["status"], self.mem.get32(self.r["status"]) | 1)
        self.done = True


def run_stream(mem, roles):
    """The roles of one launch to their end; a role nobody will ever answer
    leaves at its deadline.  Returns the stamp count of each."""
    waves = [StreamWave(mem, r) for r in roles]
    while not all(w.done for w in waves):
        if not any([w.step() for w in waves]):
            for w in waves:
                if not w.done:
                    w.expire()
    return [w.stamped for w in waves]


# ------------------------------------------------------------ the memory ----

class Channel:
    """One channel's regions in a Layout: tail header and ring, head line, a
    stamp region and a status pair for each of the two roles."""

    def __init__(self, lay, name, nbytes, depth, iters):
        slot = lay.add("%s tail+ring" % name, HEADER + depth * nbytes)
        self.tail, self.ring = slot, slot + HEADER
        self.head = lay.add("%s head" % name, LINE)
        self.send_total = iters + 2 + SPARE_STAMPS
        self.recv_total = iters + SPARE_STAMPS
        self.send_stamps = lay.add("%s sender stamps" % name, 8 * self.send_total)
        self.recv_stamps = lay.add("%s receiver stamps" % name, 8 * self.recv_total)
        self.send_status = lay.add("%s sender status" % name, 8)
        self.recv_status = lay.add("%s receiver status" % name, 8)
        self.nbytes, self.depth, self.iters = nbytes, depth, iters

    def clear(self, mem, base):
        """Flags as earlier launches left them, status words zeroed."""
        mem.put64(self.tail, base)
        mem.put64(self.head, base)
        for st in (self.send_status, self.recv_status):
            mem.put64(st, 0)

    def role(self, sender, base, ticks, check_all=0, iters=None):
        r = {"bytes": self.nbytes, "base": base, "depth": self.depth, "iters": self.iters if iters is None else iters,
             "sender": sender, "check_all": check_all, "timeout_ticks": ticks, "ring": self.ring}
        if sender:
            r.update(out_flag=self.tail, in_flag=self.head, stamps=self.send_stamps, status=self.send_status)
        else:
            r.update(out_flag=self.head, in_flag=self.tail, stamps=self.recv_stamps, status=self.recv_status)
        return r


def on_device(dev, role):
    return {k: dev.ptr(v) if k in STREAM_POINTERS else v for k, v in role.items()}


def take_stamps(img, at, total, written):
    """The stamps a role wrote: exactly `written` entries, non-decreasing, the
    rest still guard.  Puts the guard back so the arena can be compared with
    the model, which has no clock."""
    vals = list(struct.unpack_from("<%dQ" % total, img, at))
    assert vals[written:] == [GUARD64] * (total - written), "a stamp past entry %d was written" % (written - 1)
    got = vals[:written]
    assert GUARD64 not in got, "a stamp that is due was not written"
    assert got == sorted(got), "stamps decrease: %r" % (got,)
    struct.pack_into("<%dQ" % total, img, at, *([GUARD64] * total))
    return got


def status_of(mem, at):
    return mem.get32(at), mem.get32(at + 4)


# ---------------------------- A. a receiver against a pre-written ring ----

def prewritten(nbytes, depth, iters, base):
    lay = Layout()
    ch = Channel(lay, "ch0", nbytes, depth, iters)
    mem = Mem(lay)
    ch.clear(mem, base)
    for i in range(iters):
        at = ch.ring + (i % depth) * nbytes
        mem.img[at:at + nbytes] = message(base + i + 1, nbytes)
    mem.put64(ch.tail, base + iters)
    return mem, ch


def run_receiver(native, kind, mem, ch, role):
    dev = Device(native, kind, mem)
    stamped, = run_stream(mem, [role])
    native.stream([on_device(dev, role)], null_stream())
    img, words = dev.read()
    take_stamps(img, ch.recv_stamps, ch.recv_total, stamped)
    assert_same((img, words), mem)
    return stamped


BASES = [pytest.param(0, id="zero"), pytest.param(2**40 + 3, id="above32")]


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("check_all", [0, 1])
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("nbytes", [16, 48, 1040, 4096])
@pytest.mark.parametrize("depth,iters", [(1, 1), (2, 2), (8, 5), (8, 8)])
def test_receiver_against_a_prewritten_ring(native, hz, depth, iters, nbytes, base, check_all, kind):
    """iters <= depth messages lie in the ring and tail says so: the receiver
    never spins, finds nothing wrong, hands back head = base + iters and
    stamps exactly iters entries; the ring and the tail are untouched."""
    mem, ch = prewritten(nbytes, depth, iters, base)
    ring = bytes(mem.img[ch.tail - 256:ch.ring + depth * nbytes + 256])
    stamped = run_receiver(native, kind, mem, ch, ch.role(0, base, int(2 * hz), check_all))
    assert stamped == iters
    assert mem.get64(ch.head) == base + iters
    assert status_of(mem, ch.recv_status) == (0, 0)
    assert bytes(mem.img[ch.tail - 256:ch.ring + depth * nbytes + 256]) == ring


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("check_all,count", [(1, 2), (0, 1)])
@pytest.mark.parametrize("half", ["x", "y"])
@pytest.mark.parametrize("nbytes", [48, 1040, 4096])
def test_receiver_counts_wrong_vectors(native, hz, nbytes, half, check_all, count, kind):
    """One vector in the middle of message 1 and the last vector of message 2
    are wrong in one of their two words: check_all counts both, the end check
    only the last one.  The credit is handed back all the same."""
    base, depth, iters = 2**33 + 1, 4, 4
    mem, ch = prewritten(nbytes, depth, iters, base)
    nvec = nbytes // 16
    off = 0 if half == "x" else 8
    for msg, vec in ((1, nvec // 2), (2, nvec - 1)):
        at = ch.ring + msg * nbytes + 16 * vec + off
        mem.put64(at, mem.get64(at) ^ (1 << 32))
    run_receiver(native, kind, mem, ch, ch.role(0, base, int(2 * hz), check_all))
    assert status_of(mem, ch.recv_status) == (0, count)
    assert mem.get64(ch.head) == base + iters


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("check_all", [0, 1])
@pytest.mark.parametrize("nbytes", [16, 1040])
def test_receiver_tells_a_stale_slot(native, hz, nbytes, check_all, kind):
    """Slot 1 still holds the message of one lap earlier (seq - depth), whole
    and well formed: every vector the receiver checks there counts."""
    base, depth, iters = 2**33 + 1, 4, 4
    mem, ch = prewritten(nbytes, depth, iters, base)
    at = ch.ring + nbytes
    mem.img[at:at + nbytes] = message(base + 2 - depth, nbytes)
    run_receiver(native, kind, mem, ch, ch.role(0, base, int(2 * hz), check_all))
    assert status_of(mem, ch.recv_status) == (0, len(checked_vectors(nbytes, check_all)))


# ------------------------- B. a sender with every credit granted already ----

@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("nbytes", [16, 1040, 4096, 65536])
@pytest.mark.parametrize("depth,iters", [(1, 1), (1, 4), (2, 7), (8, 5), (8, 25)])
def test_sender_with_credits_granted(native, hz, depth, iters, nbytes, base, kind):
    """head == base + iters from the start, so the sender never waits: slot k
    ends up holding the last message with i % depth == k (slots never reached
    stay guard), tail == base + iters, and iters + 2 stamps are written."""
    lay = Layout()
    ch = Channel(lay, "ch0", nbytes, depth, iters)
    mem = Mem(lay)
    ch.clear(mem, base)
    mem.put64(ch.head, base + iters)
    role = ch.role(1, base, int(2 * hz))
    dev = Device(native, kind, mem)
    stamped, = run_stream(mem, [role])
    native.stream([on_device(dev, role)], null_stream())
    img, words = dev.read()
    take_stamps(img, ch.send_stamps, ch.send_total, stamped)
    assert_same((img, words), mem)
    assert stamped == iters + 2
    assert mem.get64(ch.tail) == base + iters and mem.get64(ch.head) == base + iters
    assert status_of(mem, ch.send_status) == (0, 0)
    for k in range(min(depth, iters)):
        last = max(i for i in range(iters) if i % depth == k)
        assert bytes(mem.img[ch.ring + k * nbytes:ch.ring + (k + 1) * nbytes]) == message(base + last + 1, nbytes)


# -------------------------- C. senders and receivers in one launch ----

def flow_memory(nbytes, depth, iters, channels, bases):
    lay = Layout()
    chans = [Channel(lay, "ch%d" % c, nbytes, depth, iters) for c in range(channels)]
    mem = Mem(lay)
    for ch, base in zip(chans, bases):
        ch.clear(mem, base)
    return mem, chans


def launch_flow(native, hz, dev, mem, chans, bases, check_all):
    """One launch of every channel's receiver and sender, compared with the
    model; then the causal order of the stamps, channel by channel."""
    ticks = int(5 * hz)
    roles = [ch.role(0, b, ticks, check_all) for ch, b in zip(chans, bases)]
    roles += [ch.role(1, b, ticks) for ch, b in zip(chans, bases)]
    stamped = run_stream(mem, roles)
    iters, depth = chans[0].iters, chans[0].depth
    assert stamped == [iters] * len(chans) + [iters + 2] * len(chans)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    native.stream([on_device(dev, r) for r in roles], null_stream())
    torch.cuda.synchronize()
    host_s = time.perf_counter() - t0
    img, words = dev.read()
    first, last = None, None
    for ch in chans:
        send = take_stamps(img, ch.send_stamps, ch.send_total, iters + 2)
        recv = take_stamps(img, ch.recv_stamps, ch.recv_total, iters)
        # One device clock, so all exact.  A message arrives after the sender
        # started it; a slot is republished only after its credit; the sender
        # leaves after the last message was consumed.
        for i in range(iters):
            assert send[i] <= recv[i], "message %d arrived at %d, before the sender began it at %d" % (i, recv[i], send[i])
        for i in range(depth, iters):
            assert recv[i - depth] <= send[i + 1], "message %d published at %d, before slot's credit at %d" % (
                i, send[i + 1], recv[i - depth])
        assert recv[iters - 1] <= send[iters + 1]
        first = send[0] if first is None else min(first, send[0])
        last = send[-1] if last is None else max(last, send[-1])
    assert_same((img, words), mem)
    # A kernel cannot have run longer than the host waited for it.
    span_s = (last - first) / hz
    assert 0 < span_s <= host_s, "%d ticks at %g Hz are %.6f s, the host waited %.6f s" % (last - first, hz, span_s, host_s)


def assert_flow_finished(mem, chans, bases, total):
    """Flags at base + total, status clean, slot k holding the last message
    with i % depth == k of the last launch (sequence numbers run on)."""
    for ch, base in zip(chans, bases):
        assert mem.get64(ch.tail) == base + total and mem.get64(ch.head) == base + total
        assert status_of(mem, ch.send_status) == (0, 0) and status_of(mem, ch.recv_status) == (0, 0)
        for k in range(min(ch.depth, ch.iters)):
            last = max(i for i in range(ch.iters) if i % ch.depth == k)
            want = message(base + total - ch.iters + last + 1, ch.nbytes)
            assert bytes(mem.img[ch.ring + k * ch.nbytes:ch.ring + (k + 1) * ch.nbytes]) == want


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("channels", [1, 4])
@pytest.mark.parametrize("nbytes", [16, 1040, 4096, 65536])
@pytest.mark.parametrize("depth", [1, 2, 8])
@pytest.mark.parametrize("long", [False, True], ids=["3xdepth+1", "300"])
def test_credits_flow(native, hz, long, depth, nbytes, channels, kind):
    """Senders and receivers of every channel in one launch, each channel with
    its own ring, flags, stamps and status, bases above 2**32 and different
    per channel.  The first launch checks every vector; a second one on the
    same memory counts on from where the first stopped, nothing reset, and
    checks the ends only.  After each the arena is the model's."""
    iters = 300 if long else 3 * depth + 1
    bases = [2**32 + 5 + 1000 * c for c in range(channels)]
    mem, chans = flow_memory(nbytes, depth, iters, channels, bases)
    dev = Device(native, kind, mem)
    launch_flow(native, hz, dev, mem, chans, bases, check_all=1)
    assert_flow_finished(mem, chans, bases, iters)
    launch_flow(native, hz, dev, mem, chans, [b + iters for b in bases], check_all=0)
    assert_flow_finished(mem, chans, bases, 2 * iters)


LIMITS = [pytest.param(8, 1040, 2, id="16-roles"),            # MAX_STREAM_ROLES: 8 receivers and 8 senders
          pytest.param(1, 1 << 20, 4, id="1MiB-4MiB-ring"),   # the largest message in the largest ring
          pytest.param(1, 65536, 64, id="depth-64")]          # the deepest ring, again 4 MiB


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("channels,nbytes,depth", LIMITS)
def test_credits_flow_at_the_limits(native, hz, channels, nbytes, depth, kind):
    """test_credits_flow at the shapes the kernel's limits name (kernels.hpp:
    16 roles a launch, 1 MiB a message, depth 64, a ring of 4 MiB), each ring
    lapped three times: 3 x depth + 1 messages, then as many again."""
    assert native.MAX_STREAM_ROLES == 2 * 8 and depth * nbytes <= 4 << 20
    iters = 3 * depth + 1
    bases = [2**32 + 5 + 1000 * c for c in range(channels)]
    mem, chans = flow_memory(nbytes, depth, iters, channels, bases)
    dev = Device(native, kind, mem)
    launch_flow(native, hz, dev, mem, chans, bases, check_all=1)
    assert_flow_finished(mem, chans, bases, iters)
    launch_flow(native, hz, dev, mem, chans, [b + iters for b in bases], check_all=0)
    assert_flow_finished(mem, chans, bases, 2 * iters)


# --------------------------------------------------------- D. deadlines ----

DEADLINE_S = 0.02
BACKSTOP_S = 5.0


def run_to_deadline(dev, launch, release):
    """Launches on a side stream and waits for the kernel to leave by itself.
    A safety cap, not a measurement: 5 s after the launch, and in any case once
    the stream is seen done, the host stores every awaited value (release), so
    even broken deadline code ends; the test fails if that is what ended it."""
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


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("depth", [1, 4])
def test_sender_without_credits_stops_at_the_ring(native, hz, depth, kind):
    """A sender of depth + 1 messages whose head (a HostWords line) stays at
    base: it publishes exactly depth messages, leaves at its deadline with
    status bit 0, tail == base + depth, and depth + 1 stamps."""
    nbytes, base, iters = 1040, 2**33 + 5, depth + 1
    lay = Layout()
    ch = Channel(lay, "ch0", nbytes, depth, iters)
    mem = Mem(lay, nwords=1)
    ch.clear(mem, base)
    mem.put64(Mem.word(0), base)
    role = ch.role(1, base, int(DEADLINE_S * hz))
    role["in_flag"] = Mem.word(0)
    dev = Device(native, kind, mem)
    stamped, = run_stream(mem, [role])
    run_to_deadline(dev, lambda s: native.stream([on_device(dev, role)], s), [(Mem.word(0), base + iters)])
    mem.put64(Mem.word(0), base + iters)  # the release above
    img, words = dev.read()
    take_stamps(img, ch.send_stamps, ch.send_total, stamped)
    assert_same((img, words), mem)
    assert stamped == depth + 1
    assert status_of(mem, ch.send_status) == (1, 0)
    assert mem.get64(ch.tail) == base + depth


@pytest.mark.parametrize("kind", MEMORY)
@pytest.mark.parametrize("behind", [0, 2**40 + 1 - (2**32 + 5)], ids=["at-base", "above32"])
def test_receiver_whose_tail_never_moves(native, hz, behind, kind):
    """The tail (a HostWords line) stays at base, or at 2**32 + 5, short of
    base + 1 in the high 32 bits only: the receiver leaves at its deadline
    with status bit 0, having stamped nothing and never written head."""
    nbytes, depth, iters, base = 1040, 2, 3, 2**40 + 1
    lay = Layout()
    ch = Channel(lay, "ch0", nbytes, depth, iters)
    mem = Mem(lay, nwords=1)
    ch.clear(mem, base)
    mem.put64(Mem.word(0), base - behind)
    role = ch.role(0, base, int(DEADLINE_S * hz), 1)
    role["in_flag"] = Mem.word(0)
    untouched = bytes(mem.img)
    dev = Device(native, kind, mem)
    stamped, = run_stream(mem, [role])
    run_to_deadline(dev, lambda s: native.stream([on_device(dev, role)], s), [(Mem.word(0), base + iters)])
    mem.put64(Mem.word(0), base + iters)  # the release above
    img, words = dev.read()
    take_stamps(img, ch.recv_stamps, ch.recv_total, stamped)
    assert_same((img, words), mem)
    assert stamped == 0 and status_of(mem, ch.recv_status) == (1, 0)
    expected = bytearray(untouched)
    struct.pack_into("<I", expected, ch.recv_status, 1)
    assert bytes(mem.img) == bytes(expected)
    assert mem.get64(ch.head) == base


# ------------------------------------------------------- bad arguments ----

def test_stream_refuses_bad_roles(native, hz):
    """Checked before anything touches the device."""
    lay = Layout()
    ch = Channel(lay, "ch0", 64, 2, 3)
    mem = Mem(lay)
    ch.clear(mem, 0)
    dev = Device(native, "tensor", mem)
    good = on_device(dev, ch.role(1, 0, int(hz)))
    assert native.MAX_STREAM_ROLES == 16
    for change in ({"bytes": 24}, {"bytes": 0}, {"bytes": (1 << 20) + 16}, {"depth": 0}, {"depth": 65}, {"iters": 0},
                   {"iters": 100001}, {"depth": 8, "bytes": 1 << 20}, {"ring": 0}, {"ring": good["ring"] + 8},
                   {"status": 0}, {"nonsense": 1}):
        with pytest.raises(ValueError):
            native.stream([dict(good, **change)], null_stream())
    with pytest.raises(ValueError):
        native.stream([], null_stream())
    with pytest.raises(ValueError):
        native.stream([good] * 17, null_stream())
    assert_same(dev.read(), mem)
