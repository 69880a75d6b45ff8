"""Emulated ranks of a direct peer-write exchange group (include/emf_hip.h, csrc/peer_exchange.hip) on ONE stream.

The transport's kernels never find out whether their peers are other GPUs, other processes or nobody at all: a rank is
an emf_peer_t, i.e. `world` receive-buffer pointers, `world` flag-page pointers and an error word.  Here all of them are
ordinary device memory of one process, and an exchange with sequence number s is PLAYED, on the null stream:

    1. every rank's producer runs (it stores into slot[rank] of every emulated peer),
    2. the test copies s into the flag words 0 .. world-1 of every flag page (a plain host-to-device copy),
    3. every rank's consumer runs: its signal rewrites the value that is already there, its poll ends on the first read.

No kernel waits for another kernel and no thread spins, so a protocol that only works when ranks happen to interleave
cannot pass by luck, and one that is wrong cannot hang: the wait is bounded by TIMEOUT_MS and a bookkeeping mistake of a
test ends as a set error word.  (Word 64 of a flag page is NOT a flag but the device-side mirror of the error word,
peer_core.hpp kDevErrorWord: a consumer behind a wait launch skips its exchange when it reads s there.  It stays zero.)

What the emulation pins beyond the consumers' outputs, which the tests compare themselves:
  * the receive buffers byte for byte.  The helper keeps a host mirror of every buffer, the tests tell it what each sender
    must have stored (`expect`), and `check_slots` compares whole buffers: the message, the poison in the rest of the slot,
    the other parity half, which must still be all poison.  Slots are poisoned between sequences, so a consumer that reads
    the stale half reads poison.
  * guard regions: `slot_guard` bytes at the end of every slot (slotBytes = message + guard; 0 for the tests of an exactly
    sized slot, where a neighbour's overrun shows in `check_slots`) and GUARD_BYTES behind every buffer.
  * the error words (0) and the flag pages (s in the flag words, 0 elsewhere) after every consumer.
Producers run in ascending rank order for sequences 1, 2, 5, 6 ... and descending for 3, 4, 7, 8 ...: with four sequences both
orders meet both parities, so a sender that overruns its slot is seen whichever neighbour it overwrites."""
import numpy as np

from emfusion_amd import _lib
from emfusion_amd.devmem import DeviceArray, memcpy_d2h

FLAG_PAGE_WORDS = 1024  # 4096 bytes
DEV_ERROR_WORD = 64     # peer_core.hpp kDevErrorWord
GUARD_BYTES = 256
TIMEOUT_MS = 2000
SEQUENCES = (1, 2, 3, 4)

# 16-byte poison patterns (u32 words).  Floats: every word a NaN, so one stale or foreign word makes a sum NaN.
NAN_POISON = np.full(4, 0xFFC0DEAD, np.uint32)
# Hit keys ((raylength bits << 32) | list position): position 240 -- inside the kernels' 256-entry id table, beyond every
# object list used here -- at a denormal raylength, i.e. a key smaller than every real one: a stale read wins every minimum.
KEY_POISON = np.array([0xF0, 0x1, 0xF0, 0x1], np.uint32)


def round16(n):
    return (int(n) + 15) // 16 * 16


class PeerEmulation:
    def __init__(self, ops, world, message_bytes, wait_in_front, poison=NAN_POISON, slot_guard=GUARD_BYTES):
        assert 1 <= world <= _lib.MAX_PEERS and slot_guard % 16 == 0
        self.ops, self.world = ops, world
        self.slot_bytes = round16(message_bytes) + slot_guard
        self.slot_guard = slot_guard
        self.buffer_bytes = ops.peer_buffer_bytes(world, self.slot_bytes)
        assert self.buffer_bytes == 2 * world * self.slot_bytes
        total = self.buffer_bytes + GUARD_BYTES
        self._poison = np.tile(np.asarray(poison, np.uint32).view(np.uint8), total // 16)
        self.buffers = [DeviceArray.from_numpy(self._poison) for _ in range(world)]
        self.mirror = [self._poison.copy() for _ in range(world)]
        self.flags = [DeviceArray.zeros((FLAG_PAGE_WORDS,), np.uint32) for _ in range(world)]
        self.errors = [DeviceArray.zeros((1,), np.uint32) for _ in range(world)]
        self.signalled = 0
        self.groups = []
        for r in range(world):
            g = _lib.EmfPeer()
            g.rank, g.world = r, world
            for p in range(world):
                g.slots[p] = self.buffers[p].ptr
                g.flags[p] = self.flags[p].ptr
            g.slotBytes = self.slot_bytes
            g.error = self.errors[r].ptr
            g.timeoutMs, g.waitInFront, g.systemFences = TIMEOUT_MS, int(bool(wait_in_front)), 0
            self.groups.append(g)

    # ---- the play ----
    def slot_offset(self, seq, sender):
        return ((seq & 1) * self.world + sender) * self.slot_bytes

    def poison(self):
        for buf, m in zip(self.buffers, self.mirror):
            buf.copy_from(self._poison)
            m[:] = self._poison

    def expect(self, seq, sender, data, offset=0):
        """Sender `sender` stores `data` (any dtype, taken as bytes) at `offset` of its slot on every rank."""
        b = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert offset + b.size <= self.slot_bytes - self.slot_guard, "a test's expectation overruns the message area"
        at = self.slot_offset(seq, sender) + offset
        for m in self.mirror:
            m[at:at + b.size] = b

    def signal(self, seq):
        page = np.zeros(FLAG_PAGE_WORDS, np.uint32)
        page[:self.world] = seq
        for f in self.flags:
            f.copy_from(page)
        self.signalled = seq

    def producer_order(self, seq):
        ranks = list(range(self.world))
        return ranks if ((seq - 1) // 2) % 2 == 0 else ranks[::-1]

    def play(self, seq, producer, consumer):
        """producer(rank, group) for every rank, the flags, consumer(rank, group) for every rank with the cheap checks behind
        each, then the receive buffers byte for byte.  The caller has poisoned the slots and stated its expectations."""
        for r in self.producer_order(seq):
            producer(r, self.groups[r])
        self.signal(seq)
        for r in range(self.world):
            consumer(r, self.groups[r])
            self.check_guards(f"behind the consumer of rank {r}, sequence {seq}")
        self.check_slots(f"sequence {seq}")

    # ---- the checks ----
    def _read(self, rank, offset, nbytes):
        out = np.empty(nbytes, np.uint8)
        memcpy_d2h(out, self.buffers[rank].ptr + offset)
        return out

    def check_guards(self, when):
        """Error words, flag pages, and the guard regions behind every slot and every buffer."""
        want = np.zeros(FLAG_PAGE_WORDS, np.uint32)
        want[:self.world] = self.signalled
        for r in range(self.world):
            err = int(self.errors[r].numpy()[0])
            assert err == 0, f"{when}: error word of rank {r} holds {err} (a wait timed out)"
            page = self.flags[r].numpy()
            assert np.array_equal(page, want), f"{when}: flag page of rank {r}: words {np.flatnonzero(page != want)[:8].tolist()}"
            regions = [(self.buffer_bytes, GUARD_BYTES)]
            if self.slot_guard:
                regions += [(k * self.slot_bytes + self.slot_bytes - self.slot_guard, self.slot_guard)
                            for k in range(2 * self.world)]
            for off, n in regions:
                got = self._read(r, off, n)
                assert np.array_equal(got, self._poison[off:off + n]), \
                    f"{when}: guard at byte {off} of rank {r}'s buffer ({self.describe(off)}) was written"

    def describe(self, offset):
        if offset >= self.buffer_bytes:
            return f"{offset - self.buffer_bytes} bytes behind the buffer"
        k, at = divmod(offset, self.slot_bytes)
        return f"parity {k // self.world}, slot of sender {k % self.world}, byte {at} of {self.slot_bytes}"

    def check_slots(self, when):
        for r in range(self.world):
            got = self.buffers[r].numpy()
            if not np.array_equal(got, self.mirror[r]):
                bad = np.flatnonzero(got != self.mirror[r])
                raise AssertionError(f"{when}: receive buffer of rank {r} differs in {bad.size} bytes, first at {bad[0]} "
                                     f"({self.describe(int(bad[0]))}): {got[bad[0]]:#x}, expected {self.mirror[r][bad[0]]:#x}")
