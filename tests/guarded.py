"""Guarded device buffers for the GPU tests (helper module, not a test file).

One allocation = front guard | body of EXACTLY the declared byte size | back guard.  The guards hold a byte pattern that is compared
byte for byte after a call, so a store past the body is seen instead of landing in the allocator's slack, and the body pointer can be
placed at the minimum alignment an entry accepts (``ptr % 256 == offset``) instead of the 256+ bytes every torch allocation has.

Guard size is a condition of the test, not a measurement: a stray store must land INSIDE a guard.  The callers size them by the
largest unit the kernel under test stores at once (out_guard / SCRATCH_GUARD / IN_GUARD below)."""
import numpy as np
import torch

ALIGN = 256                   # the body pointer is ``offset`` bytes past a multiple of this
IN_GUARD = 64 << 10           # inputs: nothing is stored, a stray read of up to a 64-KiB run stays inside
SCRATCH_GUARD = 1 << 20       # exchange scratch / workspaces: four 256-KiB slots (the largest parked unit is one slot of a 256 x 256 tile)

F16_NAN, F16_ONE = b"\x00\x7e", b"\x00\x3c"   # fp16 0x7e00 / 0x3c00 (little-endian bytes), bf16 NaN 0x7fc0
BF16_NAN, BF16_ONE = b"\xc0\x7f", b"\x80\x3f"
I8_MAX, I8_MIN = b"\x7f", b"\x80"


def out_guard(N, esize):
    """Guard of an [M, N] output: the tallest tile is 256 rows, so rows M .. M + 255 of a last tile written without its row bound
    (or the 256 rows in front of a tile addressed one tile row too low) stay inside."""
    return max(64 << 10, 256 * int(N) * int(esize))


def i32_pattern(v):
    return np.array([v], np.int32).tobytes()


def _pattern(fill):
    if isinstance(fill, (bytes, bytearray)):
        return np.frombuffer(bytes(fill), np.uint8)
    return np.array([int(fill) & 0xFF], np.uint8)


class Guarded:
    """A device buffer of exactly ``nbytes`` with ``guard`` bytes of pattern in front and behind.

    ``fill``: a byte value or a bytes pattern (e.g. F16_NAN); the pattern's phase is taken from the body's start, so multi-byte
    elements line up with the body.  Unless ``init`` (anything numpy can view as bytes, of exactly ``nbytes``) is given the body
    holds the pattern as well.  ``offset``: ``ptr % 256`` of the body (0 = as aligned as the allocation)."""

    def __init__(self, nbytes, fill, init=None, guard=256, offset=0, device="cuda:0"):
        self.n, self.fill, self.guard, self.offset = int(nbytes), fill, int(guard), int(offset)
        assert 0 <= self.offset < ALIGN and self.guard > 0
        total = self.guard + ALIGN + self.n + self.guard
        self.buf = torch.empty(total, dtype=torch.uint8, device=device)
        base = self.buf.data_ptr()
        self.start = self.guard + (self.offset - (base + self.guard)) % ALIGN      # body = buf[start : start + n]
        self.end = self.start + self.n
        self._want = None
        self.set_guards(fill)
        self.set_body(init)

    # ---- filling -------------------------------------------------------------------------------------------------------
    def _tiled(self, lo, hi, fill):
        """Pattern bytes for buffer positions [lo, hi), phase 0 at the body's start."""
        pat = _pattern(fill)
        if pat.size == 1:
            return np.full(hi - lo, pat[0], np.uint8)
        return pat[(np.arange(lo, hi, dtype=np.int64) - self.start) % pat.size]

    def set_guards(self, fill):
        """(Re)fill both guards; the body is left alone."""
        self.guard_fill = fill
        front = torch.from_numpy(self._tiled(0, self.start, fill)).to(self.buf.device)
        back = torch.from_numpy(self._tiled(self.end, self.buf.numel(), fill)).to(self.buf.device)
        self.buf[:self.start] = front
        self.buf[self.end:] = back
        self._want = (front, back)

    def set_body(self, init=None):
        if init is None:
            raw = self._tiled(self.start, self.end, self.fill)
        elif isinstance(init, torch.Tensor):
            self.buf[self.start:self.end] = init.contiguous().reshape(-1).view(torch.uint8).to(self.buf.device)
            return
        else:
            raw = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
        assert raw.size == self.n, (raw.size, self.n)
        if self.n:
            self.buf[self.start:self.end] = torch.from_numpy(np.ascontiguousarray(raw)).to(self.buf.device)

    # ---- reading -------------------------------------------------------------------------------------------------------
    @property
    def ptr(self):
        return self.buf.data_ptr() + self.start

    def body_bytes(self):
        """The body as a device uint8 tensor (a view)."""
        return self.buf[self.start:self.end]

    def body(self, dtype, shape=None):
        b = self.body_bytes().cpu().numpy().copy().view(dtype)
        return b.reshape(shape) if shape is not None else b

    def guard_damage(self):
        """None if both guards still hold their pattern, else a description of the changed bytes: which guard, how many, and
        the first / last offsets relative to the body (negative: in front; >= 0 behind, counted from the body's end)."""
        notes = []
        for name, got, want, origin in (("front", self.buf[:self.start], self._want[0], -self.start),
                                        ("back", self.buf[self.end:], self._want[1], 0)):
            if torch.equal(got, want):
                continue
            bad = torch.nonzero(got != want).reshape(-1)
            notes.append(f"{name} guard: {bad.numel()} bytes changed, offsets {int(bad[0]) + origin} .. {int(bad[-1]) + origin} "
                         f"({'before the body' if origin else 'past the end of the body'}; guard {self.guard} bytes, body {self.n} bytes)")
        return "; ".join(notes) if notes else None

    def get(self, dtype, shape=None):
        """(body as ``dtype`` [shape], whether both guards are intact)."""
        return self.body(dtype, shape), self.guard_damage() is None


def assert_intact(g, what):
    damage = g.guard_damage()
    assert damage is None, f"{what}: an access outside the buffer -- {damage}"
