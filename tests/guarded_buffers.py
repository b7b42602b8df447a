"""Guarded buffers: what a test hands a kernel so that a store or a load outside the stated size is seen.

One allocation holds a front guard of 64 KiB, a 256-byte aligned interior of EXACTLY the stated number of bytes, and a
back guard of 64 KiB; all three are filled with one 32-bit pattern before the call.  (``guard``: another size for both
guards, a multiple of 4.)  Afterwards

  - ``check()`` compares both guards with the pattern: a store outside the interior is reported with its byte offset
    from the interior's start or end;
  - ``same_bits(a, b)`` compares the interiors of two buffers that went through the same call under the two FILLS: an
    element the call never wrote keeps each fill and differs, and so does a result that depends on what a buffer held
    before the call or on bytes behind an input's end (inputs sit in guarded buffers too: ``place``);
  - ``rows_hold_fill(rows, ...)`` asserts that rows a contract calls "not written" still hold the pattern, and
    ``bytes_hold_fill(offset, nbytes)`` the same of any byte range (uint8 outputs of odd sizes, a stream's tail).

The two patterns: 0xFFFFFFFF is a NaN as a float and -1 as an index or a count, 0x00000000 is zero.  There is no large
positive pattern on purpose: a stale positive count would drive a kernel off its buffers, and these tests are there to
detect, not to provoke.  64 KiB covers a full tile of the widest output row of the inference kernels (256 samples x 24
bones x 4 bytes = 24 KiB); the training kernels' file asks for 256 KiB: one 128-sample padding tile of a 256-wide fp32
layer is 128 KiB.  Works on CPU tensors as on the device (tests/test_guarded_buffers_cpu.py)."""
import torch

GUARD = 64 * 1024
ALIGN = 256
FILLS = (0xFFFFFFFF, 0x00000000)


def as_i32(pattern):
    """The 32-bit pattern as the int32 value that holds its bits."""
    pattern &= 0xFFFFFFFF
    return pattern - (1 << 32) if pattern >= (1 << 31) else pattern


class GuardViolation(AssertionError):
    pass


class GuardedBuffer:
    """``nbytes`` interior bytes between two guards, everything filled with the 32-bit ``fill``.  ``name`` appears in
    every report.  ``misalign``: extra bytes (a multiple of 4 below 256) by which the interior's start is moved off its
    256-byte alignment, for the entries that must refuse such a pointer.  ``guard``: bytes of each guard."""

    def __init__(self, nbytes, fill, device='cpu', name='buffer', misalign=0, guard=GUARD):
        nbytes, guard = int(nbytes), int(guard)
        assert nbytes >= 0 and 0 <= misalign < ALIGN and misalign % 4 == 0 and guard > 0 and guard % 4 == 0
        self.nbytes, self.fill, self.name, self.guard = nbytes, fill & 0xFFFFFFFF, name, guard
        total = guard + 2 * ALIGN + (nbytes + 3) // 4 * 4 + guard
        self.words = torch.empty(total // 4, dtype=torch.int32, device=device)
        self.words.fill_(as_i32(fill))
        base = self.words.data_ptr()
        assert base % 4 == 0
        self.start = guard + (-(base + guard)) % ALIGN + misalign          # byte offset of the interior
        self.bytes = self.words.view(torch.uint8)
        assert self.start + nbytes + guard <= total and (self.ptr - misalign) % ALIGN == 0

    # ---------------------------------------------------------------- the interior
    @property
    def ptr(self):
        """Address of the interior's first byte (what the kernel is given)."""
        return self.words.data_ptr() + self.start

    @property
    def device(self):
        return self.words.device

    def view(self, dtype=torch.float32, *shape):
        """The interior as a typed tensor of ``shape`` (default: flat); shares the buffer's memory."""
        t = self.bytes[self.start:self.start + self.nbytes].view(dtype)
        return t.view(*shape) if shape else t

    def interior_bytes(self):
        return self.bytes[self.start:self.start + self.nbytes]

    # ---------------------------------------------------------------- the guards
    def _first_bad(self, lo, hi):
        """Byte offset (in the allocation) of the first byte of [lo, hi) that differs from the pattern, or None.  Whole
        words are compared as int32, the ragged bytes next to an interior whose size is no multiple of 4 one by one."""
        pat = self.fill.to_bytes(4, 'little')
        wlo, whi = (lo + 3) // 4, hi // 4
        for b in range(lo, min(wlo * 4, hi)):                       # ragged head (at most 3 bytes)
            if int(self.bytes[b]) != pat[b % 4]:
                return b
        if whi > wlo:
            bad = (self.words[wlo:whi] != as_i32(self.fill)).nonzero()
            if bad.numel():
                w = wlo + int(bad[0])
                got = (int(self.words[w]) & 0xFFFFFFFF).to_bytes(4, 'little')
                return 4 * w + next(i for i in range(4) if got[i] != pat[i])
        for b in range(max(whi * 4, lo), hi):
            if int(self.bytes[b]) != pat[b % 4]:
                return b
        return None

    def violations(self):
        """[(region, offset)]: region 'front' with the (negative) byte offset from the interior's start, region 'back'
        with the byte offset from the interior's end (0 = the first byte past it); the first differing byte of each."""
        out = []
        end = self.start + self.nbytes
        b = self._first_bad(0, self.start)
        if b is not None:
            out.append(('front', b - self.start))
        b = self._first_bad(end, self.bytes.numel())
        if b is not None:
            out.append(('back', b - end))
        return out

    def check(self):
        """Both guards still hold the pattern; else GuardViolation naming the first differing byte."""
        v = self.violations()
        if v:
            raise GuardViolation('; '.join(
                '%s: %s guard written at byte %+d from the interior\'s %s (interior: %d bytes, fill 0x%08X)'
                % (self.name, r, off, 'start' if r == 'front' else 'end', self.nbytes, self.fill) for r, off in v))

    # ---------------------------------------------------------------- the fill inside
    def rows_hold_fill(self, rows, n_rows, row_bytes, offset=0):
        """Rows ``rows`` (a boolean mask of n_rows entries, or indices) of the interior seen as [n_rows][row_bytes] from
        byte ``offset`` on still hold the pattern; row_bytes and offset are multiples of 4.  GuardViolation names the
        first row that does not."""
        assert row_bytes % 4 == 0 and offset % 4 == 0 and offset + n_rows * row_bytes <= self.nbytes
        w0 = (self.start + offset) // 4
        v = self.words[w0:w0 + n_rows * row_bytes // 4].view(n_rows, row_bytes // 4)
        rows = torch.as_tensor(rows, device=self.device)
        idx = rows.nonzero().reshape(-1) if rows.dtype == torch.bool else rows.reshape(-1).long()
        if rows.dtype == torch.bool:
            assert rows.numel() == n_rows
        bad = (v[idx] != as_i32(self.fill)).any(1).nonzero()
        if bad.numel():
            r = int(idx[int(bad[0])])
            raise GuardViolation('%s: row %d (of %d, %d bytes each) was written: it must keep the fill 0x%08X'
                                 % (self.name, r, n_rows, row_bytes, self.fill))

    def holds_fill(self):
        """The whole interior still holds the pattern (an entry that refuses its arguments writes nothing)."""
        b = self._first_bad(self.start, self.start + self.nbytes)
        if b is not None:
            raise GuardViolation('%s: interior written at byte %d: it must keep the fill 0x%08X'
                                 % (self.name, b - self.start, self.fill))

    def bytes_hold_fill(self, offset=0, nbytes=None):
        """Bytes [offset, offset + nbytes) of the interior (default: to its end) still hold the pattern -- any byte
        offset and count: the tail of a byte stream behind its stated length, rows of an odd number of bytes."""
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        assert 0 <= offset and 0 <= nbytes and offset + nbytes <= self.nbytes
        b = self._first_bad(self.start + offset, self.start + offset + nbytes)
        if b is not None:
            raise GuardViolation('%s: byte %d of the interior was written: bytes %d .. %d must keep the fill 0x%08X'
                                 % (self.name, b - self.start, offset, offset + nbytes, self.fill))


def place(tensor, fill, device=None, name='input', guard=GUARD):
    """A guarded buffer of exactly the bytes of ``tensor`` (contiguous), holding a copy of it: a kernel that reads past
    the end of this input reads the fill, and under the other fill it reads something else."""
    t = tensor.contiguous()
    device = t.device if device is None else device
    g = GuardedBuffer(t.numel() * t.element_size(), fill, device, name, guard=guard)
    if t.numel():
        g.view(t.dtype).copy_(t.reshape(-1))
    return g


def same_bits(a, b, rows=None, n_rows=None, row_bytes=None, offset=0):
    """The interiors of ``a`` and ``b`` (two GuardedBuffers of one size, filled differently, after the same call) hold
    the same bytes -- on all of the interior, or on the ``rows`` of its [n_rows][row_bytes] view from byte ``offset``.
    GuardViolation names the first differing byte offset."""
    assert a.nbytes == b.nbytes
    if rows is None:
        x, y = a.interior_bytes(), b.interior_bytes()
    else:
        rows = torch.as_tensor(rows, device=a.device)
        idx = rows.nonzero().reshape(-1) if rows.dtype == torch.bool else rows.reshape(-1).long()
        sl = slice(a.start + offset, a.start + offset + n_rows * row_bytes)
        x = a.bytes[sl].view(n_rows, row_bytes)[idx]
        y = b.bytes[b.start + offset:b.start + offset + n_rows * row_bytes].view(n_rows, row_bytes)[idx.to(b.device)]
    d = (x != y.to(x.device)).reshape(-1).nonzero()
    if d.numel():
        k = int(d[0])
        if rows is not None:
            k = offset + int(idx[k // row_bytes]) * row_bytes + k % row_bytes
        raise GuardViolation('%s: byte %d of the interior differs between the fills 0x%08X and 0x%08X: never written, or '
                             'computed from what a buffer held before the call' % (a.name, k, a.fill, b.fill))
