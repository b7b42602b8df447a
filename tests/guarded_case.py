"""One call of a C entry with every buffer in a guarded buffer (tests/guarded_buffers.py), under each of the two fills:
what tests/test_gpu_buffer_bounds.py (inference) and tests/test_gpu_train_buffer_bounds.py (training) share."""
import numpy as np
import torch

from tests import guarded_buffers as gb

STATUS_F16_RANGE = 1


def dev():
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return torch.device('cuda:0')


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.uint8).reshape(-1)


class Case:
    """The buffers of one call under one fill: inputs (``put``: a copy of the array in a buffer of exactly its size),
    packed images (``packed``) and outputs / workspaces (``new``).  ``done`` synchronises and checks (a) and (e).
    ``guard``: bytes of every buffer's guards.  ``device``: where the buffers live (default: the GPU; the CPU for the
    self-tests of tests/test_guarded_buffers_cpu.py)."""

    def __init__(self, fill, guard=gb.GUARD, device=None):
        self.fill, self.guard, self.g, self.orig, self.status = fill, guard, {}, {}, {}
        self.device = dev() if device is None else torch.device(device)

    def put(self, name, a):
        if a is None:
            return None
        t = (a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).to(self.device).contiguous()
        self.g[name] = gb.place(t, self.fill, name=name, guard=self.guard)
        self.orig[name] = self.g[name].interior_bytes().clone()
        return self.g[name].ptr

    def packed(self, name, image):
        """``image``: (tensor of the pack wrapper, exact byte size, byte offset of the status word or 0)."""
        t, nbytes, off = image
        ptr = self.put(name, t.view(torch.uint8)[:nbytes].clone())
        self.status[name] = off
        return ptr

    def new(self, name, nbytes, misalign=0):
        self.g[name] = gb.GuardedBuffer(nbytes, self.fill, self.device, name, misalign, guard=self.guard)
        return self.g[name].ptr

    def f(self, name, *shape):
        return self.g[name].view(torch.float32, *shape)

    def i(self, name, *shape):
        return self.g[name].view(torch.int32, *shape)

    def u8(self, name, *shape):
        return self.g[name].view(torch.uint8, *shape)

    def i64(self, name, *shape):
        return self.g[name].view(torch.int64, *shape)

    def d(self, name, *shape):
        return self.g[name].view(torch.float64, *shape)

    def done(self):
        if self.device.type == 'cuda':
            torch.cuda.synchronize()
        for g in self.g.values():
            g.check()
        for name, was in self.orig.items():
            now = self.g[name].interior_bytes().clone()
            off = self.status.get(name, 0)
            if off:
                old_w = int(was[off:off + 4].view(torch.int32))
                new_w = int(now[off:off + 4].view(torch.int32))
                assert new_w in (old_w, old_w | STATUS_F16_RANGE), (name, hex(old_w), hex(new_w))
                now[off:off + 4] = was[off:off + 4]
            assert torch.equal(now, was), 'input %s was written' % name
        return self


def both(fn, guard=gb.GUARD, check=False):
    """fn(case) under each fill -> the two finished cases.  ``check``: fn returns the entry's return code (None = 0), and
    one that is not 0 raises."""
    out = []
    for fill in gb.FILLS:
        c = Case(fill, guard)
        rc = fn(c)
        if check:
            ok(rc or 0, getattr(fn, '__name__', 'call'))
        out.append(c.done())
    return out


def same(a, b, names, rows=None, n_rows=None, row_bytes=None, offset=0):
    for n in names:
        gb.same_bits(a.g[n], b.g[n], rows, n_rows, row_bytes, offset)


def eq(c, name, t):
    assert torch.equal(bits(c.g[name].view(torch.uint8 if t.element_size() == 1 else torch.int32)), bits(t)), name


def eqb(c, name, t, nbytes=None):
    """The interior of buffer ``name`` holds exactly the bytes of tensor ``t`` (its first ``nbytes``), whatever the
    element type: uint8 images of odd sizes, int64 counts, float64 results."""
    want = t.contiguous().reshape(-1).view(torch.uint8)
    want = want if nbytes is None else want[:nbytes]
    got = c.g[name].interior_bytes()
    assert got.numel() == want.numel() and torch.equal(got, want.to(got.device)), name


def ok(rc, what):
    from humannerf_amd import _lib
    _lib.check(rc, what)
