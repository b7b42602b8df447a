"""tests/guarded_buffers.py on CPU tensors: every violation the GPU tests of tests/test_gpu_buffer_bounds.py rely on is
planted here by hand and must be reported with its offset, and a clean run must pass.  Nothing is planted in a kernel:
this file is the evidence that those checks have teeth."""
import numpy as np
import pytest
import torch

from tests import guarded_buffers as gb

P, B = 777, 7                       # 777 rows of 7 floats: 21 756 bytes, off every 16-byte and 256-byte boundary


def _kernel(buf, rows=None):
    """A well-behaved 'kernel': writes row r of the [P][B] float interior with r + column / 8, on ``rows`` or all."""
    v = buf.view(torch.float32, P, B)
    want = torch.arange(P, dtype=torch.float32)[:, None] + torch.arange(B, dtype=torch.float32)[None] / 8
    if rows is None:
        v.copy_(want)
    else:
        v[rows] = want[rows]


@pytest.mark.parametrize('fill', gb.FILLS)
@pytest.mark.parametrize('nbytes', [0, 1, 3, 4, 255, 256, P * B * 4, 37 * 53])
def test_layout_and_clean_run(nbytes, fill):
    g = gb.GuardedBuffer(nbytes, fill, name='clean')
    assert g.ptr % 256 == 0 and g.start >= gb.GUARD and g.bytes.numel() - g.start - nbytes >= gb.GUARD
    assert g.interior_bytes().numel() == nbytes
    assert bool((g.interior_bytes() == (fill & 0xFF)).all())
    g.interior_bytes().fill_(0x5A)                                  # every interior byte written, nothing else
    assert g.violations() == []
    g.check()
    if nbytes % 4 == 0:
        assert g.view(torch.int32).numel() == nbytes // 4


@pytest.mark.parametrize('fill', gb.FILLS)
def test_write_one_element_past_the_end(fill):
    g = gb.GuardedBuffer(P * B * 4, fill, name='out')
    _kernel(g)
    g.check()
    g.words[(g.start + g.nbytes) // 4] = 0x3F800000                 # element P * B of a float view
    assert g.violations() == [('back', 0 if fill else 2)]           # 1.0f = 00 00 80 3F: over zeros bytes 2, 3 differ
    with pytest.raises(gb.GuardViolation, match=r"out: back guard written at byte \+%d from the interior's end" % (0 if fill else 2)):
        g.check()


@pytest.mark.parametrize('fill', gb.FILLS)
def test_write_one_byte_past_a_ragged_end(fill):
    """An interior of 37 x 53 bytes (a ray mask) ends inside a word: the byte behind it is guard."""
    g = gb.GuardedBuffer(37 * 53, fill, name='mask')
    g.interior_bytes().fill_(1)
    g.check()
    g.bytes[g.start + g.nbytes] = 1
    assert g.violations() == [('back', 0)]
    g.bytes[g.start + g.nbytes] = fill & 0xFF
    g.bytes[g.start + g.nbytes + 2] = 1                             # the last ragged byte of that word
    assert g.violations() == [('back', 2)]


@pytest.mark.parametrize('fill', gb.FILLS)
def test_write_one_element_before_the_start(fill):
    g = gb.GuardedBuffer(P * B * 4, fill, name='out')
    _kernel(g)
    g.words[g.start // 4 - 1] = 0x12345678
    assert g.violations() == [('front', -4)]
    with pytest.raises(gb.GuardViolation, match=r"out: front guard written at byte -4 from the interior's start"):
        g.check()


@pytest.mark.parametrize('fill', gb.FILLS)
def test_write_at_the_far_end_of_the_back_guard(fill):
    g = gb.GuardedBuffer(P * B * 4, fill, name='out')
    _kernel(g)
    g.words[(g.start + g.nbytes + gb.GUARD) // 4 - 1] = 0x12345678  # the last word of the 64 KiB behind the interior
    assert g.violations() == [('back', gb.GUARD - 4)]
    with pytest.raises(gb.GuardViolation, match=r'\+%d from' % (gb.GUARD - 4)):
        g.check()
    h = gb.GuardedBuffer(P * B * 4, fill)
    h.words[0] = 0x12345678                                         # and the far end of the front guard
    assert h.violations() == [('front', -h.start)] and h.start >= gb.GUARD


def test_an_element_never_written_differs_between_the_fills():
    a, b = (gb.GuardedBuffer(P * B * 4, f, name='raw') for f in gb.FILLS)
    for g in (a, b):
        _kernel(g)
    gb.same_bits(a, b)                                              # the clean run
    a, b = (gb.GuardedBuffer(P * B * 4, f, name='raw') for f in gb.FILLS)
    rows = torch.ones(P, dtype=torch.bool)
    rows[P - 1] = False                                             # the 'kernel' forgets its last tail row
    for g in (a, b):
        _kernel(g, rows)
        g.check()                                                   # (no guard sees that)
    with pytest.raises(gb.GuardViolation, match='raw: byte %d of the interior differs' % ((P - 1) * B * 4)):
        gb.same_bits(a, b)
    gb.same_bits(a, b, rows=rows, n_rows=P, row_bytes=B * 4)        # on the rows it wrote the two runs agree
    with pytest.raises(gb.GuardViolation, match='byte %d ' % ((P - 1) * B * 4)):
        gb.same_bits(a, b, rows=torch.tensor([3, P - 1]), n_rows=P, row_bytes=B * 4)


def test_a_result_that_depends_on_bytes_behind_an_input_differs_between_the_fills():
    """An input placed in a guarded buffer: a 'kernel' that reads one element past its end computes something else
    under each fill."""
    x = torch.arange(P, dtype=torch.float32)
    outs = []
    for f in gb.FILLS:
        g = gb.place(x, f, name='x')
        assert torch.equal(g.view(torch.float32), x) and g.nbytes == 4 * P
        o = gb.GuardedBuffer(4 * P, f, name='y')
        wide = g.words[g.start // 4:g.start // 4 + P + 1]          # reads x[p + 1]: one past the end at p = P - 1
        o.view(torch.int32).copy_(wide[:-1] ^ wide[1:])
        g.check(), o.check()
        outs.append(o)
    with pytest.raises(gb.GuardViolation, match='y: byte %d ' % (4 * (P - 1))):
        gb.same_bits(*outs)


@pytest.mark.parametrize('fill', gb.FILLS)
def test_a_row_that_must_stay_untouched(fill):
    g = gb.GuardedBuffer(P * B * 4, fill, name='raw')
    listed = torch.zeros(P, dtype=torch.bool)
    listed[torch.from_numpy(np.random.RandomState(1).permutation(P)[:129])] = True
    _kernel(g, listed)
    g.rows_hold_fill(~listed, P, B * 4)                             # the clean run
    g.rows_hold_fill((~listed).nonzero().reshape(-1), P, B * 4)     # (indices as well as a mask)
    r = int((~listed).nonzero()[5])
    g.view(torch.float32, P, B)[r, B - 1] = 2.5
    with pytest.raises(gb.GuardViolation, match=r'raw: row %d \(of %d, %d bytes each\) was written' % (r, P, B * 4)):
        g.rows_hold_fill(~listed, P, B * 4)
    with pytest.raises(gb.GuardViolation, match='raw: interior written at byte'):
        g.holds_fill()
    h = gb.GuardedBuffer(P * B * 4, fill, name='ws')
    h.holds_fill()                                                  # a refused call leaves everything
    # planes: plane 1 of [2][P][B] starts at byte offset P * B * 4
    k = gb.GuardedBuffer(2 * P * B * 4, fill, name='planes')
    k.view(torch.float32, 2, P, B)[1, 7] = 1.0
    k.rows_hold_fill(torch.ones(P, dtype=torch.bool), P, B * 4)
    with pytest.raises(gb.GuardViolation, match='row 7 '):
        k.rows_hold_fill(torch.ones(P, dtype=torch.bool), P, B * 4, offset=P * B * 4)


BIG_GUARD = 256 * 1024              # the guard of tests/test_gpu_train_buffer_bounds.py


@pytest.mark.parametrize('fill', gb.FILLS)
@pytest.mark.parametrize('nbytes', [0, 3, P * B * 4])
def test_guard_size_argument_layout_and_clean_run(nbytes, fill):
    for guard in (4, gb.GUARD, BIG_GUARD):
        g = gb.GuardedBuffer(nbytes, fill, name='clean', guard=guard)
        assert g.guard == guard and g.ptr % 256 == 0 and guard <= g.start < guard + 256
        assert g.bytes.numel() - g.start - nbytes >= guard
        g.interior_bytes().fill_(0x5A)
        assert g.violations() == []
        g.check()
    assert gb.GuardedBuffer(nbytes, fill).guard == gb.GUARD          # the default stays 64 KiB
    x = torch.arange(P, dtype=torch.float32)
    h = gb.place(x, fill, name='x', guard=BIG_GUARD)
    assert h.guard == BIG_GUARD and h.start >= BIG_GUARD and torch.equal(h.view(torch.float32), x)
    h.check()
    assert gb.place(x, fill).guard == gb.GUARD


@pytest.mark.parametrize('fill', gb.FILLS)
@pytest.mark.parametrize('side', ['back', 'front'])
def test_a_write_one_padding_tile_away_needs_the_larger_guard(side, fill):
    """A 'kernel' that writes one whole 128-sample tile of a 256-wide fp32 layer too many: its last element lies
    128 KiB - 4 bytes behind the interior's end (or as far in front of its start).  The 64 KiB guard does not reach
    there and reports nothing; the 256 KiB guard names the byte."""
    tile = 128 * 256 * 4
    assert gb.GUARD < tile <= BIG_GUARD
    found = {}
    for guard in (gb.GUARD, BIG_GUARD):
        g = gb.GuardedBuffer(P * B * 4, fill, name='acts', guard=guard)
        _kernel(g)
        g.check()                                                   # the clean run passes at either size
        at = g.start + g.nbytes + tile - 4 if side == 'back' else g.start - tile
        if guard == BIG_GUARD:
            g.words[at // 4] = 0x12345678
        else:                   # the 64 KiB allocation ends before that byte: the store lands in somebody else's memory
            assert not 0 <= at < g.bytes.numel()
        found[guard] = g.violations()
    assert found[gb.GUARD] == []
    assert found[BIG_GUARD] == [('back', tile - 4) if side == 'back' else ('front', -tile)]
    with pytest.raises(gb.GuardViolation, match=r"acts: %s guard written at byte %s from" %
                       (side, r'\+%d' % (tile - 4) if side == 'back' else '-%d' % tile)):
        g.check()


def test_misaligned_interior_for_the_refusal_cases():
    g = gb.GuardedBuffer(1024, gb.FILLS[0], misalign=128)
    assert g.ptr % 256 == 128
    g.check()


# ------------------------------------------------------------- what tests/test_gpu_aux_buffer_bounds.py added
@pytest.mark.parametrize('fill', gb.FILLS)
def test_a_byte_range_that_must_stay_untouched(fill):
    """A byte stream of 1001 bytes whose first 613 are written: the tail holds the fill; a byte written at the stated
    length, or the last one, is named."""
    g = gb.GuardedBuffer(1001, fill, name='stream')
    g.interior_bytes()[:613] = 0x5A
    g.bytes_hold_fill(613)
    g.bytes_hold_fill(613, 0), g.bytes_hold_fill(1001), g.bytes_hold_fill(700, 3)
    with pytest.raises(gb.GuardViolation, match='stream: byte 612 of the interior was written'):
        g.bytes_hold_fill(612)
    g.interior_bytes()[1000] = 0x5A
    with pytest.raises(gb.GuardViolation, match='stream: byte 1000 of the interior was written'):
        g.bytes_hold_fill(613)
    g.bytes_hold_fill(613, 1000 - 613)
    g.check()
    gb.GuardedBuffer(0, fill).bytes_hold_fill()                     # a zero-byte buffer holds it trivially


@pytest.mark.parametrize('fill', gb.FILLS)
def test_case_views_of_bytes_int64_and_float64(fill):
    """Case on CPU tensors: inputs of an odd number of bytes sit in exactly that many, int64 and float64 views address
    the interior, eqb compares bytes of any type, and done() sees a written input and a written guard."""
    from tests.guarded_case import Case, eqb
    c = Case(fill, guard=1024, device='cpu')
    img = np.arange(5 * 7 * 3, dtype=np.uint8).reshape(5, 7, 3)                 # 105 bytes
    c.put('img', img)
    c.put('off', np.array([0, 3, 1 << 40], np.int64))
    c.put('empty', np.zeros((0, 3), np.float32))
    c.new('out8', 35), c.new('cnt', 16), c.new('D', 24)
    assert c.g['img'].nbytes == 105 and c.g['empty'].nbytes == 0 and c.g['img'].ptr % 256 == 0
    assert torch.equal(c.u8('img', 5, 7, 3), torch.from_numpy(img)) and int(c.i64('off')[2]) == 1 << 40
    c.u8('out8', 5, 7).copy_(torch.arange(35, dtype=torch.uint8).view(5, 7))
    c.i64('cnt').copy_(torch.tensor([7, -1]))
    c.d('D').copy_(torch.tensor([0.5, float('inf'), float('nan')], dtype=torch.float64))
    c.done()
    eqb(c, 'out8', torch.arange(35, dtype=torch.uint8))
    eqb(c, 'cnt', torch.tensor([7, -1]))
    eqb(c, 'D', torch.tensor([0.5, float('inf'), float('nan')], dtype=torch.float64))          # bytes: a NaN equals itself
    eqb(c, 'cnt', torch.tensor([7, -1, 9]), nbytes=16)                                         # (the first bytes of a longer one)
    with pytest.raises(AssertionError, match='cnt'):
        eqb(c, 'cnt', torch.tensor([7, 5]))
    with pytest.raises(AssertionError, match='out8'):
        eqb(c, 'out8', torch.arange(36, dtype=torch.uint8))                                   # another size
    c.u8('img')[104] ^= 1                                                                     # the last byte of an input
    with pytest.raises(AssertionError, match='input img was written'):
        c.done()
    c.u8('img')[104] ^= 1
    c.g['out8'].bytes[c.g['out8'].start + 35] ^= 0xFF                                         # one byte behind an odd-sized output
    with pytest.raises(gb.GuardViolation, match=r"out8: back guard written at byte \+0 "):
        c.done()
