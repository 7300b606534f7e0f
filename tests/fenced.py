"""Operands inside fences, for both backends of tests/kernel_backend.py (numpy views on `emu`, tensor views with an offset
data_ptr() on `hip`).

fenced(be, array, misalign=0) places `array` in the middle of a larger buffer of its own and returns a view with the
array's shape whose address is `misalign` 4-byte elements past a 16-byte boundary. Everything else in the buffer is
fence: a NaN with a payload no arithmetic produces for float types, the sentinel INT_FENCE for integer types. With `ld`
and `off` the 2-D array is the column block [:, off:off + cols] of a matrix of row stride `ld` (the dense layer's W and
grad_W); the matrix's other columns are fence too, and `misalign` then speaks of the matrix's first element, as it does
for the callers that hand the library W + off.

A kernel that reads outside its operand meets a NaN (0 * NaN is NaN: a zero-filled K column does not hide it); one that
writes outside it is caught by assert_fence_intact, which compares every fence element bit for bit. On the GPU the
fences also keep such a stray access inside memory the test owns: at least max(64, one row stride) elements on both
sides.

fenced_bytes(be, nbytes, fill) does the same for the buffers whose size the library dictates (workspaces, plans,
descriptor blocks): a uint8 view of exactly `nbytes` bytes, `misalign` bytes past an `align`-byte boundary, between two
fences of the float fence pattern that are each at least as large as the buffer and never under 4 KiB, so that an overrun
by a whole tile row still lands in memory the test owns. `fill` is what the buffer holds before the call (FILLS).
"""
import numpy as np

FLOAT_FENCE_BITS = {4: 0x7FC5AFE5, 8: 0x7FF85AFE5AFE5AFE}     # quiet NaNs with a payload
INT_FENCE = -77                                              # small: an index made of it stays near the buffer


def _bits_dtype(dtype):
    return np.dtype('i%d' % np.dtype(dtype).itemsize)


def fence_bits(dtype):
    """The fence of `dtype` as the integer of the same width."""
    dtype = np.dtype(dtype)
    if np.issubdtype(dtype, np.floating):
        return np.array(FLOAT_FENCE_BITS[dtype.itemsize], dtype='u%d' % dtype.itemsize).view(_bits_dtype(dtype))[()]
    return _bits_dtype(dtype).type(INT_FENCE)


def _layout(shape, ld, off):
    """(elements the matrix spans, fence elements on each side, flat indices of the operand inside the span)."""
    n = int(np.prod(shape, dtype=np.int64))
    if ld is None:
        stride = int(shape[-1]) if len(shape) else 1
        return n, max(64, stride), np.arange(n, dtype=np.int64)
    rows, cols = shape
    assert 0 <= off and off + cols <= ld, 'the block must lie inside a row'
    idx = (np.arange(rows, dtype=np.int64)[:, None] * ld + off + np.arange(cols, dtype=np.int64)[None, :]).reshape(-1)
    return rows * ld, max(64, ld), idx


def fenced(be, array, misalign=0, ld=None, off=0):
    array = np.asarray(array)
    dtype, item = array.dtype, array.dtype.itemsize
    assert 0 <= misalign <= 3 and (misalign == 0 or item == 4), 'misalign counts 4-byte elements'
    assert ld is None or array.ndim == 2
    span, fence, _ = _layout(array.shape, ld, off)
    slack = 16 // item + (4 if item == 4 else 0)              # room to choose the address
    total = fence + slack + span + fence
    image = np.full(total, fence_bits(dtype), dtype=_bits_dtype(dtype)).view(dtype)
    buf = be.put(image)
    base = be.ptr(buf)
    assert base % item == 0
    start = fence
    while (base + start * item) % 16 != 4 * misalign:
        start += 1
    assert start + span + fence <= total
    if ld is None:
        view = buf[start:start + span].reshape(array.shape)
    else:
        view = buf[start:start + span].reshape(array.shape[0], ld)[:, off:off + array.shape[1]]
    if be.name == 'emu':
        view[...] = array
    else:
        view.copy_(be.torch.from_numpy(np.ascontiguousarray(array)))
    assert (be.ptr(view) - 4 * off * (ld is not None)) % 16 == 4 * misalign
    assert tuple(view.shape) == tuple(array.shape)
    return view


BYTE_FENCE = np.array([FLOAT_FENCE_BITS[4]], dtype='<u4').view(np.uint8)      # the float fence, byte by byte
# what a library-sized buffer may hold when the call starts: zeros; the fence NaN; every bit set (-1 as an integer, an
# all-ones counter, a negative NaN as a float); 1.0f (a large positive integer; an accumulator that is never cleared stays
# finite and gives a visibly wrong sum); and bytes that differ from word to word, 4099 of them repeated (a prime: no two of
# a layout's planes start alike -- two counters that are subtracted from each other cancel any uniform fill)
FILLS = {'zeros': np.zeros(4, dtype=np.uint8), 'nan': BYTE_FENCE, 'ones': np.full(4, 0xFF, dtype=np.uint8),
         'one_f32': np.array([0x3F800000], dtype='<u4').view(np.uint8),
         'noise': np.random.RandomState(4099).randint(0, 256, size=4099).astype(np.uint8)}
MIN_BYTE_FENCE = 4096


def _pattern(word, n):
    return np.resize(word, n) if n else np.zeros(0, dtype=np.uint8)


def fenced_bytes(be, nbytes, fill, align=256, misalign=0):
    nbytes = int(nbytes)
    assert nbytes >= 0 and align >= 4 and align % 4 == 0 and 0 <= misalign < align
    fence = max(nbytes, MIN_BYTE_FENCE)
    fence += -fence % 4
    total = fence + align + misalign + nbytes + fence
    buf = be.put(_pattern(BYTE_FENCE, total))
    base = be.ptr(buf)
    assert base % 4 == 0
    start = fence
    while (base + start) % align != misalign:
        start += 1
    assert start + nbytes + fence <= total
    view = buf[start:start + nbytes]
    if be.name == 'emu' and nbytes == 0:                # (an empty slice forgets where it starts)
        view = np.ndarray((0,), np.uint8, buffer=buf, offset=start)
    image = _pattern(FILLS[fill], nbytes)               # (the fill's words start at the view's first byte)
    if be.name == 'emu':
        view[...] = image
    else:
        view.copy_(be.torch.from_numpy(image))
    assert (nbytes == 0 or be.ptr(view) == base + start) and int(view.shape[0]) == nbytes
    return view


def _base_and_start(be, view):
    if be.name == 'emu':
        base = view.base
        assert base is not None and base.ndim == 1 and base.base is None, 'not a view made by fenced()'
        start = (view.ctypes.data - base.ctypes.data) // view.dtype.itemsize
        return np.array(base), int(start), view.shape, [s // view.dtype.itemsize for s in view.strides]
    base = view._base
    assert base is not None and base.dim() == 1 and base._base is None, 'not a view made by fenced()'
    be.torch.cuda.synchronize()
    return base.cpu().numpy(), int(view.storage_offset()), tuple(view.shape), list(view.stride())


def assert_fence_intact(be, view, what=''):
    """Every element of the buffer fenced() made for `view` that is not the view's own still holds the fence, to the bit."""
    whole, start, shape, strides = _base_and_start(be, view)
    inside = np.zeros(whole.shape[0], dtype=bool)
    idx = np.full(shape, start, dtype=np.int64)
    for axis, (n, s) in enumerate(zip(shape, strides)):
        sh = [1] * len(shape)
        sh[axis] = n
        idx = idx + (np.arange(n, dtype=np.int64) * s).reshape(sh)
    inside[idx.reshape(-1)] = True
    if whole.dtype == np.uint8:                         # fenced_bytes(): the float fence byte by byte, from the base on
        bad = np.nonzero(~inside & (whole != _pattern(BYTE_FENCE, whole.shape[0])))[0]
    else:
        bits = whole.view(_bits_dtype(whole.dtype))
        bad = np.nonzero(~inside & (bits != fence_bits(whole.dtype)))[0]
    assert bad.size == 0, '%s: %d fence elements overwritten, the first at %+d from the operand' % (
        what, bad.size, int(bad[0]) - start)
