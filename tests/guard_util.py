"""Guard bands for kernel tests (a plain helper module): an output, or an input the product keeps in a LONGER buffer,
sits between two bands of rows -- and, for a leading dimension larger than the row, between columns -- that hold a
known bit pattern.  A store one row or one 8-column chunk past the logical extent then changes a byte the test
compares (assert_bands_untouched), and a read past the extent meets a value that cannot stay hidden: NaN / inf / 1e30
in the result, or a bit of the sticky overflow word.

Patterns are INTEGER bit patterns and every comparison is on integer views, so NaN != NaN cannot hide a change."""
import math

import torch

# fp32: a quiet NaN with a recognisable payload, and a finite value far outside fp16's range (a NaN is invisible to the
# producers' range guards, which compare `|x| >= 65504`; 1e30 is not)
F32_NAN = 0x7FC0BEEF
F32_BIG = 0x7149F2CA   # 1e30
SPLIT_INF = 0x7C00     # fp16 +inf, both planes of a split row

_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16,
             torch.int16: torch.int16, torch.int32: torch.int32, torch.int64: torch.int64, torch.uint8: torch.uint8}


def x8_poison():
    """One (row, 32-column tile) of x8 rows [2, 32] int16: the fp16 plane +inf, the hi8 plane bytes 0x7F and the lo8
    plane bytes 0xFF (both e4m3 NaN)."""
    t = torch.empty(2, 32, dtype=torch.int16)
    t[0] = SPLIT_INF
    t[1, :16] = 0x7F7F
    t[1, 16:] = -1
    return t


def bits(t):
    """integer view of a tensor (same shape)"""
    return t.view(_INT_VIEW[t.dtype])


def fill_bits(t, pattern):
    """fills t with an integer bit pattern of its element size, or with an integer tensor that broadcasts to it"""
    if torch.is_tensor(pattern):
        bits(t).copy_(pattern.to(t.device).expand_as(t))
    else:
        v, n = int(pattern), 8 * t.element_size()
        bits(t).fill_(v - (1 << n) if v >= 1 << (n - 1) and t.dtype != torch.uint8 else v)
    return t


def banded(rows, tail_shape, dtype, device, band=16, poison=0):
    """-> (whole, view): whole [band' + rows + band', *tail_shape] filled with `poison`, view = whole[band':band' + rows]
    (contiguous; band' = `band` rounded up until the view starts on a 16-byte boundary).  poison: an integer bit
    pattern, an integer tensor that broadcasts to the buffer, or a function that fills the buffer."""
    row_bytes = int(math.prod(tail_shape)) * torch.empty(0, dtype=dtype).element_size()
    step = 16 // math.gcd(16, row_bytes)
    band = -(-int(band) // step) * step
    whole = torch.empty((2 * band + rows, *tail_shape), dtype=dtype, device=device)
    if callable(poison):
        poison(whole)
    else:
        fill_bits(whole, poison)
    view = whole[band:band + rows]
    assert view.is_contiguous() and view.data_ptr() % 16 == 0 and whole.shape[0] - band - rows == band
    return whole, view


def band_of(whole, rows):
    return (whole.shape[0] - rows) // 2


def assert_bands_untouched(whole, band, rows, snapshot, c0=None, n=None, what='buffer'):
    """Every byte of `whole` outside rows [band, band + rows) -- and, with c0 / n, outside columns [c0, c0 + n) of those
    rows (2-D buffers with a leading dimension larger than the row) -- equals `snapshot` (whole.clone() before the
    launch)."""
    a, b = bits(whole), bits(snapshot)
    assert a.shape == b.shape
    for name, sl in (('before', slice(0, band)), ('after', slice(band + rows, None))):
        if not torch.equal(a[sl], b[sl]):
            bad = (a[sl] != b[sl]).reshape(a[sl].shape[0], -1).any(dim=1).nonzero().flatten()
            first = int(bad[0]) + (0 if name == 'before' else band + rows)
            raise AssertionError(f'{what}: {bad.numel()} rows of the band {name} the extent were written; first: row '
                                 f'{first - band} relative to the extent of {rows} rows')
    if c0 is not None:
        inner_a, inner_b = a[band:band + rows], b[band:band + rows]
        for name, sl in (('left of', slice(0, c0)), ('right of', slice(c0 + n, None))):
            assert torch.equal(inner_a[:, sl], inner_b[:, sl]), f'{what}: columns {name} the extent were written'
