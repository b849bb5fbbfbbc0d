"""Lattice operands and the zero-tolerance comparison behind tests/test_exact_lattice.py (numpy only).

Operands drawn from a small lattice make every product, every partial sum in ANY order and every stored value exactly
representable: fp32 accumulation is then exact however a kernel tiles, splits or reorders it, a 16-bit store rounds nothing,
and the device result must equal the float64 oracle as numbers.

  integer lattice   x, dy, kernel in {-1, 0, +1}, bias integers in [-2, 2]           unit 1
  dyadic lattice    x, dy in {k / 8 : |k| <= 8}, kernel in {-1, -1/2, 0, 1/2, 1},
                    bias multiples of 1/2                                             unit 1/64 (x * dy), 1/16 (x * kernel)

Layouts named by `layout_hint` (components r, i, j, k are four contiguous channel blocks):
  'channels_last'   (N, *spatial, 4 C)      'channels_first'  (N, 4 C, *spatial)      'dense'  (M, 4 C)
  'kernel'          (*taps, Cq, 4 F)        'bias'            (4 F,)
"""
import numpy as np

COMPONENTS = 'rijk'
FP32_EXACT = float(2 ** 24)
_EXACT_RANGE = {'bfloat16': 256.0, 'float16': 2048.0, 'float32': FP32_EXACT}


def _dtype_name(dtype):
    return str(dtype).split('.')[-1]


def exact_range(dtype):
    """Every integer of magnitude <= this survives a store in `dtype` (8 / 11 / 24 significand bits); a power-of-two factor
    (dropout 0.5's scale 2, a PReLU slope 1/4) moves only the exponent, so the bound applies to the integer part."""
    return _EXACT_RANGE[_dtype_name(dtype)]


def _signed(rng, shape, density, magnitudes):
    """Magnitudes drawn uniformly from `magnitudes`, non-zero with probability `density`, signs balanced."""
    shape = tuple(int(s) for s in shape)
    mag = np.asarray(magnitudes, dtype=np.float64)[rng.randint(0, len(magnitudes), size=shape)]
    sign = np.where(rng.randint(0, 2, size=shape) == 0, -1.0, 1.0)
    return (mag * sign * (rng.random_sample(shape) < density)).astype(np.float32)


def integer_lattice(rng, shape, density=0.5):
    """float32 values in {-1, 0, +1}: non-zero with probability `density`, both signs equally likely."""
    return _signed(rng, shape, density, [1.0])


def integer_bias(rng, n):
    return rng.randint(-2, 3, size=int(n)).astype(np.float32)


def dyadic_lattice(rng, shape, kind='activation', density=0.5):
    """kind = 'activation' (x, dy): {k / 8 : |k| <= 8};  'kernel': {-1, -1/2, 0, 1/2, 1};  'bias': multiples of 1/2 in [-2, 2]."""
    if kind == 'activation':
        return _signed(rng, shape, density, [k / 8.0 for k in range(1, 9)])
    if kind == 'kernel':
        return _signed(rng, shape, density, [0.5, 1.0])
    if kind == 'bias':
        return (rng.randint(-4, 5, size=shape) / 2.0).astype(np.float32)
    raise ValueError(kind)


def layer_operands(rng, x_shape, w_shape, y_shape=None, use_bias=True, lattice='integer', density=0.5, kernel_density=0.5):
    """Draws in the order x, kernel, bias (and dy when y_shape is given)."""
    if lattice == 'integer':
        draw = lambda s, kind, d: integer_lattice(rng, s, d)
        bias = lambda n: integer_bias(rng, n)
    else:
        draw = lambda s, kind, d: dyadic_lattice(rng, s, kind, d)
        bias = lambda n: dyadic_lattice(rng, (n,), 'bias')
    x = draw(x_shape, 'activation', density)
    w = draw(w_shape, 'kernel', kernel_density)
    b = bias(w_shape[-1]) if use_bias else None
    dy = draw(y_shape, 'activation', density) if y_shape is not None else None
    return x, w, b, dy


def term_bounds(x, w, b, dy, n_out_positions):
    """Operand-only upper bounds of the SUM OF ABSOLUTE TERMS of each output of a layer: a cell of y gathers at most
    taps * 4 Cq products (+ the bias), a cell of dx at most taps * 4 F, a kernel-gradient entry 4 products per output
    position (the four Hamilton blocks its compact entry sits in) and a bias-gradient entry one dy per position."""
    mx = lambda a: 0.0 if a is None else float(np.abs(a).max()) if np.size(a) else 0.0
    taps = int(np.prod(w.shape[:-2]))
    cq, f4 = int(w.shape[-2]), int(w.shape[-1])
    out = dict(y=taps * 4 * cq * mx(x) * mx(w) + mx(b))
    if dy is not None:
        out['dx'] = taps * f4 * mx(dy) * mx(w)
        out['dkernel'] = 4.0 * n_out_positions * mx(x) * mx(dy)
        out['dbias'] = n_out_positions * mx(dy)
    return out


def assert_preconditions(results, dtype, unit=1.0, abs_terms=None, exact_store=True):
    """The case is inside exact arithmetic -- a case that is not FAILS (lower the kernel density; never skip).

    results      name -> float64 array of the ORACLE (never of the code under test)
    unit        the lattice spacing of the results (1 for the integer lattice, 1/64 for the dyadic one)
    abs_terms    name -> upper bound of the sum of absolute terms of any cell (term_bounds): below 2^24 units no partial sum,
                 in any order, can round in an fp32 accumulator
    exact_store  16-bit outputs ('y', 'dx') must also survive the store unrounded: |value| / unit <= exact_range(dtype).
                 False for the dyadic lattice, whose 16-bit outputs are held to ONE rounding instead."""
    name16 = ('y', 'dx')
    for name, v in results.items():
        v = np.asarray(v, dtype=np.float64) / unit
        assert np.array_equal(v, np.rint(v)), '%s: the oracle result leaves the lattice (unit %g)' % (name, unit)
        top = float(np.abs(v).max()) if v.size else 0.0
        limit = exact_range(dtype) if (name in name16 and exact_store) else FP32_EXACT
        assert top <= limit, '%s: max |value| = %g lattice units exceeds the exact range %g of %s: lower the density' \
            % (name, top, limit, _dtype_name(dtype) if name in name16 else 'the fp32 accumulator')
    for name, bound in (abs_terms or {}).items():
        assert bound / unit < FP32_EXACT, '%s: the sum of absolute terms may reach %g lattice units (>= 2^24): fp32 partial ' \
            'sums could round; lower the density' % (name, bound / unit)


def assert_bounds_in_range(bounds, dtype):
    """Operand-only form of the precondition for 16-bit outputs where the full oracle is too slow: `bounds` (name -> the largest
    magnitude the INTEGER part of any cell can reach) must lie inside exact_range(dtype); a power-of-two factor on top of
    the integer part (dropout 0.5's scale) does not enter."""
    for name, b in bounds.items():
        assert b <= exact_range(dtype), '%s: operand bound %g exceeds the exact range %g of %s: lower the kernel density' \
            % (name, b, exact_range(dtype), _dtype_name(dtype))


def expanded_kernel_sums(w):
    """(max absolute column sum, max absolute row sum) of the Hamilton-expanded kernel: a cell of y gathers, over all taps, input
    channels and the four input components, one entry of each compact part p = a ^ b for its filter (column sum: over taps, Cq
    and the four parts at one f); a cell of dx gathers every filter and part at one (tap, cq) row, summed over the taps."""
    a = np.abs(np.asarray(w, dtype=np.float64))
    cq, f = a.shape[-2], a.shape[-1] // 4
    a = a.reshape(-1, cq, 4, f)
    col = a.sum(axis=(0, 1, 2)).max()            # per filter f: all taps, channels, parts
    row = a.sum(axis=(0, 2, 3)).max()            # per input channel: all taps, parts, filters
    return float(col), float(row)


def _unravel(flat, shape, layout):
    """A flat index as a readable position + (row, column-within-component) of the GEMM view of the tensor."""
    idx = tuple(int(i) for i in np.unravel_index(int(flat), shape))
    if layout == 'kernel':
        f = shape[-1] // 4
        tap, cq, ch = idx[:-2], idx[-2], idx[-1]
        row = int(np.ravel_multi_index(idx[:-1], shape[:-1]))
        return 'tap %s, input channel %d, component %s, filter %d' % (tap, cq, COMPONENTS[ch // f], ch % f), row, ch % f
    if layout == 'bias':
        f = shape[0] // 4
        return 'component %s, filter %d' % (COMPONENTS[idx[0] // f], idx[0] % f), None, None
    if layout == 'channels_first':
        n, ch, sp = idx[0], idx[1], idx[2:]
        c = shape[1] // 4
        row = int(np.ravel_multi_index((n,) + sp, (shape[0],) + tuple(shape[2:])))
    elif layout in ('channels_last', 'dense'):
        n, sp, ch = idx[0], idx[1:-1], idx[-1]
        c = shape[-1] // 4
        row = int(np.ravel_multi_index(idx[:-1], shape[:-1]))
    else:
        return 'index %s' % (idx,), None, None
    return 'sample %d, position %s, component %s, channel %d' % (n, sp, COMPONENTS[ch // c], ch % c), row, ch % c


def describe(flat, shape, layout, got, want):
    where, row, col = _unravel(flat, shape, layout)
    tile = '' if row is None else ' [64-row tile %d, 32-column block %d]' % (row // 64, col // 32)
    return '%s%s: got %r, want %r' % (where, tile, float(got.reshape(-1)[flat]), float(want.reshape(-1)[flat]))


def assert_equal_exact(got, want, name, layout_hint=None):
    """Numeric equality, tolerance zero (np.array_equal on float64: +0 == -0).  The failure names the first and the worst
    mismatch by position, with the 64-row tile and 32-column block of the GEMM view for y / dx / dkernel."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, '%s: shape %s != %s' % (name, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(~(got.reshape(-1) == want.reshape(-1)))
    diff = np.abs(got.reshape(-1)[bad] - want.reshape(-1)[bad])
    worst = int(bad[int(np.nanargmax(diff))]) if not np.all(np.isnan(diff)) else int(bad[0])
    raise AssertionError('%s: %d of %d values differ from the exact result\n  first: %s\n  worst: %s'
                         % (name, bad.size, got.size, describe(int(bad[0]), got.shape, layout_hint, got, want),
                            describe(worst, got.shape, layout_hint, got, want)))


def layout_of(rank, kw):
    if rank == 0:
        return 'dense'
    return 'channels_first' if kw.get('data_format', 'channels_last') == 'channels_first' else 'channels_last'
