"""numpy reference of the training-summary statistics (csrc/wn_stats.hip) and the inputs the CPU and GPU tests share.  Nothing here comes from the code
under test: the bucket table is the issue's loop in Python floats (IEEE doubles), the bucket of a value is numpy.searchsorted(limits, x, side='right')
on the float32 value widened to float64, every sum is numpy float64.

Bounds.  A sum of n doubles in ANY order differs from the exact sum by at most gamma(n) * sum |terms|, gamma(n) = (n - 1) u / (1 - (n - 1) u), u = 2^-53
(Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 with the any-order constant).  The terms themselves are exact: a float32 widened to double,
or the product of two such (48 significant bits).  So sum is checked within gamma * sum |x| and sum_squares within gamma * sum x^2 of numpy's float64
values; counts, minimum, maximum and the non-finite counters are exact and are checked for equality.

FAULTS are seeded into THIS reference only (reference_hist(fault=...)): each makes the reference wrong in one way a careless implementation would be, and
the comparison of the tests must tell it from the code under test."""
import numpy as np

N_BUCKETS = 1551
U = 2.0 ** -53
FAULTS = ('side_left', 'float32_table', 'padding_counted', 'nonfinite_binned', 'float32_squares')
SUMMARY = ('num', 'min', 'max', 'sum', 'sum_squares', 'n_nan', 'n_pos_inf', 'n_neg_inf')
SHAPES = [(1, 1, 1), (1, 63, 63), (1, 64, 80), (2, 65, 65), (3, 257, 300), (2, 4099, 4099), (8, 1031, 1040)]      # (B, T, pitch)
TENSOR_COUNTS = (1, 7, 8, 64, 4095, 4096, 4097, 8200, 24576)


def limits():
    pos = []
    v = 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    assert len(pos) == 774
    pos.append(float(np.finfo(np.float64).max))
    return np.array([-p for p in reversed(pos)] + [0.0] + pos, np.float64)


LIMITS = limits()


def gamma(n):
    n = max(int(n), 1)
    return (n - 1) * U / (1.0 - (n - 1) * U)


def edge_values():
    """for every limit with |limit| <= 1e20 the float32 values around it (the nearest float32 and its two neighbours: at least one on either side), +-0, the
    smallest denormals, +-FLT_MAX, NaN and +-inf"""
    f = LIMITS[np.abs(LIMITS) <= 1e20].astype(np.float32)
    inf = np.float32(np.inf)
    vals = np.concatenate([np.nextafter(f, -inf), f, np.nextafter(f, inf)])
    fm, dn = np.finfo(np.float32).max, np.float32(1.4e-45)
    extra = np.array([0.0, -0.0, dn, -dn, fm, -fm, np.nan, np.inf, -np.inf, 1e-12], np.float32)
    return np.concatenate([vals, extra]).astype(np.float32)


def value_sets(B, T, seed=0):
    """the three inputs of the tests as dense float32 [B, T]: the edge values (tiled over the batch), audio-like (tanh of normals), log-scale-like
    (uniform in [-7, 0])"""
    rng = np.random.RandomState(1234 + seed)
    e = edge_values()
    edges = np.resize(rng.permutation(e), (B, T)).astype(np.float32)
    audio = np.tanh(rng.randn(B, T)).astype(np.float32)
    logs = rng.uniform(-7.0, 0.0, (B, T)).astype(np.float32)
    return {'edges': edges, 'audio': audio, 'log_scales': logs}


def ragged_lengths(B, T):
    """row lengths in [0, T]: the first row full, one row empty when there are at least two, the others odd cuts"""
    ln = [T] + [max(0, T - 1 - 37 * i) for i in range(1, B)]
    if B >= 2:
        ln[B // 2] = 0
    return np.array(ln, np.int32)


def with_pitch(x, pitch, lengths=None, poison=np.nan):
    """dense [B, T] -> [B, pitch] with the pitch gap, and everything beyond lengths[b], poisoned"""
    B, T = x.shape
    out = np.full((B, pitch), poison, np.float32)
    out[:, :T] = x
    if lengths is not None:
        for b in range(B):
            out[b, int(lengths[b]):] = poison
    return out


def reference_hist(x, lengths=None, fault=None):
    """x float32 [B, T]; returns the histogram dict of _ext.TrainStats.histogram plus 'abs_sum' and 'n' (elements looked at) for the bounds"""
    with np.errstate(over='ignore'):          # (the float32 faults overflow, as they would in the code they stand for)
        return _reference_hist(x, lengths, fault)


def _reference_hist(x, lengths, fault):
    x = np.asarray(x, np.float32)
    B, T = x.shape
    ln = [T] * B if lengths is None else [int(v) for v in lengths]
    if fault == 'padding_counted':
        ln = [T] * B
    v = np.concatenate([x[b, :ln[b]] for b in range(B)]) if B else np.zeros(0, np.float32)
    fin = np.isfinite(v)
    res = {'n_nan': int(np.isnan(v).sum()), 'n_pos_inf': int(np.isposinf(v).sum()), 'n_neg_inf': int(np.isneginf(v).sum()), 'n': int(v.size)}
    table = LIMITS.astype(np.float32).astype(np.float64) if fault == 'float32_table' else LIMITS
    if fault == 'nonfinite_binned':
        binned = np.nan_to_num(v.astype(np.float64), nan=0.0, posinf=3e38, neginf=-3e38)
        f = binned
    else:
        f = v[fin].astype(np.float64)
        binned = f
    idx = np.searchsorted(table, binned, side='left' if fault == 'side_left' else 'right')
    res['bucket'] = np.bincount(np.minimum(idx, N_BUCKETS - 1), minlength=N_BUCKETS).astype(np.int64)
    res['num'] = int(f.size)
    res['min'] = float(f.min()) if f.size else 0.0
    res['max'] = float(f.max()) if f.size else 0.0
    res['sum'] = float(np.sum(f, dtype=np.float64))
    res['abs_sum'] = float(np.sum(np.abs(f), dtype=np.float64))
    if fault == 'float32_squares':
        res['sum_squares'] = float(np.sum(f.astype(np.float32) ** 2, dtype=np.float32))
    else:
        res['sum_squares'] = float(np.sum(f * f, dtype=np.float64))
    res['sq_sum'] = float(np.sum(f * f, dtype=np.float64))
    return res


def check_hist(got, ref, who=''):
    """the exact parts equal, the sums inside the derived bound; prints the figures before it asserts"""
    g = gamma(ref['num'])
    e_sum, e_sq = abs(got['sum'] - ref['sum']), abs(got['sum_squares'] - ref['sum_squares'])
    b_sum, b_sq = g * ref['abs_sum'], g * ref['sq_sum']
    print('%s: num %d, |sum err| %.3e (bound %.3e), |sum_squares err| %.3e (bound %.3e)' % (who, ref['num'], e_sum, b_sum, e_sq, b_sq))
    assert np.array_equal(np.asarray(got['bucket']), ref['bucket']), (who, 'bucket counts', np.flatnonzero(np.asarray(got['bucket']) != ref['bucket'])[:8])
    for k in ('num', 'n_nan', 'n_pos_inf', 'n_neg_inf'):
        assert int(got[k]) == ref[k], (who, k, got[k], ref[k])
    for k in ('min', 'max'):
        assert float(got[k]) == ref[k], (who, k, got[k], ref[k])
    assert int(np.sum(got['bucket'])) == int(got['num']) == ref['n'] - ref['n_nan'] - ref['n_pos_inf'] - ref['n_neg_inf'], (who, 'sum of the buckets')
    assert e_sum <= b_sum, (who, 'sum', e_sum, b_sum)
    assert e_sq <= b_sq, (who, 'sum_squares', e_sq, b_sq)


def same_hist(a, b):
    """bit identity of two histogram dicts"""
    return (np.array_equal(a['bucket'], b['bucket']) and all(int(a[k]) == int(b[k]) for k in ('num', 'n_nan', 'n_pos_inf', 'n_neg_inf'))
            and all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ('min', 'max', 'sum', 'sum_squares')))


def tensor_table(seed=0, inside=False):
    """a flat float32 buffer holding tensors of TENSOR_COUNTS elements with NaN-poisoned gaps between them, magnitudes from 1e-20 to 1e15 (one decade
    step per tensor, mixed inside the large ones).  inside: a NaN, an inf and a -inf are planted INSIDE three of the tensors.
    Returns flat, [(offset, count)]"""
    rng = np.random.RandomState(77 + seed)
    mags = 10.0 ** np.linspace(-20, 15, len(TENSOR_COUNTS))
    parts, table, off = [], [], 0
    for i, n in enumerate(TENSOR_COUNTS):
        gap = 1 + (i * 5) % 7
        parts.append(np.full(gap, np.nan, np.float32)); off += gap
        t = (rng.randn(n) * mags[i]).astype(np.float32)
        if n >= 4096:
            t[::3] *= np.float32(1e-6)
        if inside and n in (7, 4097, 24576):
            t[n // 2] = {7: np.nan, 4097: np.inf, 24576: -np.inf}[n]
        parts.append(t); table.append((off, n)); off += n
    parts.append(np.full(3, np.nan, np.float32))
    return np.concatenate(parts).astype(np.float32), table


def reference_tensors(flat, table):
    """float64 [nt, 4] = {sum of squares, max |x|, non-finite count, count} and the bound of the first column"""
    out, bound = np.zeros((len(table), 4), np.float64), np.zeros(len(table), np.float64)
    for i, (off, n) in enumerate(table):
        v = np.asarray(flat[off:off + n], np.float32)
        f = v[np.isfinite(v)].astype(np.float64)
        out[i] = (np.sum(f * f, dtype=np.float64), np.abs(f).max() if f.size else 0.0, n - f.size, n)
        bound[i] = gamma(f.size) * out[i, 0]
    return out, bound


def check_tensors(got, ref, bound, who=''):
    got = np.asarray(got, np.float64)
    err = np.abs(got[:, 0] - ref[:, 0])
    print('%s: worst sum-of-squares error / bound %.3f over %d tensors' % (who, float(np.max(err / np.maximum(bound, 1e-300))) if len(err) else 0.0, len(err)))
    assert np.all(err <= bound), (who, 'sum of squares', err, bound)
    assert np.array_equal(got[:, 1:], ref[:, 1:]), (who, 'max |x|, non-finite count or count', got[:, 1:], ref[:, 1:])
