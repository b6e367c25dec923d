"""Sample-rate conversion, stated in numpy float64 (the yardstick of tests/test_resample_cpu.py and tests/test_hip_resample.py).

g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g, s = min(1, L / M);  h(t) = rolloff sinc(rolloff t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta) for |t| < Z;
    y[m] = s sum_k x[k] h(s (m M / L - k)),  m < ceil(n L / M)                                                         (direct)
    y[m] = sum_{j < T} C[p][j] x[k0 - W + 1 + j],  W = ceil(Z max(L, M) / L), T = 2 W, k0 = floor(m M / L), p = (m M) mod L  (polyphase)
Streaming: S inputs given, E outputs emitted; final: E = ceil(S L / M), else E = max(0, ceil((S - W) L / M)).  `Stream` is a stand-in push loop that keeps a
row's whole history; its `fault` argument seeds one of FAULTS for the tests that show each is caught."""
import math

import numpy as np

ZEROS, BETA, ROLLOFF = 64, 14.769656459379492, 0.9475937167399596
FAULTS = ('phase_off_by_one', 'one_tap_short', 's_dropped', 'floor_n_out', 'early_emit')


def plan(sr_in, sr_out, zeros=ZEROS):
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    if L == 1 and M == 1:
        return L, M, 0, 0
    W = -(-zeros * max(L, M) // L)
    return L, M, W, 2 * W


def proto(t, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    t = np.asarray(t, np.float64)
    r = t / zeros
    inside = np.abs(r) < 1.0
    w = np.i0(beta * np.sqrt(np.where(inside, 1.0 - r * r, 0.0))) / np.i0(beta)
    return np.where(inside, rolloff * np.sinc(rolloff * t) * w, 0.0)


def num_out(n, L, M, fault=None):
    return n * L // M if fault == 'floor_n_out' else -(-n * L // M)


def ready(S, L, M, W, final=False, fault=None):
    if final:
        return num_out(S, L, M, fault)
    e = max(0, -(-(S - W) * L // M)) if S > W else 0
    return e + 1 if fault == 'early_emit' and S > W else e


def table(sr_in, sr_out, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF, fault=None):
    """C [L, T] in float64"""
    L, M, W, T = plan(sr_in, sr_out, zeros)
    big = max(L, M)
    s = 1.0 if fault == 's_dropped' else L / big
    p = np.arange(L)[:, None] + (1 if fault == 'phase_off_by_one' else 0)
    j = np.arange(T)[None, :]
    C = s * proto((p + (W - 1 - j) * L) / big, zeros, beta, rolloff)
    if fault == 'one_tap_short':
        C[:, T - 1] = 0.0
    return C


def _gather(x, L, M, W, T, m):
    """X [len(m), T]: the taps of outputs m, zeros outside the row; and the phases"""
    m = np.asarray(m, np.int64)
    k = (m * M // L)[:, None] - W + 1 + np.arange(T)[None, :]
    ok = (k >= 0) & (k < len(x))
    return np.where(ok, np.asarray(x)[np.clip(k, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0), m * M % L


def polyphase(x, sr_in, sr_out, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF, m=None, C=None, return_bound_sum=False, fault=None):
    """float64 outputs m (default: all) of row x by the polyphase form; with return_bound_sum also sum_j |c_j x_j| per output"""
    x = np.asarray(x, np.float64)
    L, M, W, T = plan(sr_in, sr_out, zeros)
    if m is None:
        m = np.arange(num_out(len(x), L, M, fault))
    if T == 0:
        y = x[np.asarray(m, np.int64)]
        return (y, np.abs(y)) if return_bound_sum else y
    C = table(sr_in, sr_out, zeros, beta, rolloff, fault) if C is None else np.asarray(C, np.float64)
    X, p = _gather(x, L, M, W, T, m)
    prod = C[p] * X
    y = prod.sum(axis=1)
    return (y, np.abs(prod).sum(axis=1)) if return_bound_sum else y


def direct(x, sr_in, sr_out, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """the definition, every k of the row for every m"""
    x = np.asarray(x, np.float64)
    L, M, W, T = plan(sr_in, sr_out, zeros)
    if T == 0:
        return x.copy()
    s = min(1.0, L / M)
    m = np.arange(num_out(len(x), L, M))[:, None]
    k = np.arange(len(x))[None, :]
    return s * (proto(s * (m * M - k * L) / L, zeros, beta, rolloff) * x[None, :]).sum(axis=1)


def _fma32(c, x, acc):
    """float32 fmaf(c, x, acc), correctly rounded: the product of two float32 is exact in float64; the sum is rounded TO ODD there (two-sum gives the exact
    error), and a value rounded to odd at 53 bits rounds to 24 bits as the exact value does"""
    p = c.astype(np.float64) * x.astype(np.float64)
    a = acc.astype(np.float64)
    s = p + a
    bb = s - p
    e = (p - (s - bb)) + (a - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0.0) & even
    toward = np.where((e > 0.0), np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def emulate32(x, C32, L, M, W):
    """the device's chain in numpy float32: one accumulator per output from 0, T fmaf in ascending j, taps outside the row read 0"""
    x = np.asarray(x, np.float32)
    T = 2 * W
    n_out = num_out(len(x), L, M)
    if T == 0:
        return x.copy()
    X, p = _gather(x, L, M, W, T, np.arange(n_out))
    X = X.astype(np.float32)
    Cp = np.asarray(C32, np.float32)[p]
    acc = np.zeros(n_out, np.float32)
    for j in range(T):
        acc = _fma32(Cp[:, j], X[:, j], acc)
    return acc


def bound32(bound_sum, T):
    """a T-term fmaf chain in float32 with once-rounded coefficients against the exact sum"""
    return 1.01 * (T + 2) * 2.0 ** -24 * bound_sum


class Stream:
    """Stand-in push loop of ONE row in float64: keeps the whole history since the restart and evaluates the newly ready outputs from it."""

    def __init__(self, sr_in, sr_out, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF, fault=None):
        self.args, self.fault = (sr_in, sr_out, zeros, beta, rolloff), fault
        self.L, self.M, self.W, self.T = plan(sr_in, sr_out, zeros)
        self.C = table(sr_in, sr_out, zeros, beta, rolloff, fault) if self.T else None
        self.x, self.E = np.zeros(0), 0

    def push(self, x, restart=False, final=False):
        if restart:
            self.x, self.E = np.zeros(0), 0
        self.x = np.concatenate([self.x, np.asarray(x, np.float64)])
        E1 = max(self.E, ready(len(self.x), self.L, self.M, self.W, final, self.fault))
        y = polyphase(self.x, *self.args, m=np.arange(self.E, E1), C=self.C, fault=self.fault)
        self.E = E1
        return y


def upfirdn_reference(x, sr_in, sr_out, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """an independent construction: scipy.signal.upfirdn with hf[j] = s h(s (j - c) / L), c the smallest multiple of M covering the support, read from c / M"""
    from scipy.signal import upfirdn
    L, M, W, T = plan(sr_in, sr_out, zeros)
    s = min(1.0, L / M)
    c = -(-zeros * max(L, M) // M) * M
    hf = s * proto(s * (np.arange(2 * c + 1) - c) / L, zeros, beta, rolloff)
    y = upfirdn(hf, np.asarray(x, np.float64), up=L, down=M)
    n_out = num_out(len(x), L, M)
    return y[c // M: c // M + n_out]


def tone_fit(y, freqs_cycles_per_sample, lo, hi):
    """least-squares amplitudes of the given frequencies in y[lo:hi]"""
    m = np.arange(lo, hi)
    cols = []
    for f in freqs_cycles_per_sample:
        cols += [np.cos(2 * np.pi * f * m), np.sin(2 * np.pi * f * m)]
    coef = np.linalg.lstsq(np.stack(cols, 1), np.asarray(y, np.float64)[lo:hi], rcond=None)[0]
    return np.hypot(coef[0::2], coef[1::2])
