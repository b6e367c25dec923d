"""Float64 reference of the pitch check (csrc/wn_pitch.h), the error bound of the float32 evaluation, the per-frame decidability test and f0 tolerance, the
signal generator of the pitch tests, and the float64 comparison of two tracks.  Test infrastructure: nothing here is loaded by the product.

The estimator (include/wavenet_mi355.h, "pitch check"): with L = W + tau_max, frame f covers the signal indices [f hop - L // 2, f hop - L // 2 + L), zeros
outside [0, n): x_0 ... x_{L-1};  d(tau) = sum_{j < W} (x_j - x_{j+tau})^2,  c(tau) = sum_{k <= tau} d(k),  d'(tau) = d(tau) tau / c(tau) (1 where c = 0,
d'(0) = 1).

The bound  beta = (W + tau_max + 8) 2^-24,  relative, on every d'(tau)
    u = 2^-24.  A term of d is e^2 with e = fl(x_j - x_{j+tau}): one rounding, squared exactly inside the fused multiply-add, whose sum is rounded once
    per step: a term is touched by at most three kinds of rounding -- its own difference (twice, as it is squared) and the roundings of the running sum
    after it, of which there are at most W.  All terms are non-negative, so the relative error of a sum is at most the largest relative error of a term
    plus one u per addition: d is within (W + 2) u.  The prefix c adds at most tau_max non-negative values, tau_max u more; the product d tau and the
    division are one rounding each.  Counting the roundings a single value passes through -- W + 2 for d, tau_max for the prefix, 2 for the product and
    the quotient, and 4 u of slack for the second-order terms -- gives beta.  This is the figure the tests hold the device to.  It is NOT the rigorous
    worst case of the quotient: numerator and denominator each carry up to (W + 2) u of independent error, so the worst case is (2 W + tau + 5) u, about
    1.7 beta at the production geometry.  beta is the tighter of the two, so the test asks more than the worst case would; it holds with a wide margin
    because rounding errors of one sign do not line up over a thousand terms: a plain float32 numpy evaluation and the device's order both stay below
    about 0.15 beta on the test signals (the GPU test records the worst ratio in profiles/pitch_parity.json).

Decidability of a frame (decide): the pick compares d' values with the threshold and with each other.  A frame is decidable when every comparison the
reference's pick made has a margin |x - y| > 2 beta max(|x|, |y|) -- each side moves by at most beta times itself, so a float32 evaluation inside the
bound makes the same decision -- and, voiced, den > 64 beta max(a, b, c).  The comparisons: every d'(tau) against the threshold from tau_min up to and
including the first crossing (all of the search range for an unvoiced frame), and every step of the walk including the one that ended it.

The f0 tolerance of a decidable voiced frame (f0_tolerance): a, b, c are each within beta' = beta + 4 u of exact (4 u: the float32 roundings of forming
num = a - c and den = (a - 2 b) + c, bounded by u times the magnitudes involved).  So |num' - num| <= E_n = beta' (a + c), |den' - den| <= E_d = beta'
(a + 2 b + c) <= 4 beta' max(a, b, c) < den / 16 by decidability, and with delta = num / (2 den):
    |delta' - delta| <= D = ( E_n + |num| E_d / den ) / ( 2 (den - E_d) ) + 2 u |delta|                 (the quotient's and the halving's roundings)
f0 = sr / (tau + delta), with one rounding for the sum and one for the quotient (sr and tau are exact):
    |f0' - f0| <= f0 ( D / (tau + delta - D) + 4 u ).
"""
import numpy as np

U = 2.0 ** -24
GEOMETRIES = {
    'A': dict(sample_rate=2000, hop=16, window=64, tau_min=5, tau_max=40, threshold=0.15),
    'P': dict(sample_rate=22050, hop=275, window=1024, tau_min=44, tau_max=368, threshold=0.15),      # the production geometry: 60 ... 500 Hz at 22.05 kHz
    'M': dict(sample_rate=6400, hop=32, window=128, tau_min=8, tau_max=128, threshold=0.15),          # tau_max an exact multiple of the wave width
}
COLUMNS = ('frames', 'voiced_a', 'voiced_b', 'both', 'vuv_error', 'gpe', 'f0_rmse_cents', 'f0_bias_cents', 'f0_fine_rmse_cents')


def beta(geo):
    return (geo['window'] + geo['tau_max'] + 8) * U


def span(geo):
    return geo['window'] + geo['tau_max']


def num_frames(n, geo):
    return 1 + int(n) // geo['hop']


def frame_matrix(x, geo, dtype=np.float64):
    """[F, L]: row f = the signal indices [f hop - L // 2, f hop - L // 2 + L) of x, zeros outside"""
    x = np.asarray(x, dtype=dtype).reshape(-1)
    L, hop, F = span(geo), geo['hop'], num_frames(len(x), geo)
    pad = np.concatenate((np.zeros(L // 2, dtype), x, np.zeros((F - 1) * hop + L, dtype)))
    idx = np.arange(F)[:, None] * hop + np.arange(L)[None, :]
    return pad[idx]


def dprime(x, geo, dtype=np.float64):
    """d'[F, tau_max + 1] by the definition.  dtype float32: numpy's own (pairwise) float32 sums, the yardstick of the bound"""
    X = frame_matrix(x, geo, dtype)
    W, TM = geo['window'], geo['tau_max']
    d = np.zeros((X.shape[0], TM + 1), dtype)
    for tau in range(1, TM + 1):
        e = X[:, :W] - X[:, tau:tau + W]
        d[:, tau] = (e * e).sum(axis=1, dtype=dtype)
    c = np.cumsum(d, axis=1, dtype=dtype)
    taus = np.arange(TM + 1).astype(dtype)
    out = np.ones_like(d)
    np.divide(d * taus, c, out=out, where=c > 0)
    out[:, 0] = 1
    return out


def dprime_brute(x, geo):
    """the same by a double loop over frames and lags and a Python sum over j: nothing shared with dprime but the definition"""
    x = [float(v) for v in np.asarray(x, np.float64).reshape(-1)]
    n, W, TM, L, hop = len(x), geo['window'], geo['tau_max'], span(geo), geo['hop']
    out = np.ones((num_frames(n, geo), TM + 1))
    for f in range(out.shape[0]):
        s0 = f * hop - L // 2
        fr = [x[s] if 0 <= s < n else 0.0 for s in range(s0, s0 + L)]
        c = 0.0
        for tau in range(1, TM + 1):
            d = 0.0
            for j in range(W):
                e = fr[j] - fr[j + tau]
                d += e * e
            c += d
            out[f, tau] = d * tau / c if c > 0 else 1.0
    return out


def dprime_autocorr(x, geo):
    """the same through the float64 identity d(tau) = E(0) + E(tau) - 2 r(tau), E(t) = sum_j x_{j+t}^2, r(tau) = sum_j x_j x_{j+tau}"""
    X = frame_matrix(x, geo)
    W, TM = geo['window'], geo['tau_max']
    d = np.zeros((X.shape[0], TM + 1))
    e0 = (X[:, :W] ** 2).sum(axis=1)
    for tau in range(1, TM + 1):
        d[:, tau] = e0 + (X[:, tau:tau + W] ** 2).sum(axis=1) - 2.0 * (X[:, :W] * X[:, tau:tau + W]).sum(axis=1)
    c = np.cumsum(d, axis=1)
    out = np.ones_like(d)
    np.divide(d * np.arange(TM + 1), c, out=out, where=c > 0)
    out[:, 0] = 1
    return out


def pick(dp, geo):
    """The pick of one frame from d'[tau_max + 1] -> dict(voiced, tau, delta, f0, ap, pairs): pairs lists every comparison made, (x, y)"""
    lo, hi, th = geo['tau_min'], geo['tau_max'] - 1, float(geo['threshold'])
    pairs, at = [], -1
    for tau in range(lo, hi + 1):
        pairs.append((float(dp[tau]), th))
        if dp[tau] < th:
            at = tau
            break
    if at < 0:
        return dict(voiced=False, tau=0, delta=0.0, f0=0.0, ap=float(np.min(dp[lo:hi + 1])), pairs=pairs)
    while at + 1 <= hi:
        pairs.append((float(dp[at + 1]), float(dp[at])))
        if not dp[at + 1] < dp[at]:
            break
        at += 1
    a, b, c = float(dp[at - 1]), float(dp[at]), float(dp[at + 1])
    den = a - 2.0 * b + c
    delta = 0.5 * (a - c) / den if den > 0 else 0.0
    return dict(voiced=True, tau=at, delta=delta, f0=geo['sample_rate'] / (at + delta), ap=b, pairs=pairs, abc=(a, b, c), den=den)


def decide(p, geo):
    """is the frame of pick() p decidable at the bound beta?"""
    bt = beta(geo)
    if any(abs(x - y) <= 2.0 * bt * max(abs(x), abs(y)) for x, y in p['pairs']):
        return False
    return (not p['voiced']) or p['den'] > 64.0 * bt * max(p['abc'])


def f0_tolerance(p, geo):
    """absolute tolerance of a decidable voiced frame's f0 (the module docstring derives it)"""
    a, b, c = p['abc']
    bp = beta(geo) + 4.0 * U
    e_n, e_d, den, num = bp * (a + c), bp * (a + 2.0 * b + c), p['den'], a - c
    D = (e_n + abs(num) * e_d / den) / (2.0 * (den - e_d)) + 2.0 * U * abs(p['delta'])
    return p['f0'] * (D / (p['tau'] + p['delta'] - D) + 4.0 * U)


def track(x, geo):
    """the float64 reference of one row: d' [F, tau_max + 1] and the list of pick() dicts, each with 'decidable' and, voiced and decidable, 'tol'"""
    dp = dprime(x, geo)
    picks = []
    for f in range(dp.shape[0]):
        p = pick(dp[f], geo)
        p['decidable'] = decide(p, geo)
        if p['voiced'] and p['decidable']:
            p['tol'] = f0_tolerance(p, geo)
        picks.append(p)
    return dp, picks


def compare(f0_a, f0_b, frames):
    """float64 comparison of two tracks [B, >= frames[b]] -> [B, 9], columns COLUMNS"""
    out = np.zeros((len(frames), 9))
    for r, n in enumerate(frames):
        a, b = np.asarray(f0_a[r][:n], np.float64), np.asarray(f0_b[r][:n], np.float64)
        va, vb = a > 0, b > 0
        both = va & vb
        ratio = b[both] / a[both]
        cents = 1200.0 * np.log2(ratio)
        gross = np.abs(ratio - 1.0) > 0.2
        nb = int(both.sum())
        out[r, :4] = n, va.sum(), vb.sum(), nb
        out[r, 4] = (va != vb).sum() / n if n else 0.0
        if nb:
            out[r, 5] = gross.sum() / nb
            out[r, 6] = np.sqrt(np.mean(cents ** 2))
            out[r, 7] = np.mean(cents)
        if nb - gross.sum() > 0:
            out[r, 8] = np.sqrt(np.mean(cents[~gross] ** 2))
    return out


# ---- signals
def tone(geo, n, f0, harmonics=3, phase=0.0):
    """a steady tone of `harmonics` harmonics (amplitudes 1, 1/2, 1/3 ...), float32"""
    t = np.arange(n) / float(geo['sample_rate'])
    x = sum(np.sin(2 * np.pi * f0 * (h + 1) * t + phase * (h + 1)) / (h + 1) for h in range(harmonics))
    return (0.3 * x).astype(np.float32)


def signal(geo, n, seed):
    """n samples that alternate vibrato harmonic segments with 1 % noise, noise segments and silence, seeded; float32.  Segment lengths are 1.2 ... 2.5 frame
    spans; f0 lies inside the search range with a margin, the harmonics below Nyquist"""
    rng = np.random.RandomState(seed)
    sr, L = float(geo['sample_rate']), span(geo)
    out = np.zeros(n, np.float64)
    at, kind = 0, int(rng.randint(3))
    while at < n:
        m = min(n - at, int(rng.uniform(1.2, 2.5) * L))
        if kind == 0:
            f0 = rng.uniform(1.25 * sr / geo['tau_max'], 0.8 * sr / geo['tau_min'])
            t = np.arange(m) / sr
            ph = 2 * np.pi * f0 * (t - 0.02 / (2 * np.pi * 5.0) * np.cos(2 * np.pi * 5.0 * t)) + rng.uniform(0, 2 * np.pi)      # 2 % vibrato at 5 Hz
            nh = max(1, min(3, int(0.45 * sr / f0)))
            seg = sum(np.sin((h + 1) * ph) / (h + 1) for h in range(nh))
            out[at:at + m] = rng.uniform(0.1, 0.5) * (seg + 0.01 * rng.randn(m))
        elif kind == 1:
            out[at:at + m] = rng.uniform(0.05, 0.3) * rng.randn(m)
        at += m
        kind = (kind + 1 + int(rng.randint(2))) % 3
    return out.astype(np.float32)


TILE = 8          # wn_pitch_frame_tile(): the GPU test asserts it is this, the lengths below sit around its multiples
LONGEST = {'A': 4000, 'P': 6000, 'M': 3000}      # samples of the longest row (P: below 0.3 s)
_CASES = {}


def case_lengths(name):
    """row lengths of geometry `name`: 0, 1, hop - 1, hop, hop + 1, L - 1, L; F = TILE - 1, TILE, TILE + 1 and 2 TILE + 1 frames; one long row"""
    geo = GEOMETRIES[name]
    hop, L = geo['hop'], span(geo)
    return [0, 1, hop - 1, hop, hop + 1, L - 1, L] + [(F - 1) * hop + hop // 2 for F in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)] + [LONGEST[name]]


def case(name):
    """(geo, lengths, rows, refs) of geometry `name`, built once: rows[b] float32 [lengths[b]] = signal(seed 100 + b), refs[b] = track(rows[b])"""
    if name not in _CASES:
        geo = GEOMETRIES[name]
        lengths = case_lengths(name)
        rows = [signal(geo, n, 100 + b) for b, n in enumerate(lengths)]
        _CASES[name] = (geo, lengths, rows, [track(r, geo) for r in rows])
    return _CASES[name]


def batch(rows, ld=None, order=None, fill=np.nan):
    """[B, ld] float32 holding rows[order[b]] with `fill` beyond every row's length"""
    order = list(range(len(rows))) if order is None else list(order)
    ld = max(len(rows[i]) for i in order) if ld is None else ld
    out = np.full((len(order), max(ld, 1)), fill, np.float32)
    for b, i in enumerate(order):
        out[b, :len(rows[i])] = rows[i]
    return out


def check_case(name, dp, f0, ap, who, order=None):
    """every row of an evaluation of case(name) (in `order`) under check_row; the cap on excused frames: at most 1 % of the case's.  Returns the worst
    d' error / bound"""
    geo, lengths, rows, refs = case(name)
    order = list(range(len(rows))) if order is None else list(order)
    worst, frames, excused = 0.0, 0, 0
    for b, i in enumerate(order):
        w, F, ex = check_row(geo, refs[i][0], refs[i][1], dp[b], f0[b], ap[b], (who, name, i))
        worst, frames, excused = max(worst, w), frames + F, excused + ex
    assert excused * 100 <= frames, (who, name, 'excused', excused, 'of', frames)
    return worst, frames, excused


# An exact tie inside the walk.  Small-integer samples make every d an exact integer, so d'(9) = d'(10) = 2 / 5 of frame 7 are one real number and round alike
# in any precision; d'(8) = 54 / 43 is above the threshold 1 / 2, and d'(11) = 143 / 388 lies below the tie.  The walk steps only on a strict decrease: it
# stays at tau* = 9 (f0 = 1000 / 9.5), where a walk that stepped on equality would go on to 11 (f0 = 94.9).  The decidability test excuses ties, so the
# signals above cannot show this; found by a seeded search over random integer signals in exact rational arithmetic.
TIE_GEO = dict(sample_rate=1000, hop=4, window=8, tau_min=2, tau_max=12, threshold=0.5)
TIE_SIGNAL = np.array([-2, -2, -2, 0, 2, 0, 2, 2, 0, 0, 2, -1, -2, 0, 1, 0, 1, 2, 2, -1, 1, -1, -2, -2, 1, 1, -2, 2, 1, 2, -1, -1, -2, -2, 0, 1, -1, -2, -1, 0], np.float32)
TIE_FRAME, TIE_TAU = 7, 9


def check_tie(f0, dp, who):
    """f0 [F] and dp [F, 13] of an evaluation of TIE_SIGNAL: the tie is exact, the walk stopped at it"""
    ref_dp, picks = track(TIE_SIGNAL, TIE_GEO)
    p = picks[TIE_FRAME]
    assert ref_dp[TIE_FRAME, 9] == ref_dp[TIE_FRAME, 10] == 0.4 and ref_dp[TIE_FRAME, 11] < 0.4 and p['tau'] == TIE_TAU and abs(p['f0'] - 1000 / 9.5) < 1e-9
    assert dp[TIE_FRAME][9] == dp[TIE_FRAME][10] == np.float32(0.4), (who, dp[TIE_FRAME])
    assert abs(float(f0[TIE_FRAME]) - p['f0']) <= 1e-5 * p['f0'], (who, float(f0[TIE_FRAME]), p['f0'])


def check_row(geo, ref_dp, picks, dp, f0, ap, who):
    """One row of an evaluation (hook or device: float32 dp [F, tau_max + 1], f0, ap [F]) against its float64 reference under the assertions of the
    pitch tests: every d' within beta |ref|; on decidable frames the voiced flag, tau* and f0 inside its tolerance.  Returns (worst d' error / bound,
    frames, excused frames)."""
    F, bt, sr = ref_dp.shape[0], beta(geo), float(geo['sample_rate'])
    dp, f0, ap = np.asarray(dp, np.float64)[:F], np.asarray(f0, np.float64)[:F], np.asarray(ap, np.float64)[:F]
    err = np.abs(dp - ref_dp)
    lim = bt * np.abs(ref_dp)
    assert np.all(err <= lim), (who, 'd prime', float((err / np.maximum(lim, 1e-300)).max()))
    worst = float((err[lim > 0] / lim[lim > 0]).max()) if np.any(lim > 0) else 0.0
    excused = 0
    for f, p in enumerate(picks):
        if not p['decidable']:
            excused += 1
            continue
        assert (f0[f] > 0) == p['voiced'], (who, f, 'voiced flag', f0[f], p['voiced'])
        if p['voiced']:
            tau = int(np.rint(sr / f0[f] - p['delta']))
            assert tau == p['tau'], (who, f, 'tau*', tau, p['tau'])
            assert abs(f0[f] - p['f0']) <= p['tol'], (who, f, 'f0', f0[f], p['f0'], p['tol'])
            assert abs(ap[f] - p['ap']) <= bt * p['ap'], (who, f, 'ap')
        else:
            assert abs(ap[f] - p['ap']) <= bt * p['ap'], (who, f, 'ap')
    return worst, F, excused


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
