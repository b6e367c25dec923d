"""Reference of the spectral denoiser (csrc/wn_denoise.hip; definition in the issue text of csrc/wn_denoise.h): the four steps in float64 numpy, a float32
stand-in of the same formulation (explicit basis matrices in np.float32, sequential overlap-add) whose error against float64 is the YARDSTICK, the
signals of the tests, and the one parity rule that the device tests and the host-hook tests share:

    per row   |got - ref| <= 8 x max(yardstick of that row, 2^-23 max|x| of that row)      for every sample of the row

8 x the float32 yardstick is the standing margin of the mel analysis, the reconstruction check and the temperature work; the floor is one roundoff of the
largest value.  The map X -> X max(0, 1 - t / |X|) is a proximal map: non-expansive in X and 1-Lipschitz in t, so no element is excused.
The stand-in takes a `fault` to seed one of five mistakes; tests/test_denoise_cpu.py shows that the parity rule catches each."""
import numpy as np

GEOMETRIES = {'A': (64, 16), 'B': (96, 20), 'P': (1024, 256)}
FAULTS = ('synthesis_window_dropped', 'edge_frames_left_out_of_window_sum', 'nyquist_weighted_2', 'threshold_on_power', 'profile_one_bin_off')
KINDS = ('tone', 'below', 'straddle', 'above', 'impulse', 'zeros')
STRENGTHS = (0.0, 0.5, 1.0, 4.0)
EPS = 2.0 ** -23


def window(n_fft, dtype=np.float64):
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)).astype(dtype)


def num_frames(n, hop):
    return 1 + n // hop


def frame_matrix(x, n_fft, hop):
    """[F, n_fft]: frame f = the n_fft samples centred on f hop, zeros outside [0, n)"""
    x = np.asarray(x)
    n, H = len(x), n_fft // 2
    F = num_frames(n, hop)
    xp = np.zeros((F - 1) * hop + n_fft, x.dtype)
    m = min(n, len(xp) - H)
    xp[H:H + m] = x[:m]
    return xp[np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]]


def stft(x, n_fft, hop):
    return np.fft.rfft(frame_matrix(np.asarray(x, np.float64), n_fft, hop) * window(n_fft), axis=1)


def shrink(X, t):
    m = np.abs(X)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(m > t, (m - t) / m, 0.0)
    return X * s


def overlap_add(y, n, n_fft, hop, wsq, skip_edge_den=False):
    """y [F, n_fft] windowed frames -> out [n]; both sums over the covering frames in ascending f"""
    F, H = y.shape[0], n_fft // 2
    num = np.zeros((F - 1) * hop + n_fft, y.dtype)
    den = np.zeros_like(num)
    for f in range(F):
        num[f * hop:f * hop + n_fft] += y[f]
        if not (skip_edge_den and f in (0, F - 1)):
            den[f * hop:f * hop + n_fft] += wsq
    with np.errstate(divide='ignore', invalid='ignore'):
        return (num[H:H + n] / den[H:H + n]).astype(y.dtype)


def istft(Y, n, n_fft, hop):
    w = window(n_fft)
    return overlap_add(np.fft.irfft(Y, n_fft, axis=1) * w, n, n_fft, hop, w * w)


def inside(n, n_fft, hop):
    """frames whose window lies wholly inside [0, n)"""
    f = np.arange(num_frames(n, hop))
    return f[(f * hop >= n_fft // 2) & (f * hop + n_fft // 2 <= n)]


def fit(rows, n_fft, hop):
    """rows: list of 1-D signals -> profile [1 + n_fft / 2] float64; ValueError when no frame lies wholly inside any row"""
    tot, cnt = np.zeros(1 + n_fft // 2), 0
    for x in rows:
        if len(x) == 0:
            continue
        sel = inside(len(x), n_fft, hop)
        if len(sel):
            tot += np.abs(stft(x, n_fft, hop)[sel]).sum(0)
            cnt += len(sel)
    if cnt == 0:
        raise ValueError('no row holds a whole window of n_fft = %d samples' % n_fft)
    return tot / cnt


def denoise(x, profile, strength, n_fft, hop):
    x = np.asarray(x, np.float64)
    if len(x) == 0:
        return x.copy()
    return istft(shrink(stft(x, n_fft, hop), strength * np.asarray(profile, np.float64)[None, :]), len(x), n_fft, hop)


# ---- the float32 stand-in: explicit matrices, every product and sum in np.float32
_BASES = {}


def bases(n_fft):
    """(A_re, A_im [n_fft, bins], B_re, B_im [bins, n_fft]) float32, built in float64 with the angle reduced as the integer (j k) mod n_fft; window folded
    into both, Hermitian weights and 1 / n_fft into the inverse"""
    if n_fft not in _BASES:
        H = n_fft // 2
        j, k = np.arange(n_fft)[:, None], np.arange(H + 1)[None, :]
        ang = 2.0 * np.pi * ((j * k) % n_fft) / n_fft
        w = window(n_fft)[:, None]
        h = np.full(H + 1, 2.0); h[0] = h[H] = 1.0
        c, s = np.cos(ang), np.sin(ang)
        s[:, 0] = 0.0; s[:, H] = 0.0
        c[:, H] = np.where(np.arange(n_fft) % 2, -1.0, 1.0)
        _BASES[n_fft] = ((w * c).astype(np.float32), (-w * s).astype(np.float32),
                         ((w * c * h / n_fft).T).astype(np.float32).copy(), ((-w * s * h / n_fft).T).astype(np.float32).copy())
    return _BASES[n_fft]


def standin_spectrum(x, n_fft, hop):
    A_re, A_im, _, _ = bases(n_fft)
    fr = frame_matrix(np.asarray(x, np.float32), n_fft, hop)
    return fr @ A_re, fr @ A_im


def standin_fit(rows, n_fft, hop):
    tot, cnt = np.zeros(1 + n_fft // 2, np.float32), 0
    for x in rows:
        if len(x) == 0:
            continue
        sel = inside(len(x), n_fft, hop)
        if len(sel):
            re, im = standin_spectrum(x, n_fft, hop)
            for f in sel:
                tot = tot + np.sqrt(re[f] * re[f] + im[f] * im[f])
            cnt += len(sel)
    return (tot / np.float32(cnt)).astype(np.float32)


def standin(x, profile, strength, n_fft, hop, fault=None):
    assert fault is None or fault in FAULTS
    x = np.asarray(x, np.float32)
    if len(x) == 0:
        return x.copy()
    H = n_fft // 2
    _, _, B_re, B_im = bases(n_fft)
    if fault == 'synthesis_window_dropped':
        w = window(n_fft)
        with np.errstate(divide='ignore', invalid='ignore'):
            B_re, B_im = [np.where(w[None, :] > 0, b / w[None, :], 0.0).astype(np.float32) for b in (B_re, B_im)]
    if fault == 'nyquist_weighted_2':
        B_re = B_re.copy(); B_re[H] *= 2
    re, im = standin_spectrum(x, n_fft, hop)
    p = np.asarray(profile, np.float32)
    if fault == 'profile_one_bin_off':
        p = np.concatenate([p[1:], p[-1:]])
    t = (np.float32(strength) * p)[None, :]
    pw = re * re + im * im
    m = np.sqrt(pw)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(pw > t, (pw - t) / pw, 0.0) if fault == 'threshold_on_power' else np.where(m > t, (m - t) / m, 0.0)
    s = s.astype(np.float32)
    y = (re * s) @ B_re + (im * s) @ B_im
    wsq = (window(n_fft) ** 2).astype(np.float32)
    return overlap_add(y.astype(np.float32), len(x), n_fft, hop, wsq, skip_edge_den=fault == 'edge_frames_left_out_of_window_sum')


# ---- signals and the parity rule
def lengths_of(n_fft, hop):
    return [0, 1, 15, 16, 17, n_fft // 2 - 1, n_fft, 32 * hop - 1, 32 * hop, 32 * hop + 1, 64 * hop + 1, 2000]


def noise_profile(n_fft, hop, seed=1):
    """the profile every test subtracts: fitted (float64) on unit-variance-ish noise of another draw"""
    rs = np.random.RandomState(seed)
    return fit([0.1 * rs.randn(16 * n_fft).astype(np.float32)], n_fft, hop).astype(np.float32)


def signal(kind, n, seed, n_fft):
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    nz = 0.1 * rs.randn(n)      # the level the profile was fitted at
    if kind == 'tone':
        x = 0.5 * np.sin(2 * np.pi * t * 3.3 / n_fft * 4) + nz
    elif kind == 'below':
        x = 1e-3 * nz
    elif kind == 'straddle':
        x = nz
    elif kind == 'above':
        x = 100.0 * nz
    elif kind == 'impulse':
        x = np.zeros(n)
        if n:
            x[min(n - 1, n // 3)] = 1.0
    elif kind == 'zeros':
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def row_bound(x, ref, profile, strength, n_fft, hop):
    """8 x max(yardstick of the row, 2^-23 max|x|): the yardstick is the stand-in's worst error on this very row"""
    if len(x) == 0:
        return 0.0, 0.0
    yard = float(np.max(np.abs(standin(x, profile, strength, n_fft, hop).astype(np.float64) - ref)))
    return 8.0 * max(yard, EPS * float(np.max(np.abs(x)))), yard


def check_rows(got, wav, lengths, profile, strength, n_fft, hop):
    """got, wav [B, pitch]: every sample of every row against float64 under the rule -> (worst error / bound, worst yardstick / (2^-23 max|x|)); asserts
    nothing.  A row of zeros has bound 0: its output must be exact zeros (ratio 0 then, inf otherwise)."""
    worst, scale = 0.0, 0.0
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        x = np.asarray(wav[b, :n], np.float32)
        ref = denoise(x, profile, strength, n_fft, hop)
        bound, yard = row_bound(x, ref, profile, strength, n_fft, hop)
        err = float(np.max(np.abs(np.asarray(got[b, :n], np.float64) - ref)))
        worst = max(worst, 0.0 if err == 0.0 else (np.inf if bound == 0.0 else err / bound))
        mx = float(np.max(np.abs(x)))
        if mx > 0:
            scale = max(scale, yard / (EPS * mx))
    return worst, scale


def check_profile(got, rows, n_fft, hop):
    """every bin of a fitted profile against float64: |got - ref| <= 8 x max(yardstick, 2^-23 max ref) -> worst error / bound"""
    ref = fit(rows, n_fft, hop)
    yard = float(np.max(np.abs(standin_fit(rows, n_fft, hop).astype(np.float64) - ref)))
    bound = 8.0 * max(yard, EPS * float(np.max(ref)))
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref))) / bound


def batch(kind, lengths, seed, n_fft, pad=7, fill=np.nan):
    """[B, max(lengths) + pad] float32: row b holds signal(kind, lengths[b]); what lies beyond is `fill` (never read by a correct implementation)"""
    wav = np.full((len(lengths), max(max(lengths), 1) + pad), fill, np.float32)
    for b, n in enumerate(lengths):
        wav[b, :n] = signal(kind, n, seed + 17 * b, n_fft)
    return wav
