"""Reference of the Griffin-Lim baseline (csrc/wn_griffin.hip; definition at the top of csrc/wn_griffin.h): float64 numpy restated from librosa's published
stft / istft (periodic Hann of win_size centred in n_fft, centred frames with zero padding, windowed inverse, overlap-add, division by the window-square
sum, trim of n_fft / 2), a float32 stand-in of the same formulation (explicit basis matrices in np.float32) whose error against float64 is the YARDSTICK,
the signals of the tests, and the STAGED parity rule the device tests and the host-hook tests share.  One iteration is not Lipschitz where a bin of
STFT(y) is near zero, so it is never compared end to end; each stage is compared with float64 applied to the DEVICE's own input of that stage:

    spectrum    |X - STFT64(y0)|                 <= 8 x max(stand-in's worst error in that frame, 2^-23 x the frame's largest |X|)   every element
    output      |y - ISTFT64(project64(X_dev))|  <= 8 x max(yardstick of that row, 2^-23 max|y| of that row)                        every sample
    magnitudes  |S - S64(mel)|                   <= 8 x max(yardstick of that frame, 2^-23 x the frame's largest value)             every element

The factor 8 and the floors are the standing rule of tests/denoise_ref.py.  The stand-in takes a `fault` to seed one of five mistakes;
tests/test_griffin_cpu.py shows that the staged rule catches each."""
import numpy as np

GEOMETRIES = {'A': (64, 48, 12), 'B': (96, 80, 20), 'C': (64, 64, 16), 'P': (2048, 1100, 275)}
FRAMES = (2, 31, 32, 33, 65)
KINDS = ('noise', 'tones', 'impulses', 'tone', 'zeros')
FAULTS = ('synthesis_window_dropped', 'edge_frames_left_out_of_window_sum', 'nyquist_weighted_2', 'magnitude_before_power', 'window_not_centred')
EPS = 2.0 ** -23
FACTOR = 8.0


def num_samples(F, hop):
    return hop * (F - 1)


def window(n_fft, win, centred=True):
    """[n_fft] float64: periodic Hann of win at offset (n_fft - win) // 2"""
    w = np.zeros(n_fft)
    off = (n_fft - win) // 2 if centred else 0
    w[off:off + win] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return w


def frame_matrix(y, F, n_fft, hop):
    """[F, n_fft]: frame f = the n_fft samples centred on f hop, zeros outside [0, n)"""
    y = np.asarray(y)
    H = n_fft // 2
    yp = np.zeros((F - 1) * hop + n_fft, y.dtype)
    m = min(len(y), len(yp) - H)
    yp[H:H + m] = y[:m]
    return yp[np.arange(F)[:, None] * hop + np.arange(n_fft)[None, :]]


def stft(y, F, geo):
    n_fft, win, hop = geo
    return np.fft.rfft(frame_matrix(np.asarray(y, np.float64), F, n_fft, hop) * window(n_fft, win), axis=1)


def overlap_add(fr, F, n_fft, hop, wsq, skip_edge_den=False):
    """fr [F, n_fft] windowed frames -> y [hop (F - 1)]; both sums over the covering frames in ascending f"""
    H, n = n_fft // 2, hop * (F - 1)
    num = np.zeros((F - 1) * hop + n_fft, fr.dtype)
    den = np.zeros_like(num)
    for f in range(F):
        num[f * hop:f * hop + n_fft] += fr[f]
        if not (skip_edge_den and f in (0, F - 1)):
            den[f * hop:f * hop + n_fft] += wsq
    with np.errstate(divide='ignore', invalid='ignore'):
        return (num[H:H + n] / den[H:H + n]).astype(fr.dtype)


def window_square_sum(F, geo):
    """the denominator of every sample of a row of F frames"""
    n_fft, win, hop = geo
    w = window(n_fft, win)
    den = np.zeros((F - 1) * hop + n_fft)
    for f in range(F):
        den[f * hop:f * hop + n_fft] += w * w
    return den[n_fft // 2:n_fft // 2 + hop * (F - 1)]


def istft(Y, F, geo):
    n_fft, win, hop = geo
    w = window(n_fft, win)
    return overlap_add(np.fft.irfft(Y, n_fft, axis=1) * w, F, n_fft, hop, w * w)


def project(X, S):
    """S X / |X|; an exactly zero X takes the phase (1, 0); bins 0 and n_fft / 2 keep their real part alone"""
    X = np.array(X, np.complex128)
    X[:, 0] = X[:, 0].real; X[:, -1] = X[:, -1].real
    m = np.abs(X)
    with np.errstate(divide='ignore', invalid='ignore'):
        ph = np.where(m > 0, X / m, 1.0)
    return np.asarray(S, np.float64) * ph


def start(S, u, F, geo):
    """y0 = ISTFT(S e^{2 pi i u}); u None: zero phase"""
    S = np.asarray(S, np.float64)
    return istft(S.astype(np.complex128) if u is None else S * np.exp(2j * np.pi * np.asarray(u, np.float64)), F, geo)


def iterate(y, S, F, geo, iters=1):
    for _ in range(iters):
        y = istft(project(stft(y, F, geo), S), F, geo)
    return y


def convergence(y, S, F, geo):
    """|| |STFT(y)| - S ||_F / || S ||_F in float64"""
    S = np.asarray(S, np.float64)
    return float(np.linalg.norm(np.abs(stft(y, F, geo)) - S) / np.linalg.norm(S))


# ---- mel -> magnitudes
def mel_basis(num_mels, n_fft):
    """a dense non-negative filter bank [num_mels, 1 + n_fft / 2] of overlapping triangles on a warped axis (the shape of librosa's, any geometry)"""
    nb = 1 + n_fft // 2
    edges = (nb - 1) * (np.linspace(0.0, 1.0, num_mels + 2) ** 1.6)
    k = np.arange(nb)[None, :]
    lo, mid, hi = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    tri = np.maximum(0.0, np.minimum((k - lo) / np.maximum(mid - lo, 1e-9), (hi - k) / np.maximum(hi - mid, 1e-9)))
    tri[0, 0] = 1.0
    return (tri * (2.0 / (hi - lo))).astype(np.float32)


def pinv_of(basis):
    """what the binding hands to wn_griffin_create: np.linalg.pinv in float64, rounded to float32 once: [1 + n_fft / 2, num_mels]"""
    return np.ascontiguousarray(np.linalg.pinv(np.asarray(basis, np.float64)).astype(np.float32))


MEL_VARIANTS = {      # (signal_normalization, allow_clipping, symmetric_mels)
    'clip_sym': (1, 1, 1), 'clip_asym': (1, 1, 0), 'sym': (1, 0, 1), 'asym': (1, 0, 0), 'raw': (0, 0, 0),
}


def mel_level(variant, magnitude_power=2.0, power=1.5, min_level_db=-100.0, ref_level_db=20.0, max_abs_value=4.0):
    norm, clip, sym = MEL_VARIANTS[variant]
    return dict(norm=norm, clip=clip, sym=sym, magnitude_power=magnitude_power, power=power, lo=min_level_db, ref=ref_level_db, maxabs=max_abs_value)


def magnitudes(mel, pinv, lv, dtype=np.float64, fault=None):
    """mel [F, num_mels] normalised -> S [F, 1 + n_fft / 2] in `dtype` (float64: the reference; float32: the stand-in)"""
    t = dtype
    D = np.asarray(mel, np.float32).astype(t)
    lo, ref, m = t(lv['lo']), t(lv['ref']), t(lv['maxabs'])
    if lv['norm']:
        if lv['clip']:
            D = np.clip(D, -m if lv['sym'] else t(0), m)
        D = ((D + m) * -lo) / (t(2) * m) + lo if lv['sym'] else (D * -lo) / m + lo
    a = np.power(t(10), (D + ref) * t(0.05))
    if lv['magnitude_power'] != 1.0:
        a = np.power(a, t(1.0 / lv['magnitude_power']))
    S = np.maximum(t(1e-10), a @ np.asarray(pinv, np.float32).astype(t).T)
    if fault == 'magnitude_before_power':
        return S.astype(t)
    return (np.power(S, t(lv['power'])) if lv['power'] != 1.0 else S).astype(t)


def normalised_mel(S_lin, basis, lv):
    """a normalised mel [F, num_mels] float32 of linear magnitudes S_lin [F, bins] (the analysis of wn_mel restated, float64)"""
    M = (np.asarray(S_lin, np.float64) ** lv['magnitude_power']) @ np.asarray(basis, np.float64).T
    L = 20.0 * np.log10(np.maximum(10.0 ** (lv['lo'] / 20.0), M)) - lv['ref']
    if not lv['norm']:
        return L.astype(np.float32)
    u = (L - lv['lo']) / (-lv['lo'])
    v = (2 * lv['maxabs']) * u - lv['maxabs'] if lv['sym'] else lv['maxabs'] * u
    if lv['clip']:
        v = np.clip(v, -lv['maxabs'] if lv['sym'] else 0.0, lv['maxabs'])
    return v.astype(np.float32)


# ---- the float32 stand-in: explicit matrices, every product and sum in np.float32
_BASES = {}


def bases(geo, centred=True):
    """(A_re, A_im [n_fft, bins], B_re, B_im [bins, n_fft]) float32, built in float64 with the angle reduced as the integer (j k) mod n_fft; window folded
    into both, Hermitian weights and 1 / n_fft into the inverse"""
    key = (geo, centred)
    if key not in _BASES:
        n_fft, win, _ = geo
        H = n_fft // 2
        j, k = np.arange(n_fft)[:, None], np.arange(H + 1)[None, :]
        ang = 2.0 * np.pi * ((j * k) % n_fft) / n_fft
        w = window(n_fft, win, centred)[:, None]
        h = np.full(H + 1, 2.0); h[0] = h[H] = 1.0
        c, s = np.cos(ang), np.sin(ang)
        s[:, 0] = 0.0; s[:, H] = 0.0
        c[:, H] = np.where(np.arange(n_fft) % 2, -1.0, 1.0)
        _BASES[key] = ((w * c).astype(np.float32), (-w * s).astype(np.float32),
                       ((w * c * h / n_fft).T).astype(np.float32).copy(), ((-w * s * h / n_fft).T).astype(np.float32).copy())
    return _BASES[key]


def standin_spectrum(y, F, geo, fault=None):
    """complex64 [F, bins]"""
    A_re, A_im, _, _ = bases(geo, centred=fault != 'window_not_centred')
    fr = frame_matrix(np.asarray(y, np.float32), F, geo[0], geo[2])
    return (fr @ A_re) + 1j * (fr @ A_im)


def standin_synthesis(Y, F, geo, fault=None):
    """a projected (or start) spectrum Y complex [F, bins] -> y float32"""
    n_fft, win, hop = geo
    H = n_fft // 2
    _, _, B_re, B_im = bases(geo, centred=fault != 'window_not_centred')
    if fault == 'synthesis_window_dropped':
        w = window(n_fft, win)
        with np.errstate(divide='ignore', invalid='ignore'):
            B_re, B_im = [np.where(w[None, :] > 0, b / w[None, :], 0.0).astype(np.float32) for b in (B_re, B_im)]
    if fault == 'nyquist_weighted_2':
        B_re = B_re.copy(); B_re[H] *= 2
    fr = np.real(Y).astype(np.float32) @ B_re + np.imag(Y).astype(np.float32) @ B_im
    wsq = (window(n_fft, win) ** 2).astype(np.float32)
    return overlap_add(fr.astype(np.float32), F, n_fft, hop, wsq, skip_edge_den=fault == 'edge_frames_left_out_of_window_sum')


def standin_project(X, S):
    """float32: the larger component scaled to 1, as the kernel forms the hypot"""
    re, im = np.real(X).astype(np.float32).copy(), np.imag(X).astype(np.float32).copy()
    im[:, 0] = 0; im[:, -1] = 0
    S = np.asarray(S, np.float32)
    m = np.maximum(np.abs(re), np.abs(im))
    with np.errstate(divide='ignore', invalid='ignore'):
        r, i = re / m, im / m
        h = np.sqrt(r * r + i * i)
        yr, yi = np.where(m > 0, S * (r / h), S), np.where(m > 0, S * (i / h), np.float32(0))
    return yr.astype(np.float32) + 1j * yi.astype(np.float32)


def standin_output(X, S, F, geo, fault=None):
    return standin_synthesis(standin_project(X, S), F, geo, fault)


def standin_start(S, u, F, geo, fault=None):
    S = np.asarray(S, np.float32)
    if u is None:
        return standin_synthesis(S.astype(np.complex64), F, geo, fault)
    a = np.float32(2.0 * np.pi) * np.asarray(u, np.float32)
    return standin_synthesis(S * np.cos(a) + 1j * (S * np.sin(a)), F, geo, fault)


def standin_iterate(y, S, F, geo, iters=1):
    y = np.asarray(y, np.float32)
    for _ in range(iters):
        y = standin_output(standin_spectrum(y, F, geo), S, F, geo)
    return y


# ---- signals
def signal(kind, n, seed, n_fft):
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    if kind == 'noise':
        x = 0.3 * rs.randn(n)
    elif kind == 'tones':
        x = 0.3 * np.sin(2 * np.pi * t * 3.3 / n_fft) + 0.2 * np.sin(2 * np.pi * t * 7.1 / n_fft) + 0.02 * rs.randn(n)
    elif kind == 'impulses':
        x = np.zeros(n)
        for q in range(5):
            x[min(n - 1, (2 * q + 1) * n // 10)] = 1.0 - 0.15 * q
    elif kind == 'tone':      # most magnitudes tiny
        x = 0.5 * np.sin(2 * np.pi * t * 4.0 / n_fft)
    elif kind == 'zeros':
        x = np.zeros(n)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def target(kind, F, seed, geo):
    """the magnitudes S [F, bins] float32 of signal(kind) and the signal itself"""
    x = signal(kind, num_samples(F, geo[2]), seed, geo[0])
    return np.abs(stft(x, F, geo)).astype(np.float32), x


def uniforms(F, geo, seed):
    return np.random.RandomState(seed).rand(F, 1 + geo[0] // 2).astype(np.float32)


# ---- the staged rule: every function returns (worst error / bound, worst yardstick / floor) and asserts nothing.  A bound of 0 (all zeros) demands
# exact zeros: ratio 0 then, inf otherwise.
def _ratio(err, bound):
    err, bound = np.asarray(err, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(err))
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, np.where(bound == 0, np.inf, err / bound))
    return float(np.max(r)) if r.size else 0.0


def check_spectrum(got, y0, F, geo, standin=None):
    """got complex [F, bins]: the spectrum before the projection, against float64 STFT of the float32 input y0"""
    ref = stft(np.asarray(y0, np.float32), F, geo)
    st = standin_spectrum(y0, F, geo) if standin is None else standin
    yard = np.max(np.abs(st.astype(np.complex128) - ref), axis=1)
    floor = EPS * np.max(np.abs(ref), axis=1)
    bound = FACTOR * np.maximum(yard, floor)
    with np.errstate(divide='ignore', invalid='ignore'):
        scale = float(np.max(np.where(floor > 0, yard / floor, 0.0)))
    return _ratio(np.abs(np.asarray(got, np.complex128) - ref), bound[:, None]), scale


def check_output(got, X, S, F, geo, standin=None):
    """got [n]: the output of one iteration, against float64 projection + ISTFT of the producer's OWN spectrum X (complex, float32 values)"""
    X = np.asarray(X, np.complex64)
    ref = istft(project(X, np.asarray(S, np.float32)), F, geo)
    st = standin_output(X, S, F, geo) if standin is None else standin
    yard = float(np.max(np.abs(st.astype(np.float64) - ref))) if ref.size else 0.0
    floor = EPS * (float(np.max(np.abs(ref))) if ref.size else 0.0)
    return _ratio(np.abs(np.asarray(got, np.float64) - ref), FACTOR * max(yard, floor)), (yard / floor if floor > 0 else 0.0)


def check_start(got, S, u, F, geo, standin=None):
    """got [n]: y0 = ISTFT(S e^{2 pi i u}) against float64 (u float32 values; None: zero phase), under the output's rule"""
    ref = start(np.asarray(S, np.float32), None if u is None else np.asarray(u, np.float32), F, geo)
    st = standin_start(S, u, F, geo) if standin is None else standin
    yard = float(np.max(np.abs(st.astype(np.float64) - ref))) if ref.size else 0.0
    floor = EPS * (float(np.max(np.abs(ref))) if ref.size else 0.0)
    return _ratio(np.abs(np.asarray(got, np.float64) - ref), FACTOR * max(yard, floor)), (yard / floor if floor > 0 else 0.0)


def check_magnitudes(got, mel, pinv, lv, standin=None):
    """got [F, bins]: the magnitudes from a normalised mel against float64, per frame"""
    ref = magnitudes(mel, pinv, lv, np.float64)
    st = magnitudes(mel, pinv, lv, np.float32) if standin is None else standin
    yard = np.max(np.abs(st.astype(np.float64) - ref), axis=1)
    floor = EPS * np.max(np.abs(ref), axis=1)
    bound = FACTOR * np.maximum(yard, floor)
    return _ratio(np.abs(np.asarray(got, np.float64) - ref), bound[:, None]), float(np.max(yard / floor))


def mel_band(hp, freq):
    """[lo, hi] in Hz: where a mel of hparams `hp` can place a steady tone of `freq`.  The analysis window (Hann of win_size) spreads the tone over its main
    lobe, freq +- 2 sample_rate / win_size; every mel filter with weight inside the lobe takes part of it, and the pseudo-inverse hands a filter's energy
    back somewhere on that filter's support: the union of the supports of those filters (one bin of slack at either end).  A first version of this band
    took the one filter that weighs `freq` most; a tone between two filter centres (220 Hz at the defaults) is carried by both, and its inversion peaked in
    the neighbour's support (263 Hz, outside that filter's [161, 237])."""
    from datasets import audio
    basis = np.asarray(audio._build_mel_basis(hp), np.float64)
    hz = np.linspace(0.0, hp.sample_rate / 2.0, basis.shape[1])
    lobe = 2.0 * hp.sample_rate / float(hp.n_fft if hp.win_size is None else hp.win_size)
    inside = (hz >= freq - lobe) & (hz <= freq + lobe)
    on = np.flatnonzero(np.any(basis[np.any(basis[:, inside] > 0, axis=1)] > 0, axis=0))
    return float(hz[max(on[0] - 1, 0)]), float(hz[min(on[-1] + 1, len(hz) - 1)])


def spectral_peak(y, sr):
    """the frequency in Hz of the largest bin of the Hann-windowed spectrum of y"""
    y = np.asarray(y, np.float64)
    return float(np.argmax(np.abs(np.fft.rfft(y * np.hanning(len(y))))) * sr / len(y))
