"""Audio helpers the WaveNet path needs (reference datasets/audio.py:9-59, 70-77, 178-270): loading, pre-emphasis, silence trimming,
padding, and the mel analysis -- melspectrogram in numpy float64 (the pinned reference of the tests) and melspectrogram_device on the
GPU (csrc/wn_mel.hip through _ext.MelAnalyzer; what wavenet_preprocess.py and synthesize.py --wavs_dir run), and its model-free inverse
(reference datasets/audio.py:97-112, 151-161, 184-185, 231-235, 252-253, 272-284): inv_mel_spectrogram in numpy and inv_mel_spectrogram_device on
the GPU (csrc/wn_griffin.hip through _ext.GriffinLim) -- the Griffin-Lim baseline a trained vocoder has to beat on the same mels.  The linear
spectrogram and the lws variant belong to the Tacotron model: out of scope."""
import numpy as np
from scipy import signal
from scipy.io import wavfile


def load_wav(path, sr):
    """Reference audio.py:9-10 (librosa.core.load) on scipy: float32 in [-1, 1), channels averaged.  int16 / 32768, int32 / 2^31, uint8 as
    (x - 128) / 128, float as is.  The reference resamples to sr; no resampler here matches librosa's, so another rate is an error.
    (mi355_resample_input=True takes another road: read_wav, then resample_signals.)"""
    rate, x = wavfile.read(path)
    if rate != sr:
        raise ValueError('%s: sample rate %d, expected %d (resample the file first: no resampler here matches librosa\'s)' % (path, rate, sr))
    return _as_float_mono(path, x)


def _as_float_mono(path, x):
    if x.dtype == np.int16:
        y = x.astype(np.float32) / 32768.0
    elif x.dtype == np.int32:
        y = (x.astype(np.float64) / 2147483648.0).astype(np.float32)
    elif x.dtype == np.uint8:
        y = (x.astype(np.float32) - 128.0) / 128.0
    elif x.dtype.kind == 'f':
        y = x.astype(np.float32)
    else:
        raise ValueError('%s: unsupported sample type %s' % (path, x.dtype))
    if y.ndim == 2:
        y = y.mean(axis=1, dtype=np.float32)
    return y


def read_wav(path):
    """(sample rate, float32 signal in [-1, 1), channels averaged) of a wav file at whatever rate it has: the conversions of load_wav."""
    rate, x = wavfile.read(path)
    return int(rate), _as_float_mono(path, x)


RESAMPLE_BATCH = 20


def resample_host(x, sr_in, sr_out, **design):
    """One signal from sr_in to sr_out on the host: the plain float32 loop of wn_test_resample_host (csrc/wn_resample.h), BIT-IDENTICAL to the device's
    _ext.Resampler -- the fallback where no GPU exists.  A Kaiser-windowed sinc in closed form with resampy's published kaiser_best design values (zeros,
    beta, rolloff in **design), evaluated exactly at the polyphase positions: close to, not equal to, what librosa's load(sr=...) returned; the length is
    librosa's ceil(n sr_out / sr_in), the last sample computed."""
    from wavenet_vocoder import _ext
    return _ext.resample_rows_host([x], sr_in, sr_out, **design)[0]


def resample_signals(signals, sr_in, sr_out, device=None):
    """float32 signals from sr_in to sr_out: in batches of RESAMPLE_BATCH through ONE _ext.Resampler on the GPU when there is one (device None: ask torch),
    else resample_host one by one; the bits are the same either way.  sr_in == sr_out returns the signals as they are."""
    signals = [np.ascontiguousarray(s, dtype=np.float32) for s in signals]
    if int(sr_in) == int(sr_out) or not signals:
        return signals
    if device is None:
        import torch
        device = torch.cuda.is_available()
    if not device:
        return [resample_host(s, sr_in, sr_out) for s in signals]
    import torch
    from wavenet_vocoder import _ext
    order = sorted(range(len(signals)), key=lambda i: len(signals[i]))      # neighbours in length share a batch
    rs = _ext.Resampler(sr_in, sr_out, min(RESAMPLE_BATCH, len(signals)), max(1, max(len(s) for s in signals)))
    out = [None] * len(signals)
    try:
        for a in range(0, len(order), RESAMPLE_BATCH):
            idx = order[a:a + RESAMPLE_BATCH]
            lens = [len(signals[i]) for i in idx]
            blk = np.zeros((len(idx), max(1, max(lens))), np.float32)
            for r, i in enumerate(idx):
                blk[r, :lens[r]] = signals[i]
            y, n_out = rs.run(torch.from_numpy(blk).cuda(), lens)
            y = y.cpu().numpy()
            for r, i in enumerate(idx):
                out[i] = y[r, :n_out[r]].copy()
    finally:
        rs.close()
    return out


def preemphasis(wav, k, preemphasize=True):
    """Reference audio.py:22-25."""
    if preemphasize:
        return signal.lfilter([1, -k], [1], wav)
    return wav


def inv_preemphasis(wav, k, inv_preemphasize=True):
    """Reference audio.py:27-30."""
    if inv_preemphasize:
        return signal.lfilter([1], [1, -k], wav)
    return wav


def start_and_end_indices(quantized, silence_threshold=2):
    """Reference audio.py:33-44: first / last sample further than silence_threshold from the mu-law code of silence (127)."""
    q = np.asarray(quantized).astype(np.int64)
    loud = np.flatnonzero(np.abs(q - 127) > silence_threshold)
    assert loud.size > 0 and loud[-1] > 1, 'no sample above the silence threshold'      # the reference's backward scan stops at index 2
    return int(loud[0]), int(loud[-1])


def trim_silence(wav, hparams):
    """Reference audio.py:46-52 == librosa.effects.trim(wav, top_db=trim_top_db, frame_length=trim_fft_size, hop_length=trim_hop_size)[0],
    restated on numpy from librosa's published algorithm: centred, reflect-padded frames of trim_fft_size every trim_hop_size; mean square
    per frame; a frame is non-silent when 10 log10(max(1e-10, mse)) - 10 log10(max(1e-10, max mse)) > -trim_top_db; the result runs from
    (first non-silent frame) x hop to min(len, (last non-silent frame + 1) x hop).  No librosa exists on the build machine to pin this
    against: it is checked against signals whose trimmed bounds the construction predicts, not against librosa itself."""
    wav = np.asarray(wav)
    n_fft, hop, top_db = int(hparams.trim_fft_size), int(hparams.trim_hop_size), float(hparams.trim_top_db)
    if wav.size == 0:
        return wav
    y = np.pad(wav.astype(np.float64), n_fft // 2, mode='reflect') if wav.size > 1 else np.pad(wav.astype(np.float64), n_fft // 2, mode='edge')
    n_frames = 1 + (len(y) - n_fft) // hop
    csum = np.concatenate([[0.0], np.cumsum(y * y)])
    starts = hop * np.arange(n_frames)
    mse = (csum[starts + n_fft] - csum[starts]) / n_fft
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(max(1e-10, float(mse.max())))
    loud = np.flatnonzero(db > -top_db)
    if loud.size == 0:
        return wav[0:0]
    return wav[int(loud[0]) * hop: min(len(wav), (int(loud[-1]) + 1) * hop)]


def librosa_pad_lr(x, fsize, fshift, pad_sides=1):
    """Reference audio.py:210-219: padding that brings len(x) to (len(x) // fshift + 1) * fshift, on the right or split over both sides."""
    assert pad_sides in (1, 2)
    pad = (x.shape[0] // fshift + 1) * fshift - x.shape[0]
    if pad_sides == 1:
        return 0, pad
    return pad // 2, pad // 2 + pad % 2


def get_hop_size(hparams):
    hop_size = hparams.hop_size
    if hop_size is None:
        assert hparams.frame_shift_ms is not None
        hop_size = int(hparams.frame_shift_ms / 1000 * hparams.sample_rate)
    return hop_size


def save_wavenet_wav(wav, path, sr, inv_preemphasize=None, k=None):
    """Peak-normalise to int16 and write.  Like the reference (audio.py:17-20) the inverse pre-emphasis
    arguments are accepted and ignored; unlike it, the caller's array is not modified in place."""
    wav = np.asarray(wav, dtype=np.float32)
    out = wav * (32767 / max(0.01, float(np.max(np.abs(wav))) if wav.size else 0.01))
    wavfile.write(path, sr, out.astype(np.int16))


# ---- reconstruction mel (reference datasets/audio.py:62-68, 169-173, 222-259): only used for the diagnostic plot
# "Local Condition vs Reconst. Mel-Spectrogram" of train.py:114,154 / synthesizer.py:115.  The reference calls librosa
# (librosa.stft, librosa.filters.mel); librosa is not a dependency here, so its published algorithm is restated on numpy:
# centred frames (zero padding, pad_mode='constant'), periodic Hann window of win_size centred in n_fft, rfft; Slaney-scale
# triangular filters with area ("slaney") normalisation.
_mel_basis_cache = {}


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz = 1000.0; min_log_mel = min_log_hz / f_sp; logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-10) / min_log_hz) / logstep, mels)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0; min_log_mel = min_log_hz / f_sp; logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def _build_mel_basis(hparams):
    """== librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) (htk=False, norm='slaney'): [num_mels, 1 + n_fft // 2]."""
    assert hparams.fmax <= hparams.sample_rate // 2
    key = (hparams.sample_rate, hparams.n_fft, hparams.num_mels, hparams.fmin, hparams.fmax)
    if key not in _mel_basis_cache:
        n_mels = hparams.num_mels
        fftfreqs = np.linspace(0.0, hparams.sample_rate / 2.0, 1 + hparams.n_fft // 2)
        mel_f = _mel_to_hz(np.linspace(_hz_to_mel(hparams.fmin), _hz_to_mel(hparams.fmax), n_mels + 2))
        fdiff = np.diff(mel_f)
        ramps = mel_f[:, None] - fftfreqs[None, :]
        lower = -ramps[:-2] / fdiff[:-1, None]
        upper = ramps[2:] / fdiff[1:, None]
        weights = np.maximum(0.0, np.minimum(lower, upper))
        weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
        _mel_basis_cache[key] = weights.astype(np.float32)
    return _mel_basis_cache[key]


def _stft(y, hparams):
    """== librosa.stft(y, n_fft, hop_length, win_length, pad_mode='constant') -> complex [1 + n_fft // 2, frames]."""
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    from scipy.signal import get_window
    n_fft, hop, win = hparams.n_fft, get_hop_size(hparams), hparams.win_size
    w = get_window('hann', win, fftbins=True)
    lpad = (n_fft - win) // 2
    w = np.pad(w, (lpad, n_fft - win - lpad))
    y = np.pad(np.asarray(y, dtype=np.float64), n_fft // 2, mode='constant')
    n_frames = 1 + (len(y) - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return np.fft.rfft(y[idx] * w[None, :], axis=1).T


def _amp_to_db(x, hparams):
    min_level = np.exp(hparams.min_level_db / 20 * np.log(10))
    return 20 * np.log10(np.maximum(min_level, x))


def _normalize(S, hparams):
    m, lo = hparams.max_abs_value, hparams.min_level_db
    if hparams.allow_clipping_in_normalization:
        if hparams.symmetric_mels:
            return np.clip((2 * m) * ((S - lo) / (-lo)) - m, -m, m)
        return np.clip(m * ((S - lo) / (-lo)), 0, m)
    assert S.max() <= 0 and S.min() - lo >= 0
    if hparams.symmetric_mels:
        return (2 * m) * ((S - lo) / (-lo)) - m
    return m * ((S - lo) / (-lo))


def melspectrogram(wav, hparams):
    """Reference datasets/audio.py:62-68 -> [num_mels, frames]."""
    D = _stft(wav, hparams)
    S = _amp_to_db(np.dot(_build_mel_basis(hparams), np.abs(D) ** hparams.magnitude_power), hparams) - hparams.ref_level_db
    if hparams.signal_normalization:
        return _normalize(S, hparams)
    return S


def melspectrogram_device(wavs, hparams, analyzer=None):
    """melspectrogram for a list of 1-D signals on the GPU: a list of [num_mels, F_b] float32 arrays, F_b = 1 + len // hop (the same
    contract as melspectrogram, batched; fp32 arithmetic, csrc/wn_mel.hip).  analyzer: an _ext.MelAnalyzer to reuse (its capacity bounds the
    batch and the longest signal); None builds one for this call."""
    import torch
    from wavenet_vocoder import _ext
    wavs = [np.ascontiguousarray(w, dtype=np.float32).reshape(-1) for w in wavs]
    if not wavs:
        return []
    own = analyzer is None
    if own:
        analyzer = _ext.MelAnalyzer(hparams, min(len(wavs), 64), max(len(w) for w in wavs))
    try:
        out = [None] * len(wavs)
        order = sorted(range(len(wavs)), key=lambda i: len(wavs[i]))      # neighbours in length share a batch: little padding
        for lo in range(0, len(order), analyzer.max_batch):
            idx = order[lo:lo + analyzer.max_batch]
            lens = [len(wavs[i]) for i in idx]
            host = np.zeros((len(idx), max(1, max(lens))), dtype=np.float32)
            for r, i in enumerate(idx):
                host[r, :lens[r]] = wavs[i]
            mel = analyzer.run(torch.from_numpy(host).cuda(), lens, channels_first=True).cpu().numpy()
            for r, i in enumerate(idx):
                out[i] = np.ascontiguousarray(mel[r, :, :1 + lens[r] // analyzer.hop])
        return out
    finally:
        if own:
            analyzer.close()


# ---- mel -> wav without a model (reference datasets/audio.py:97-112, 151-161): the pseudo-inverse of the mel filters, ** power, Griffin-Lim.  librosa's
# istft is restated on numpy from its published algorithm: the inverse DFT of every frame under the same window, overlap-add, division by the
# window-square sum of the covering frames (where it exceeds the smallest normal float32, as librosa does), n_fft / 2 trimmed at both ends.
_inv_mel_basis_cache = {}


def _inv_mel_basis(hparams):
    key = (hparams.sample_rate, hparams.n_fft, hparams.num_mels, hparams.fmin, hparams.fmax)
    if key not in _inv_mel_basis_cache:
        _inv_mel_basis_cache[key] = np.linalg.pinv(np.asarray(_build_mel_basis(hparams), np.float64))
    return _inv_mel_basis_cache[key]


def _denormalize(D, hparams):
    """Reference audio.py:272-284."""
    m, lo = hparams.max_abs_value, hparams.min_level_db
    if hparams.allow_clipping_in_normalization:
        if hparams.symmetric_mels:
            return ((np.clip(D, -m, m) + m) * -lo / (2 * m)) + lo
        return (np.clip(D, 0, m) * -lo / m) + lo
    if hparams.symmetric_mels:
        return ((D + m) * -lo / (2 * m)) + lo
    return (D * -lo / m) + lo


def _db_to_amp(x):
    return np.power(10.0, x * 0.05)


def _mel_to_linear(mel_spectrogram, hparams):
    return np.maximum(1e-10, np.dot(_inv_mel_basis(hparams), mel_spectrogram))


def _window(hparams):
    from scipy.signal import get_window
    n_fft, win = hparams.n_fft, hparams.n_fft if hparams.win_size is None else hparams.win_size
    lpad = (n_fft - win) // 2
    return np.pad(get_window('hann', win, fftbins=True), (lpad, n_fft - win - lpad))


def _istft(Y, hparams):
    """== librosa.istft(Y, hop_length, win_length) for complex Y [1 + n_fft // 2, frames] -> hop (frames - 1) samples."""
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    n_fft, hop = hparams.n_fft, get_hop_size(hparams)
    w = _window(hparams)
    F = Y.shape[1]
    fr = np.fft.irfft(Y.T, n_fft, axis=1) * w[None, :]
    y = np.zeros(n_fft + hop * (F - 1))
    wss = np.zeros_like(y)
    for f in range(F):
        y[f * hop:f * hop + n_fft] += fr[f]
        wss[f * hop:f * hop + n_fft] += w * w
    ok = wss > np.finfo(np.float32).tiny
    y[ok] /= wss[ok]
    return y[n_fft // 2:n_fft // 2 + hop * (F - 1)]


def _griffin_lim(S, hparams, rng=None):
    """Reference audio.py:151-161; the random start comes from `rng` (a numpy Generator or RandomState; None: a fresh default_rng())."""
    rng = np.random.default_rng() if rng is None else rng
    u = rng.random(S.shape) if hasattr(rng, 'random') else rng.random_sample(S.shape)
    S_complex = np.abs(S).astype(np.complex128)
    y = _istft(S_complex * np.exp(2j * np.pi * u), hparams)
    for _ in range(hparams.griffin_lim_iters):
        angles = np.exp(1j * np.angle(_stft(y, hparams)))
        y = _istft(S_complex * angles, hparams)
    return y


def mel_to_magnitude(mel_spectrogram, hparams):
    """[num_mels, F] normalised mel -> the magnitudes Griffin-Lim aims at, [1 + n_fft // 2, F] (reference audio.py:99-104 and the ** power of :112)"""
    D = _denormalize(mel_spectrogram, hparams) if hparams.signal_normalization else mel_spectrogram
    return _mel_to_linear(_db_to_amp(D + hparams.ref_level_db) ** (1 / hparams.magnitude_power), hparams) ** hparams.power


def inv_mel_spectrogram(mel_spectrogram, hparams, rng=None):
    """Reference audio.py:97-112: [num_mels, F] -> the de-emphasised waveform of hop (F - 1) samples, in numpy float64 (no GPU)."""
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    return inv_preemphasis(_griffin_lim(mel_to_magnitude(np.asarray(mel_spectrogram, np.float64), hparams), hparams, rng), hparams.preemphasis, hparams.preemphasize)


def inv_mel_spectrogram_host(mels, hparams, seed=0, deemphasize=True):
    """inv_mel_spectrogram over a list of [num_mels, F_b] mels in numpy (no GPU): float32 waveforms; mel b starts from default_rng(seed + b).
    deemphasize False: the signals before the de-emphasis (the model domain of the checks)."""
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    out = []
    for b, mel in enumerate(mels):
        y = _griffin_lim(mel_to_magnitude(np.asarray(mel, np.float64), hparams), hparams, np.random.default_rng(int(seed) + b))
        out.append((inv_preemphasis(y, hparams.preemphasis, hparams.preemphasize) if deemphasize else y).astype(np.float32))
    return out


GRIFFIN_BATCH = 20


def inv_mel_spectrogram_device(mels, frames, hparams, iters=None, seed=0, griffin=None, deemphasize=True, return_model_domain=False):
    """inv_mel_spectrogram for a batch on the GPU (csrc/wn_griffin.hip): mels a list of [num_mels, F_b] arrays (frames None: their widths) or one array
    [B, num_mels, F_max] with frames the B frame counts.  Returns a list of float32 waveforms of hop (F_b - 1) samples, de-emphasised through the device
    output stage (_ext.OutputStage, in_type 'raw') when hparams.preemphasize and deemphasize; return_model_domain: (waveforms, the signals before the
    de-emphasis).  iters None: hparams.griffin_lim_iters.  The start is drawn on the device from `seed` (row b of the call's k-th batch: seed + k).
    griffin: an _ext.GriffinLim to reuse (its capacity bounds the batch and the longest mel); None builds one for this call."""
    import torch
    from wavenet_vocoder import _ext
    if getattr(hparams, 'use_lws', False):
        raise NotImplementedError('use_lws: the lws package is not available')
    if frames is None:
        mels = [np.ascontiguousarray(m, dtype=np.float32) for m in mels]
        frames = [int(m.shape[1]) for m in mels]
    else:
        frames = [int(f) for f in frames]
        mels = [np.ascontiguousarray(np.asarray(mels[b])[:, :frames[b]], dtype=np.float32) for b in range(len(frames))]
    if not mels:
        return ([], []) if return_model_domain else []
    iters = int(hparams.griffin_lim_iters) if iters is None else int(iters)
    hop = get_hop_size(hparams)
    own = griffin is None
    if own:
        griffin = _ext.GriffinLim(hparams, min(len(mels), GRIFFIN_BATCH), max(frames))
    k_de = float(hparams.preemphasis) if (hparams.preemphasize and deemphasize) else 0.0
    post = _ext.OutputStage(hparams, griffin.rows, deemphasis=k_de, in_type='raw') if k_de != 0.0 else None
    try:
        out, raw = [None] * len(mels), [None] * len(mels)
        order = sorted(range(len(mels)), key=lambda i: frames[i])      # neighbours in length share a batch: little padding
        for k, lo in enumerate(range(0, len(order), griffin.rows)):
            idx = order[lo:lo + griffin.rows]
            fr = [frames[i] for i in idx]
            host = np.zeros((len(idx), int(hparams.num_mels), max(fr)), np.float32)
            for r, i in enumerate(idx):
                host[r, :, :fr[r]] = mels[i]
            y = griffin.run_mel(torch.from_numpy(host).cuda(), fr, iters=iters, channels_first=True, seed=None if seed is None else int(seed) + k)
            n = [hop * (f - 1) for f in fr]
            z = post.finish(y, n, pcm=False) if post is not None else y
            y, z = y.cpu().numpy(), z.cpu().numpy()
            for r, i in enumerate(idx):
                raw[i], out[i] = y[r, :n[r]].copy(), z[r, :n[r]].copy()
        return (out, raw) if return_model_domain else out
    finally:
        if post is not None:
            post.close()
        if own:
            griffin.close()
