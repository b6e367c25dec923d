"""Shared by tests/test_mel_cpu.py and tests/test_hip_mel.py: the float64 reference (datasets.audio.melspectrogram, pinned by
test_host_cpu.py), the float32 yardstick that sets the device's tolerance, seeded test signals and synthetic wav folders."""
import contextlib
import os

import numpy as np

FACTOR = 8.0            # an fp32 sum taken in another order may differ from the yardstick's by this factor
FLOOR = 2.0 ** -19      # floor of the yardstick (an all-floor signal's yardstick is 0)


def mel_hparams(**over):
    import hparams as H
    hp = H._build()
    for k, v in over.items():
        setattr(hp, k, v)
    return hp


def dft_matrix_mel(wav, hp, dtype):
    """The formulation the kernel implements -- frames x [win, 2 x bins] window-folded DFT matrix (argument reduced as integers, built in
    float64), power, mel filters, level, normalisation -- evaluated on the CPU with every array and product in `dtype`.  float64: equals
    datasets.audio.melspectrogram to ~1e-13; float32: the yardstick (same arithmetic as the device up to the order of the sums)."""
    from datasets import audio
    n_fft, hop, win = hp.n_fft, audio.get_hop_size(hp), hp.win_size
    off, nb = (n_fft - win) // 2, 1 + n_fft // 2
    k = np.arange(win, dtype=np.int64)
    w = 0.5 - 0.5 * np.cos(2 * np.pi * k / win)
    idx = ((k + off)[:, None] * np.arange(nb, dtype=np.int64)[None, :]) % n_fft
    ang = 2 * np.pi * idx / n_fft
    C, S = (w[:, None] * np.cos(ang)).astype(dtype), (-w[:, None] * np.sin(ang)).astype(dtype)
    y = np.pad(np.asarray(wav, dtype=dtype), n_fft // 2, mode='constant')
    nf = 1 + len(wav) // hop
    frames = y[(hop * np.arange(nf))[:, None] + off + k[None, :]]
    re, im = frames @ C, frames @ S
    P = re * re + im * im
    if hp.magnitude_power == 1:
        P = np.sqrt(P)
    elif hp.magnitude_power != 2:
        P = P ** dtype(hp.magnitude_power / 2)
    M = P @ audio._build_mel_basis(hp).astype(dtype).T
    lvl = dtype(20) * np.log10(np.maximum(dtype(10.0 ** (hp.min_level_db / 20)), M)) - dtype(hp.ref_level_db)
    if not hp.signal_normalization:
        return lvl.T
    m, lo = dtype(hp.max_abs_value), dtype(hp.min_level_db)
    u = (lvl - lo) / (-lo)
    v = (2 * m) * u - m if hp.symmetric_mels else m * u
    if hp.allow_clipping_in_normalization:
        v = np.clip(v, -m if hp.symmetric_mels else dtype(0), m)
    return v.T


def reference(wav, hp):
    """float64 [num_mels, frames]; the non-clipping _normalize variants without the reference's assert (the kernel has none)."""
    from datasets import audio
    if hp.signal_normalization and not hp.allow_clipping_in_normalization:
        return dft_matrix_mel(np.asarray(wav, dtype=np.float64), hp, np.float64)
    return audio.melspectrogram(np.asarray(wav, dtype=np.float64), hp)


def tolerance(wav, hp, ref=None):
    """(tolerance, yardstick): yardstick = max |float32 formulation - float64 reference| for this signal; tolerance = 8 x max(yardstick,
    2^-19).  Computed from the reference only."""
    ref = reference(wav, hp) if ref is None else ref
    y32 = dft_matrix_mel(np.asarray(wav, dtype=np.float32), hp, np.float32)
    yard = float(np.max(np.abs(y32.astype(np.float64) - ref))) if ref.size else 0.0
    return FACTOR * max(yard, FLOOR), yard


def make_signal(kind, n, seed, sr=22050):
    rng = np.random.RandomState(seed)
    t = np.arange(n, dtype=np.float64)
    if kind == 'sine':
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t / sr)
    elif kind == 'harmonic':
        f0 = 140.0
        x = sum(0.3 / h * np.sin(2 * np.pi * f0 * h * t / sr + h) for h in range(1, 12))
        x = (x + 0.01 * rng.randn(n)) * (0.55 + 0.45 * np.sin(2 * np.pi * 1.7 * t / sr))
    elif kind == 'noise':
        x = 0.1 * rng.randn(n)
    elif kind == 'faint':           # straddles the clip floor
        x = 3e-3 * rng.randn(n)
    elif kind == 'zeros':
        x = np.zeros(n)
    elif kind == 'impulse':
        x = np.zeros(n); x[n // 2] = 0.8
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


KINDS = ('sine', 'harmonic', 'noise', 'faint', 'zeros', 'impulse')


def write_wav_folder(path, sr, hop, seed=0, long_frames=None):
    """Seeded synthetic recordings as int16 wav files: a harmonic tone with a silent head and tail, noise, a file shorter than one hop, and
    (long_frames) one longer than long_frames frames.  Returns {basename: float signal as load_wav must return it}."""
    from scipy.io import wavfile
    os.makedirs(path, exist_ok=True)
    rng = np.random.RandomState(seed)
    sig = {}
    tone = make_signal('harmonic', 24 * hop, seed + 1, sr)
    sig['a_tone'] = np.concatenate([np.zeros(8192, np.float32), tone, np.zeros(6144, np.float32)])
    sig['b_noise'] = (0.2 * rng.randn(31 * hop + 17)).astype(np.float32)
    sig['c_short'] = (0.2 * rng.randn(hop - 5)).astype(np.float32)
    sig['d_noise2'] = (0.05 * rng.randn(12 * hop + 3)).astype(np.float32)
    if long_frames:
        sig['e_long'] = (0.1 * rng.randn((long_frames + 3) * hop)).astype(np.float32)
    out = {}
    for name, x in sig.items():
        q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        wavfile.write(os.path.join(path, name + '.wav'), sr, q)
        out[name] = q.astype(np.float32) / 32768.0
    return out


# ---- device parity (GPU): shared by tests/test_hip_mel.py and tools/mel_timing.py
CONFIGS = [
    ('fft1024', dict(n_fft=1024, win_size=1024, hop_size=256)),
    ('fft800', dict(n_fft=800, win_size=800, hop_size=200, num_mels=40)),
    ('power1_asym', dict(magnitude_power=1.0, symmetric_mels=False)),
    ('no_norm', dict(magnitude_power=1.0, symmetric_mels=False, signal_normalization=False)),
    ('noclip_sym', dict(allow_clipping_in_normalization=False)),
    ('noclip_asym', dict(allow_clipping_in_normalization=False, symmetric_mels=False)),
    ('power1p5', dict(magnitude_power=1.5)),
]
TILES = (32, 64, 128)


@contextlib.contextmanager
def pinned_tile(tf):
    """WN_MEL_TF is read by wn_mel_create: analyzers created inside run every call on that frame tile (None: the library's own per-call pick)"""
    old = os.environ.pop('WN_MEL_TF', None)
    if tf is not None:
        os.environ['WN_MEL_TF'] = str(tf)
    try:
        yield
    finally:
        os.environ.pop('WN_MEL_TF', None)
        if old is not None:
            os.environ['WN_MEL_TF'] = old


def boundary_lengths(hop, tf, max_frames=900, q=2):
    return [1, hop - 1, 3 * hop, (tf * q - 1) * hop, (tf * q) * hop, (tf * q + 1) * hop, (max_frames - 1) * hop + hop // 2]


def ragged_batch(hp, tf, max_frames=900):
    """every boundary length of tile tf once, every signal kind at least once (the kinds cycle over the lengths, shifted for the second pass)"""
    from datasets import audio
    lens = boundary_lengths(audio.get_hop_size(hp), tf, max_frames)
    sigs = []
    for i, n in enumerate(lens + lens[2:]):
        kind = KINDS[(i + (3 if i >= len(lens) else 0)) % len(KINDS)]
        sigs.append((kind, make_signal(kind, n, 100 + i, hp.sample_rate)))
    return sigs


def run_analyzer(an, wavs, channels_first=True, gain=None, frames=None):
    import torch
    lens = [len(w) for w in wavs]
    host = np.zeros((len(wavs), max(lens)), dtype=np.float32)
    for r, w in enumerate(wavs):
        host[r, :lens[r]] = w
    out = an.run(torch.from_numpy(host).cuda(), lens, gain=gain, channels_first=channels_first, frames=frames)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_ref_cache = {}


def check_parity(hp, label, max_frames=900, tile=None):
    """The ragged boundary batch of frame tile `tile` (None: the library's pick, boundaries of its largest tile) through an analyzer pinned to
    that tile, every utterance against the float64 reference within 8 x the floored float32 yardstick.  Prints each ratio before it asserts."""
    from wavenet_vocoder import _ext
    with pinned_tile(tile):
        probe = _ext.MelAnalyzer(hp, 1, 16)
        tf = probe.frame_tile
        probe.close()
        assert tile is None or tf == tile, (tf, tile)
        sigs = ragged_batch(hp, tf, max_frames)
        wavs = [w for _, w in sigs]
        an = _ext.MelAnalyzer(hp, len(wavs), max(len(w) for w in wavs))
        dev = run_analyzer(an, wavs, channels_first=True)
        an.close()
    rows, bad = [], []
    for r, (kind, w) in enumerate(sigs):
        key = (label, kind, len(w), r)
        if key not in _ref_cache:      # references and yardsticks do not depend on the tile
            ref = reference(w, hp)
            _ref_cache[key] = (ref,) + tolerance(w, hp, ref)
        ref, tol, yard = _ref_cache[key]
        fb = 1 + len(w) // an.hop
        assert ref.shape == (hp.num_mels, fb)
        err = float(np.max(np.abs(dev[r, :, :fb].astype(np.float64) - ref)))
        ratio = err / (tol / FACTOR)
        rows.append({'config': label, 'tile': tile or 'auto', 'signal': kind, 'samples': len(w), 'frames': fb, 'yardstick': yard, 'device_err': err,
                     'ratio_to_floored_yardstick': ratio})
        print('mel parity %-11s TF=%-4s %-9s n=%7d frames=%4d yardstick=%.3e device=%.3e ratio=%.2f' % (label, tile or 'auto', kind, len(w), fb, yard, err, ratio))
        if not err <= tol:
            bad.append(rows[-1])
    assert not bad, bad
    return rows
