"""CPU-only tests of the mel analysis surface: the C ABI declarations and wn_mel_create's validation (no GPU is touched before a
configuration is accepted), the frame count, the float32 yardstick the GPU tests take their tolerance from, the host half of
wavenet_preprocess (numpy mel path) on synthetic wav files, and load_wav."""
import os
import re

import numpy as np
import pytest
import torch

from mel_util import dft_matrix_mel, make_signal, mel_hparams, reference, tolerance, write_wav_folder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEL_SYMBOLS = ['wn_mel_create', 'wn_mel_destroy', 'wn_mel_last_error', 'wn_mel_num_frames', 'wn_mel_peak', 'wn_mel_run']


def test_header_declares_and_library_exports_the_mel_entry_points():
    from wavenet_vocoder import _ext
    header = open(os.path.join(ROOT, 'include', 'wavenet_mi355.h')).read()
    declared = set(re.findall(r'\b(wn_[a-z0-9_]+)\s*\(', header))
    syms = _ext.exported_symbols()
    lib = _ext.load_library()
    for s in MEL_SYMBOLS:
        assert s in declared and s in syms and hasattr(lib, s), s
    assert '#define WN_ABI_VERSION 4' in header and _ext.WN_ABI_VERSION == 4
    assert 'typedef struct wn_mel_config' in header
    for cite in ('audio.py:70-77', '178-182', '243-270'):      # every entry names the reference lines it replaces
        assert cite in header, cite


@pytest.mark.parametrize('over,code,field', [
    (dict(win_size=4096), -2, 'win_size'),
    (dict(n_fft=2047, win_size=1100), -2, 'n_fft'),
    (dict(hop_size=0), -2, 'hop_size'),
    (dict(num_mels=0), -2, 'num_mels'),
    (dict(magnitude_power=0.0), -1, 'magnitude_power'),
    (dict(magnitude_power=-1.0), -1, 'magnitude_power'),
])
def test_create_rejects_bad_fields_before_any_device_call(over, code, field):
    """max_batch = 1 asks for a device context: a WN_E_HIP here (no GPU on the CPU box) would mean the device was touched first"""
    from wavenet_vocoder import _ext
    hp = mel_hparams(**over)
    basis = np.zeros((max(1, hp.num_mels), 1 + hp.n_fft // 2), dtype=np.float32)
    cfg = _ext.mel_config_from_hparams(hp, 1, 1000)
    import ctypes
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    rc = lib.wn_mel_create(ctypes.byref(cfg), basis.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h))
    msg = (lib.wn_mel_last_error(None) or b'').decode()
    assert rc == code and not h.value and field in msg, (rc, msg)
    if hp.num_mels > 0:      # the same through the Python class (which refuses a basis that is not [num_mels, bins] itself)
        with pytest.raises(_ext.WnError) as ei:
            _ext.MelAnalyzer(hp, 1, 1000, mel_basis=basis)
        assert ei.value.code == code and field in str(ei.value), str(ei.value)


def test_create_rejects_null_and_foreign_abi():
    import ctypes
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    hp = mel_hparams()
    basis = np.zeros((80, 1025), dtype=np.float32)
    h = ctypes.c_void_p()
    cfg = _ext.mel_config_from_hparams(hp, 1, 1000)
    assert lib.wn_mel_create(ctypes.byref(cfg), None, ctypes.byref(h)) == -1 and b'mel_basis' in lib.wn_mel_last_error(None)
    cfg.abi_version = 3
    assert lib.wn_mel_create(ctypes.byref(cfg), basis.ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)) == -1 and b'abi_version' in lib.wn_mel_last_error(None)
    with pytest.raises(ValueError):
        _ext.MelAnalyzer(hp, 0, 0, mel_basis=np.zeros((80, 1024)))
    hp.use_lws = True
    with pytest.raises(NotImplementedError):
        _ext.MelAnalyzer(hp, 0, 0)


@pytest.mark.parametrize('hop', [275, 256, 1])
def test_num_frames_and_batch_bound_on_a_geometry_only_context(hop):
    from wavenet_vocoder import _ext
    an = _ext.MelAnalyzer(mel_hparams(hop_size=hop), 0, 0)        # max_batch = 0: no device
    for n in (0, 1, hop - 1, hop, hop + 1, 100 * hop):
        assert an.num_frames(n) == 1 + n // hop
    with pytest.raises(_ext.WnError):
        an.num_frames(-1)
    assert an.frame_tile == 0
    # B <= max_batch is checked before anything is read or launched (the pointers are never followed)
    import ctypes
    lens = (ctypes.c_int32 * 1)(10)
    rc = an.lib.wn_mel_run(an.h, ctypes.c_void_p(256), 16, lens, None, ctypes.c_void_p(256), 1, 1, 0, None)
    assert rc == -2 and b'max_batch' in an.lib.wn_mel_last_error(an.h)
    rc = an.lib.wn_mel_peak(an.h, ctypes.c_void_p(256), 16, lens, 1, ctypes.c_void_p(256), None)
    assert rc == -2 and b'max_batch' in an.lib.wn_mel_last_error(an.h)
    an.close()


def test_analyzer_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from wavenet_vocoder import _ext
    with pytest.raises(_ext.WnError) as ei:
        _ext.MelAnalyzer(mel_hparams(), 1, 1000)
    assert ei.value.code == -3            # WN_E_HIP: no device -> no silent CPU path


def test_float32_yardstick_against_float64_reference():
    """Guards the tests' own yardstick: the matrix formulation in float64 is the reference (to rounding), and in float32 its error is of
    the size the tolerance was designed around -- ~1e-6 on noise, ~1e-5 on harmonic + noise, ~1e-4 on a pure sine (deeply cancelled bins
    next to the clip floor), exactly 0 on an all-floor signal."""
    hp = mel_hparams()
    n = 120 * 275 + 31
    bounds = {'noise': (1e-7, 4e-6), 'harmonic': (1e-6, 5e-5), 'sine': (1e-5, 5e-4), 'zeros': (0.0, 0.0), 'faint': (1e-7, 4e-6), 'impulse': (1e-7, 4e-6)}
    for kind, (lo, hi) in bounds.items():
        w = make_signal(kind, n, 11)
        ref = reference(w, hp)
        assert ref.shape == (80, 1 + n // 275)
        d64 = np.max(np.abs(dft_matrix_mel(w.astype(np.float64), hp, np.float64) - ref))
        tol, yard = tolerance(w, hp, ref)
        print('yardstick %-9s f64 formulation %.2e  f32 yardstick %.3e' % (kind, d64, yard))
        assert d64 <= 1e-11, (kind, d64)
        assert lo <= yard <= hi, (kind, yard)
        assert tol == 8 * max(yard, 2.0 ** -19)
    for over in (dict(n_fft=1024, win_size=1024, hop_size=256), dict(n_fft=800, hop_size=200, win_size=800, num_mels=40), dict(magnitude_power=1.0, symmetric_mels=False),
                 dict(magnitude_power=1.0, symmetric_mels=False, signal_normalization=False), dict(magnitude_power=1.5)):
        hp2 = mel_hparams(**over)
        w = make_signal('harmonic', 9000, 5)
        assert np.max(np.abs(dft_matrix_mel(w.astype(np.float64), hp2, np.float64) - reference(w, hp2))) <= 1e-10


def _preprocess(tmp, wavs, hp, tag, n_jobs=1):
    from datasets import wavenet_preprocessor
    mel_dir, wav_dir = os.path.join(tmp, tag, 'mels'), os.path.join(tmp, tag, 'audio')
    os.makedirs(mel_dir); os.makedirs(wav_dir)
    rows = wavenet_preprocessor.build_from_path(hp, wavs, mel_dir, wav_dir, n_jobs=n_jobs)
    import wavenet_preprocess
    wavenet_preprocess.save_map(rows, os.path.join(tmp, tag))
    return rows


@pytest.mark.parametrize('input_type', ['raw', 'mulaw', 'mulaw-quantize'])
def test_build_from_path_numpy_mel(tmp_path, input_type):
    from wavenet_vocoder.util import mulaw, mulaw_quantize
    tmp = str(tmp_path)
    hp = mel_hparams(input_type=input_type, max_mel_frames=60, mi355_device_mel=False)
    if input_type == 'mulaw-quantize':
        hp.out_channels = 256
    hop = 275
    sig = write_wav_folder(os.path.join(tmp, 'wavs'), hp.sample_rate, hop, long_frames=60)
    rows = _preprocess(tmp, os.path.join(tmp, 'wavs'), hp, 'a', n_jobs=2 if input_type == 'raw' else 1)      # raw: through spawned workers
    rows_b = _preprocess(tmp, os.path.join(tmp, 'wavs'), hp, 'b')
    text = open(os.path.join(tmp, 'a', 'map.txt')).read()
    assert text.replace(os.path.join(tmp, 'a'), 'X') == open(os.path.join(tmp, 'b', 'map.txt')).read().replace(os.path.join(tmp, 'b'), 'X')      # two runs: the same map.txt
    lines = text.strip().split('\n')
    names = [os.path.basename(l.split('|')[0]) for l in lines]
    assert names == ['audio-a_tone.npy', 'audio-b_noise.npy', 'audio-c_short.npy', 'audio-d_noise2.npy']      # sorted; e_long (> max_mel_frames) dropped
    silence = {'raw': 0.0, 'mulaw': mulaw(0.0, hp.quantize_channels), 'mulaw-quantize': mulaw_quantize(0, hp.quantize_channels)}[input_type]
    for line, row, row_b in zip(lines, rows, rows_b):
        cols = line.split('|')
        assert len(cols) == 6 and cols[1] == cols[2] and cols[3] == '<no_g>'
        assert os.path.basename(cols[1]) == os.path.basename(cols[0]).replace('audio-', 'mel-')
        time_steps, mel_frames = int(cols[4]), int(cols[5])
        a, m = np.load(cols[0]), np.load(cols[1])
        assert time_steps == mel_frames * hop == len(a)
        assert m.dtype == np.float32 and m.shape == (mel_frames, hp.num_mels) and mel_frames <= 60
        assert a.dtype == (np.int16 if input_type == 'mulaw-quantize' else np.float32)
        assert np.abs(m).max() <= hp.max_abs_value
        assert np.array_equal(a, np.load(row_b[0])) and np.array_equal(m, np.load(row_b[1]))
        if input_type == 'mulaw-quantize':
            assert a.min() >= 0 and a.max() <= 255
        else:
            assert np.abs(a).max() <= 1.0
    by = {os.path.basename(l.split('|')[0]): (np.load(l.split('|')[0]), int(l.split('|')[5])) for l in lines}
    # c_short: fewer samples than one hop -> one frame, padded to one hop with the encoding's silence value
    a, frames = by['audio-c_short.npy']
    assert frames == 1 and len(a) == hop
    if input_type != 'mulaw-quantize':
        assert np.all(a[len(sig['c_short']):] == np.float32(silence)) and not np.all(a[:len(sig['c_short'])] == np.float32(silence))
    else:
        assert a[-1] == silence
    # a_tone: 8192 silent samples, 24 hops of tone, 6144 silent samples.  Trim frames are 2048 long every 512, centred: frame 15 is the
    # first to reach the tone (at 8192 = 16 x 512), frame 30 the last (the tone ends at 14792) -> [15 x 512, 31 x 512) = 8192 samples.
    a, frames = by['audio-a_tone.npy']
    if input_type != 'mulaw-quantize':
        assert frames == 1 + 8192 // hop and len(a) == frames * hop
        assert np.all(a[:512 - 8] == np.float32(silence)) and np.all(a[8192:] == np.float32(silence))
        assert np.abs(a[512:512 + 24 * hop]).max() > 0.5
    else:       # the mu-law silence trim cuts to the tone itself: just under 24 hops of samples
        assert frames == 24 and silence == 127
    # Feeder takes the folder as it is (construction and metadata only)
    from wavenet_vocoder.feeder import Feeder
    hp.parse('wavenet_batch_size=1,wavenet_test_batches=1')
    fd = Feeder(None, os.path.join(tmp, 'a', 'map.txt'), os.path.join(tmp, 'a'), hp, device=torch.device('cpu'))
    assert len(fd._train_meta) + len(fd._test_meta) == 4 and all(len(r) == 6 for r in fd._metadata)


def test_build_from_path_refuses_global_conditions_and_lws(tmp_path):
    from datasets import wavenet_preprocessor
    tmp = str(tmp_path)
    write_wav_folder(os.path.join(tmp, 'wavs'), 22050, 275)
    os.makedirs(os.path.join(tmp, 'm')); os.makedirs(os.path.join(tmp, 'a'))
    with pytest.raises(RuntimeError, match='gin_channels'):
        wavenet_preprocessor.build_from_path(mel_hparams(gin_channels=4, mi355_device_mel=False), os.path.join(tmp, 'wavs'), os.path.join(tmp, 'm'), os.path.join(tmp, 'a'), n_jobs=1)
    with pytest.raises(NotImplementedError):
        wavenet_preprocessor.build_from_path(mel_hparams(use_lws=True), os.path.join(tmp, 'wavs'), os.path.join(tmp, 'm'), os.path.join(tmp, 'a'), n_jobs=1)


def test_load_wav_scaling_and_rate_error(tmp_path):
    from scipy.io import wavfile
    from datasets import audio
    p = lambda n: os.path.join(str(tmp_path), n)
    i16 = np.array([0, 16384, -32768, 32767], dtype=np.int16)
    wavfile.write(p('i16.wav'), 22050, i16)
    assert np.array_equal(audio.load_wav(p('i16.wav'), 22050), i16.astype(np.float32) / 32768)
    i32 = np.array([0, 2 ** 30, -2 ** 31, 2 ** 31 - 1], dtype=np.int32)
    wavfile.write(p('i32.wav'), 22050, i32)
    assert np.array_equal(audio.load_wav(p('i32.wav'), 22050), (i32 / 2.0 ** 31).astype(np.float32))
    u8 = np.array([128, 0, 255, 192], dtype=np.uint8)
    wavfile.write(p('u8.wav'), 22050, u8)
    assert np.array_equal(audio.load_wav(p('u8.wav'), 22050), np.array([0, -1, 127 / 128, 0.5], dtype=np.float32))
    f32 = np.array([0.25, -0.5, 1.5, 0.0], dtype=np.float32)
    wavfile.write(p('f32.wav'), 22050, f32)
    got = audio.load_wav(p('f32.wav'), 22050)
    assert got.dtype == np.float32 and np.array_equal(got, f32)
    wavfile.write(p('stereo.wav'), 22050, np.stack([i16, i16[::-1]], axis=1))
    assert np.allclose(audio.load_wav(p('stereo.wav'), 22050), (i16.astype(np.float32) + i16[::-1]) / 2 / 32768, atol=1e-7)
    with pytest.raises(ValueError, match='i16.wav'):
        audio.load_wav(p('i16.wav'), 16000)


def test_host_audio_helpers():
    from scipy.signal import lfilter
    from datasets import audio
    x = make_signal('noise', 4000, 3).astype(np.float64)
    y = audio.preemphasis(x, 0.97)
    assert np.allclose(y[1:], x[1:] - 0.97 * x[:-1]) and y[0] == x[0]
    assert np.allclose(audio.inv_preemphasis(y, 0.97), x, atol=1e-9)
    assert audio.preemphasis(x, 0.97, False) is x and np.array_equal(audio.inv_preemphasis(y, 0.97), lfilter([1], [1, -0.97], y))
    q = np.full(100, 127); q[10] = 140; q[60] = 100; q[61] = 128
    assert audio.start_and_end_indices(q, 2) == (10, 60)
    assert audio.librosa_pad_lr(np.zeros(1000), 2048, 275) == (0, 100) and audio.librosa_pad_lr(np.zeros(1100), 2048, 275) == (0, 275)
    assert audio.librosa_pad_lr(np.zeros(1000), 2048, 275, pad_sides=2) == (50, 50)
    hp = mel_hparams()
    assert audio.trim_silence(np.zeros(0, np.float32), hp).size == 0 and audio.trim_silence(np.zeros(5000, np.float32), hp).size == 5000      # librosa: all frames at the maximum
    loud = make_signal('noise', 6000, 4)
    assert len(audio.trim_silence(loud, hp)) == 6000        # nothing to trim
