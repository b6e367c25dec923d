"""Spectral denoiser without a GPU: the ABI symbols and every validation code on a geometry-only handle; the float64 reference of tests/denoise_ref.py pinned
three ways (a brute-force DFT loop, scipy.signal.stft / istft where the conventions coincide, strength 0 as the identity); the properties derived from the
definition; the host hook wn_test_denoise_host under exactly the parity rule of the device tests (denoise_ref.check_rows / check_profile); five faults seeded
into the float32 stand-in, each caught by that rule; tests/host/denoise_main.cpp under ASAN + UBSAN as an ordinary program; and the Python plumbing."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5
SYMBOLS = ['wn_denoise_create', 'wn_denoise_destroy', 'wn_denoise_last_error', 'wn_denoise_num_frames', 'wn_denoise_fit', 'wn_denoise_set_profile',
           'wn_denoise_get_profile', 'wn_denoise_run', 'wn_test_denoise_host']


def test_abi_symbols_are_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    for s in SYMBOLS:
        assert re.search(r'\b%s\(' % s, text), s
        assert s in _ext.exported_symbols()
    assert 'wn_test_denoise_host(' in hooks and 'wn_denoise_run(' not in hooks
    assert re.search(r'#define WN_ABI_VERSION\s+4\b', text) and _ext.WN_ABI_VERSION == 4
    assert _ext.STATUS[WN_E_STATE] == 'WN_E_STATE'


def _create(n_fft, hop, rows=0, max_samples=0, abi=None):
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.denoise_config(n_fft, hop, rows, max_samples)
    if abi is not None:
        cfg.abi_version = abi
    h = ctypes.c_void_p()
    return lib.wn_denoise_create(ctypes.byref(cfg), ctypes.byref(h)), h, lib


def test_every_validation_code_on_a_geometry_only_handle():
    from wavenet_vocoder import _ext
    vp = ctypes.c_void_p
    for args, code in (((1023, 8), WN_E_SHAPE), ((6, 1), WN_E_SHAPE), ((64, 0), WN_E_SHAPE), ((64, 17), WN_E_SHAPE), ((100, 25), WN_E_UNSUPPORTED),
                       ((8192, 2048), WN_E_UNSUPPORTED), ((1024, 256), 0), ((2048, 512), 0), ((64, 16), 0)):
        rc, h, lib = _create(*args)
        assert rc == code, (args, rc)
        if rc == 0:
            lib.wn_denoise_destroy(h)
        else:
            assert lib.wn_denoise_last_error(None)
    assert _create(64, 16, abi=5)[0] == WN_E_ARG and _create(64, 16, rows=-1)[0] == WN_E_ARG
    lib = _ext.load_library()
    assert lib.wn_denoise_create(None, None) == WN_E_ARG
    rc, h, lib = _create(64, 16)
    assert rc == 0 and lib.wn_denoise_num_frames(h, 100) == 7 and lib.wn_denoise_num_frames(h, -1) == WN_E_ARG and lib.wn_denoise_num_frames(None, 1) == WN_E_ARG
    x = np.zeros(8, np.float32)
    xp = x.ctypes.data_as(vp)
    one, neg = (ctypes.c_int32 * 1)(4), (ctypes.c_int32 * 1)(-1)
    prof = np.ones(33, np.float32)
    run = lambda *a: lib.wn_denoise_run(h, *a)
    assert run(xp, 8, one, 1, 1.0, xp, 8, None) == WN_E_STATE                        # before any profile
    assert lib.wn_denoise_get_profile(h, prof.ctypes.data_as(vp), None) == WN_E_STATE
    assert b'profile' in lib.wn_denoise_last_error(h)
    bad = prof.copy()
    for v in (-1.0, np.nan, np.inf):
        bad[5] = v
        assert lib.wn_denoise_set_profile(h, bad.ctypes.data_as(vp), None) == WN_E_ARG
    assert lib.wn_denoise_set_profile(h, None, None) == WN_E_ARG
    assert lib.wn_denoise_set_profile(h, prof.ctypes.data_as(vp), None) == 0
    back = np.zeros(33, np.float32)
    assert lib.wn_denoise_get_profile(h, back.ctypes.data_as(vp), None) == 0 and np.array_equal(back, prof)
    assert lib.wn_denoise_get_profile(h, None, None) == WN_E_ARG
    assert run(None, 8, one, 1, 1.0, xp, 8, None) == WN_E_ARG
    assert run(xp, 8, None, 1, 1.0, xp, 8, None) == WN_E_ARG
    assert run(xp, 8, one, 1, 1.0, None, 8, None) == WN_E_ARG
    assert run(xp, 8, one, 0, 1.0, xp, 8, None) == WN_E_ARG
    assert run(xp, 8, neg, 1, 1.0, xp, 8, None) == WN_E_ARG
    for s in (-0.5, float('nan'), float('inf')):
        assert run(xp, 8, one, 1, s, xp, 8, None) == WN_E_ARG
    assert run(xp, 8, one, 1, 1.0, xp, 8, None) == WN_E_SHAPE                        # B > max_batch = 0: a geometry-only handle refuses every batch
    assert lib.wn_denoise_fit(h, xp, 8, one, 1, None) == WN_E_SHAPE
    assert lib.wn_denoise_fit(h, None, 8, one, 1, None) == WN_E_ARG
    assert lib.wn_denoise_fit(None, xp, 8, one, 1, None) == WN_E_ARG
    lib.wn_denoise_destroy(h)
    # the shapes of a batch, through the host hook (no max_batch there): a length above either pitch
    with pytest.raises(_ext.WnError) as e:
        _ext.denoise_host(64, 16, np.zeros((1, 8), np.float32), [9], 1.0, profile=prof)
    assert e.value.code == WN_E_SHAPE


# ---- the reference, pinned three ways
def test_reference_against_a_brute_force_dft():
    n_fft, hop = 64, 16
    x = R.signal('tone', 150, 3, n_fft).astype(np.float64)
    X = R.stft(x, n_fft, hop)
    w = R.window(n_fft)
    H = n_fft // 2
    for f in (0, 3, X.shape[0] - 1):
        for k in (0, 1, 7, H):
            acc = 0j
            for j in range(n_fft):
                s = f * hop - H + j
                acc += w[j] * (x[s] if 0 <= s < len(x) else 0.0) * np.exp(-2j * np.pi * j * k / n_fft)
            assert abs(acc - X[f, k]) < 1e-12
    prof = R.noise_profile(n_fft, hop).astype(np.float64)
    Y = R.shrink(X, 1.0 * prof[None, :])
    out = R.denoise(x, prof, 1.0, n_fft, hop)
    for i in (0, 1, 40, 149):
        num = den = 0.0
        for f in range(X.shape[0]):
            j = i - f * hop + H
            if 0 <= j < n_fft:
                yj = (Y[f, 0].real + Y[f, H].real * (-1) ** j + 2 * sum((Y[f, k] * np.exp(2j * np.pi * j * k / n_fft)).real for k in range(1, H))) / n_fft
                num += w[j] * yj
                den += w[j] ** 2
        assert abs(num / den - out[i]) < 1e-12


def test_reference_against_scipy_where_the_conventions_coincide():
    from scipy import signal
    for n_fft, hop in ((64, 16), (96, 24), (1024, 256)):
        n = 7 * hop                                                   # a multiple of hop: scipy's zero boundary then frames as the reference does
        x = R.signal('tone', n, 4, n_fft).astype(np.float64)
        _, _, Z = signal.stft(x, window='hann', nperseg=n_fft, noverlap=n_fft - hop, boundary='zeros', padded=True)
        w = R.window(n_fft)
        X = R.stft(x, n_fft, hop)
        Zs = Z.T * w.sum()                                            # scaling undone
        F = X.shape[0]
        assert Zs.shape[0] >= F and np.max(np.abs(Zs[:F] - X)) < 1e-10
        prof = R.noise_profile(n_fft, hop).astype(np.float64)
        Y = np.zeros_like(Zs); Y[:F] = R.shrink(X, 0.5 * prof[None, :])
        _, back = signal.istft((Y / w.sum()).T, window='hann', nperseg=n_fft, noverlap=n_fft - hop, boundary=True)
        got = R.denoise(x, prof, 0.5, n_fft, hop)
        # scipy adds the frames beyond F (zeros here) to its window sum: the interior, where both sums cover the same frames, coincides
        lo, hi = 0, n - n_fft // 2
        assert np.max(np.abs(back[lo:hi] - got[lo:hi])) < 1e-10


@pytest.mark.parametrize('geo', [(64, 16), (96, 24), (1024, 256)])
def test_strength_zero_is_the_identity(geo):
    n_fft, hop = geo
    prof = np.ones(1 + n_fft // 2)
    for n in (1, 15, 16, 17, 100, 32 * hop, 32 * hop - 1, 32 * hop + 1, 3000):
        x = R.signal('tone', n, n, n_fft).astype(np.float64)
        assert np.max(np.abs(R.denoise(x, prof, 0.0, n_fft, hop) - x)) < 1e-12, n


# ---- derived properties
@pytest.mark.parametrize('geo', [(64, 16), (96, 20), (32, 1), (64, 5)])
def test_window_square_sum_floor(geo):
    n_fft, hop = geo
    wsq, H = R.window(n_fft) ** 2, n_fft // 2
    for n in range(1, 4 * n_fft + 1):
        F = 1 + n // hop
        den = np.zeros((F - 1) * hop + n_fft)
        for f in range(F):
            den[f * hop:f * hop + n_fft] += wsq
        assert den[H:H + n].min() >= 0.25, n


def test_shrink_properties():
    n_fft, hop = 96, 20
    prof = R.noise_profile(n_fft, hop).astype(np.float64)
    x = R.signal('tone', 700, 2, n_fft).astype(np.float64)
    X = R.stft(x, n_fft, hop)
    energy = []
    for s in (0.0, 0.25, 0.5, 1.0, 2.0, 4.0, 16.0):
        Y = R.shrink(X, s * prof[None, :])
        assert np.all(np.abs(Y) <= np.abs(X) + 1e-15)
        energy.append(float(np.sum(R.denoise(x, prof, s, n_fft, hop) ** 2)))
    assert all(b <= a * (1 + 1e-12) for a, b in zip(energy, energy[1:]))
    big = 1.01 * np.max(np.abs(X) / prof[None, :])
    assert np.all(R.denoise(x, prof, big, n_fft, hop) == 0.0)
    with pytest.raises(ValueError):
        R.fit([x[:n_fft - 1]], n_fft, hop)
    assert len(R.inside(64, 64, 16)) == 1 and len(R.inside(96, 96, 20)) == 0      # one whole window; none when no frame centre sits n_fft / 2 from both ends


# ---- the host hook under the device tests' rule
@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ['A', 'B'])
def test_host_hook_every_sample_against_float64(name, kind):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    prof = R.noise_profile(n_fft, hop)
    ls = R.lengths_of(n_fft, hop)
    for s in R.STRENGTHS:
        for i in range(0, 12, 3):
            lens = ls[i:i + 3]
            wav = R.batch(kind, lens, 200 + i, n_fft)
            got, _ = _ext.denoise_host(n_fft, hop, wav, lens, s, profile=prof)
            assert np.array_equal(np.isnan(got), np.isnan(wav))               # nothing beyond a row's length is read or written
            if kind == 'zeros':
                assert all(np.all(got[b, :n] == 0.0) for b, n in enumerate(lens))
            assert R.check_rows(got, wav, lens, prof, s, n_fft, hop)[0] <= 1.0, (s, lens)


def test_host_hook_production_geometry_and_fit():
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES['P']
    prof = R.noise_profile(n_fft, hop)
    lens = [3000, 0, 1500]
    wav = R.batch('tone', lens, 7, n_fft)
    got, _ = _ext.denoise_host(n_fft, hop, wav, lens, 1.0, profile=prof)
    w, scale = R.check_rows(got, wav, lens, prof, 1.0, n_fft, hop)
    assert w <= 1.0 and scale < 64
    for name in ('A', 'B'):
        n_fft, hop = R.GEOMETRIES[name]
        rows = [R.signal('straddle', n, 9 + i, n_fft) for i, n in enumerate([3 * n_fft + 5, n_fft - 1, 40 * hop + 3])]
        fw = np.full((3, max(len(r) for r in rows) + 2), np.nan, np.float32)
        for i, r in enumerate(rows):
            fw[i, :len(r)] = r
        _, p = _ext.denoise_host(n_fft, hop, fit_wav=fw, fit_lengths=[len(r) for r in rows])
        assert R.check_profile(p, rows, n_fft, hop) <= 1.0
        with pytest.raises(_ext.WnError) as e:                                # a signal shorter than n_fft is refused
            _ext.denoise_host(n_fft, hop, fit_wav=fw[:1], fit_lengths=[n_fft - 1])
        assert e.value.code == WN_E_SHAPE


@pytest.mark.parametrize('fault', R.FAULTS)
def test_a_seeded_fault_is_caught(fault):
    """the stand-in with one mistake seeded misses the rule by far on at least one geometry's tone; without it, it passes by construction (it IS the yardstick)"""
    caught = []
    for name in ('A', 'B'):
        n_fft, hop = R.GEOMETRIES[name]
        prof = R.noise_profile(n_fft, hop)
        x = R.signal('tone', 40 * hop + 3, 3, n_fft)
        ref = R.denoise(x, prof, 1.0, n_fft, hop)
        bound, _ = R.row_bound(x, ref, prof, 1.0, n_fft, hop)
        err = float(np.max(np.abs(R.standin(x, prof, 1.0, n_fft, hop, fault=fault).astype(np.float64) - ref)))
        caught.append(err > bound)
    assert all(caught), fault


# ---- the stand-alone host program
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/denoise_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('denoise') / 'denoise_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'denoise_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    r = host_program
    assert r.returncode == 0 and 'denoise ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = {l.split()[1]: int(l.split()[2]) for l in host_program.stdout.splitlines() if l.startswith('code ')}
    want = {'cfg_null': WN_E_ARG, 'cfg_ok': 0, 'cfg_abi': WN_E_ARG, 'cfg_batch_neg': WN_E_ARG, 'cfg_batch_zero': 0, 'cfg_samples_neg': WN_E_ARG,
            'cfg_fft_odd': WN_E_SHAPE, 'cfg_fft_small': WN_E_SHAPE, 'cfg_hop_zero': WN_E_SHAPE, 'cfg_hop_over': WN_E_SHAPE, 'cfg_hop_quarter': 0,
            'cfg_fft_not_32': WN_E_UNSUPPORTED, 'cfg_fft_large': WN_E_UNSUPPORTED, 'cfg_2048_512': 0, 'cfg_4096_1024': 0,
            'run_ok': 0, 'run_wav_null': WN_E_ARG, 'run_lengths_null': WN_E_ARG, 'run_b_zero': WN_E_ARG, 'run_pitch_negative': WN_E_ARG,
            'run_length_negative': WN_E_ARG, 'run_b_over': WN_E_SHAPE, 'run_pitch_short': WN_E_SHAPE, 'run_length_over': WN_E_SHAPE,
            'strength_zero': 0, 'strength_neg': WN_E_ARG, 'strength_nan': WN_E_ARG, 'strength_inf': WN_E_ARG,
            'profile_ok': 0, 'profile_null': WN_E_ARG, 'profile_neg': WN_E_ARG, 'profile_nan': WN_E_ARG, 'profile_inf': WN_E_ARG}
    assert got == want


# ---- Python plumbing
def test_hparams_and_the_silent_conditioning_value():
    import hparams as H
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import silent_conditioning_value
    hp = H._build()
    assert hp.mi355_output_denoise == 0.0 and _ext.denoise_geometry(hp) == (1024, 256)
    assert hp.mi355_output_denoise_profile_frames == 64 and hp.mi355_output_denoise_speaker == 0
    hp.parse('normalize_for_wavenet=False')
    assert silent_conditioning_value(hp) == -hp.max_abs_value                # the pad value of wn_mel_run and the synthesiser, through the normalisation code
    hp.parse('normalize_for_wavenet=True')
    assert silent_conditioning_value(hp) == 0.0


class _StubDenoiser:
    def __init__(self, rows, max_samples, log):
        self.rows, self.max_samples, self.log, self._p = rows, max_samples, log, np.arange(3, dtype=np.float32)
        log.append(('create', rows, max_samples))

    profile = property(lambda self: self._p, lambda self, v: (self.log.append(('set_profile',)), setattr(self, '_p', v))[0])

    def apply(self, wav, lengths, strength, out=None):
        self.log.append(('apply', list(lengths), strength, out is wav))
        return out

    def close(self):
        self.log.append(('close', self.rows))


def test_synthesizer_plumbing_with_a_stub_handle():
    import hparams as H
    from wavenet_vocoder.synthesizer import Synthesizer
    log = []
    syn = Synthesizer.__new__(Synthesizer)
    syn._hparams = H._build().parse('mi355_output_denoise=0.5')

    class Model:
        def denoiser(self, rows, max_samples):
            return _StubDenoiser(rows, max_samples, log)
    syn.model = Model()
    syn._denoiser = _StubDenoiser(1, 100, log)
    rows = object()
    assert syn._denoise(rows, [50]) is rows and log[-1] == ('apply', [50], 0.5, True)
    assert syn._denoise(rows, [50, 300]) is rows                               # too small: a larger handle takes the profile over, the old one is closed
    assert log[-4:] == [('create', 2, 300), ('set_profile',), ('close', 1), ('apply', [50, 300], 0.5, True)]
    syn._hparams.parse('mi355_output_denoise=-1')
    with pytest.raises(ValueError):
        syn._denoise(rows, [5])


def test_strength_zero_creates_no_handle():
    import hparams as H
    from wavenet_vocoder.synthesizer import Synthesizer
    syn = Synthesizer()
    syn.load(None, H._build().parse('mi355_output_denoise=0.0'))
    assert syn._denoiser is None and syn.model.engine is None                  # nothing built, nothing fitted
    rows = object()
    assert syn._denoise(rows, [5]) is rows


def test_eval_step_writes_and_scores_the_denoised_item(tmp_path, monkeypatch):
    """eval_step with mi355_output_denoise > 0 and a stub handle: the wav written and the waveform both checks score are the stub's output, the handle is
    created and fitted once per model (not once per eval) and replaced, profile kept, by a larger one for a longer item; at 0 nothing of it runs"""
    import io
    import json
    import torch
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder import train as T
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a, **k: None)
    log, scored = [], {}

    class Stub(_StubDenoiser):
        def fit_from_model(self, frames=None):
            self.log.append(('fit_from_model',))
            return self

        def apply(self, wav, lengths, strength, out=None):
            self.log.append(('apply', list(lengths), strength, out is wav))
            out.mul_(-0.5)
            return out

    class Check:
        hop = 16

        def __init__(self, name):
            self.name = name

        def score(self, wav, *a, **k):
            scored[self.name] = wav.clone()
            return [np.arange(9, dtype=np.float32)]

        def close(self):
            pass

    class Model:
        def __init__(self, n):
            self.n = n

        def initialize(self, y, c, g, lengths):
            self.tower_y_hat = [torch.linspace(-0.8, 0.8, self.n)]
            self.tower_y_target = [torch.zeros(self.n)]
            self.tower_eval_c = [torch.zeros(16, self.n // 16)]
            self.tower_eval_upsampled_local_features = [torch.zeros(16, self.n)]
            self.eval_loss = torch.tensor(1.5)

        def denoiser(self, rows, max_samples):
            return Stub(rows, max_samples, log)

        def reconstruction_check(self, rows, n):
            return Check('reconstruction')

        def pitch_check(self, rows, n):
            return Check('pitch')

    def run(model, step, extra):
        hp = H._build().parse('mi355_reconstruction_check=True,mi355_pitch_check=True,mi355_output_denoise_profile_frames=2,hop_size=16' + extra)
        out = io.StringIO()
        T.eval_step(model, (None, None, [model.n], None, None), step, str(tmp_path), str(tmp_path), out, hp, 'WaveNet')
        return json.loads(out.getvalue()), wavfile.read(str(tmp_path / ('step-%d-pred.wav' % step)))[1]

    m = Model(320)
    raw = torch.linspace(-0.8, 0.8, 320)
    row0, pcm0 = run(m, 1, '')
    assert not log and torch.equal(scored['reconstruction'].reshape(-1), raw) and torch.equal(scored['pitch'].reshape(-1), raw)
    row1, pcm1 = run(m, 2, ',mi355_output_denoise=0.5')
    den = raw * -0.5
    assert log == [('create', 1, 320), ('fit_from_model',), ('apply', [320], 0.5, True)]
    assert torch.equal(scored['reconstruction'].reshape(-1), den) and torch.equal(scored['pitch'].reshape(-1), den)          # both checks score the denoised item
    assert np.array_equal(pcm1, (den.numpy() * (32767 / 0.4)).astype(np.int16)) and not np.array_equal(pcm1, pcm0)            # and the wav is the denoised item
    assert set(row1) == set(row0) and len(row1) == 7          # step, loss, two reconstruction scalars, three pitch scalars
    run(m, 3, ',mi355_output_denoise=0.5')
    assert log[3:] == [('apply', [320], 0.5, True)]                                  # the second eval fits nothing
    m.n = 480
    run(m, 4, ',mi355_output_denoise=0.5')
    assert log[4:] == [('create', 1, 480), ('set_profile',), ('close', 1), ('apply', [480], 0.5, True)]
