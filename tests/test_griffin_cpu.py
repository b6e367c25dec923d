"""Griffin-Lim baseline without a GPU: the ABI symbols and every validation code on a geometry-only handle; the float64 reference of tests/griffin_ref.py
pinned four ways (a brute-force DFT loop, the float64 analysis tests/mel_util.py holds, ISTFT(STFT(x)) == x, scipy.signal.stft / istft where the conventions
coincide); the window-square sum of every trimmed sample; the host hook wn_test_griffin_host under exactly the staged rule of the device tests; whole runs
by their properties; five faults seeded into the float32 stand-in, each caught by that rule; tests/host/griffin_main.cpp under ASAN + UBSAN as an
ordinary program; the numpy inversion of datasets.audio; and the Python plumbing (hparams, the Synthesizer's baseline, the command line) on stand-ins."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import griffin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5
SYMBOLS = ['wn_griffin_create', 'wn_griffin_destroy', 'wn_griffin_last_error', 'wn_griffin_num_samples', 'wn_griffin_run', 'wn_test_griffin_store_spectrum',
           'wn_test_griffin_copy', 'wn_test_griffin_host']
SMALL = ('A', 'B', 'C')


def test_abi_symbols_are_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    for s in SYMBOLS:
        assert re.search(r'\b%s\(' % s, text), s
        assert s in _ext.exported_symbols()
    assert 'wn_test_griffin_host(' in hooks and 'wn_griffin_run(' not in hooks
    assert re.search(r'#define WN_ABI_VERSION\s+4\b', text) and _ext.WN_ABI_VERSION == 4      # additions only


def _create(n_fft, win, hop, rows=0, max_frames=0, abi=None, **kw):
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.griffin_config(n_fft, win, hop, max_batch=rows, max_frames=max_frames, **kw)
    if abi is not None:
        cfg.abi_version = abi
    h = ctypes.c_void_p()
    return lib.wn_griffin_create(ctypes.byref(cfg), None, ctypes.byref(h)), h, lib


def test_every_validation_code_on_a_geometry_only_handle():
    from wavenet_vocoder import _ext
    vp = ctypes.c_void_p
    for args, code in (((2047, 1100, 275), WN_E_SHAPE), ((6, 4, 1), WN_E_SHAPE), ((64, 65, 16), WN_E_SHAPE), ((64, 48, 0), WN_E_SHAPE), ((64, 48, 13), WN_E_SHAPE),
                       ((64, 64, 17), WN_E_SHAPE), ((100, 100, 25), WN_E_UNSUPPORTED), ((8192, 8192, 2048), WN_E_UNSUPPORTED), ((2048, 1100, 275), 0),
                       ((4096, 4096, 1024), 0), ((64, 48, 12), 0), ((1024, 1024, 256), 0)):
        rc, h, lib = _create(*args)
        assert rc == code, (args, rc)
        if rc == 0:
            lib.wn_griffin_destroy(h)
        else:
            assert lib.wn_griffin_last_error(None)
    assert _create(64, 48, 12, abi=5)[0] == WN_E_ARG and _create(64, 48, 12, rows=-1)[0] == WN_E_ARG and _create(64, 48, 12, max_frames=-1)[0] == WN_E_ARG
    assert _create(64, 48, 12, power=0.0)[0] == WN_E_ARG and _create(64, 48, 12, magnitude_power=float('nan'))[0] == WN_E_ARG
    assert _create(64, 48, 12, num_mels=513)[0] == WN_E_ARG
    lib = _ext.load_library()
    assert lib.wn_griffin_create(None, None, None) == WN_E_ARG
    rc, h, lib = _create(64, 48, 12)
    assert rc == 0 and lib.wn_griffin_num_samples(h, 33) == 12 * 32 and lib.wn_griffin_num_samples(h, 0) == WN_E_ARG and lib.wn_griffin_num_samples(None, 2) == WN_E_ARG
    x = np.zeros(3 * 33, np.float32)
    xp = x.ctypes.data_as(vp)
    three, one = (ctypes.c_int32 * 1)(3), (ctypes.c_int32 * 1)(1)
    run = lambda *a: lib.wn_griffin_run(h, *a)
    assert run(None, 2, 3, three, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG
    assert run(xp, 2, 3, None, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG
    assert run(xp, 3, 3, three, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG                 # src_kind
    assert run(xp, 0, 3, three, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG                 # a mel on a handle without pinv
    assert run(xp, 2, 3, three, 0, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG
    assert run(xp, 2, 3, three, 1, None, None, 0, -1, 0, xp, 40, None) == WN_E_ARG
    assert run(xp, 2, 3, three, 1, None, None, 0, 1, 2, xp, 40, None) == WN_E_ARG                 # unknown flags
    assert run(xp, 2, 3, three, 1, None, None, 0, 1, 0, xp, -1, None) == WN_E_ARG
    assert run(xp, 2, 3, one, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_SHAPE                 # F < 2
    assert run(xp, 2, 3, three, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_SHAPE               # B > max_batch = 0: a geometry-only handle refuses every batch
    assert b'max_batch' in lib.wn_griffin_last_error(h)
    assert run(None, 0, 0, None, 0, None, None, 0, 1, 1, xp, 40, None) == WN_E_STATE              # a continuation before any run
    assert lib.wn_griffin_run(None, xp, 2, 3, three, 1, None, None, 0, 1, 0, xp, 40, None) == WN_E_ARG
    assert lib.wn_test_griffin_store_spectrum(h, 1) == WN_E_STATE and lib.wn_test_griffin_copy(h, 0, xp, 3, None) == WN_E_STATE
    lib.wn_griffin_destroy(h)
    # the shapes of a batch, through the host hook (no max_batch there)
    cfg = _ext.griffin_config(64, 48, 12)
    S = np.zeros((1, 5, 33), np.float32)
    for frames, kw in (([6], {}), ([1], {}), ([5], {'y0': np.zeros((1, 47), np.float32)})):
        with pytest.raises(_ext.WnError) as e:
            _ext.griffin_host(cfg, S, frames, **kw)
        assert e.value.code == WN_E_SHAPE, frames
    with pytest.raises(_ext.WnError) as e:
        _ext.griffin_host(_ext.griffin_config(64, 48, 12, num_mels=7), np.zeros((1, 5, 7), np.float32), [5], kind='mel')      # a mel without the pseudo-inverse
    assert e.value.code == WN_E_ARG


# ---- the reference, pinned four ways
def test_reference_against_a_brute_force_dft():
    geo = R.GEOMETRIES['A']
    n_fft, win, hop = geo
    F = 14
    x = R.signal('tones', R.num_samples(F, hop), 3, n_fft).astype(np.float64)
    X = R.stft(x, F, geo)
    w = R.window(n_fft, win)
    H = n_fft // 2
    assert w[(n_fft - win) // 2 - 1] == 0 and w[(n_fft - win) // 2 + 1] > 0 and abs(w[H] - 1.0) < 1e-15      # centred in n_fft
    for f in (0, 3, F - 1):
        for k in (0, 1, 7, H):
            acc = 0j
            for j in range(n_fft):
                s = f * hop - H + j
                acc += w[j] * (x[s] if 0 <= s < len(x) else 0.0) * np.exp(-2j * np.pi * j * k / n_fft)
            assert abs(acc - X[f, k]) < 1e-12
    S = np.abs(X) * 0.5 + 0.1
    Y = R.project(X, S)
    out = R.istft(Y, F, geo)
    assert len(out) == hop * (F - 1)
    for i in (0, 1, 40, len(out) - 1):
        num = den = 0.0
        for f in range(F):
            j = i - f * hop + H
            if 0 <= j < n_fft:
                yj = (Y[f, 0].real + Y[f, H].real * (-1) ** j + 2 * sum((Y[f, k] * np.exp(2j * np.pi * j * k / n_fft)).real for k in range(1, H))) / n_fft
                num += w[j] * yj
                den += w[j] ** 2
        assert abs(num / den - out[i]) < 1e-12
    Z = np.zeros((2, H + 1), complex); Z[0, 3] = 1e-300
    P = R.project(Z, np.ones((2, H + 1)))
    assert P[1, 3] == 1.0 and abs(P[0, 3] - 1.0) < 1e-15 and np.all(P[1] == 1.0)      # an exactly zero bin takes the phase (1, 0)


def test_reference_against_the_float64_mel_analysis():
    """the forward transform through the analysis tests/mel_util.py holds (datasets.audio.melspectrogram, pinned by test_host_cpu.py): the mel of |STFT| equals it"""
    import mel_util as MU
    from datasets import audio
    for n_fft, win, hop in (R.GEOMETRIES['A'], R.GEOMETRIES['B'], (2048, 1100, 275)):
        hp = MU.mel_hparams(n_fft=n_fft, win_size=win, hop_size=hop, num_mels=12 if n_fft < 100 else 80, sample_rate=22050)
        F = 9
        x = R.signal('tones', R.num_samples(F, hop), 5, n_fft).astype(np.float64)
        X = R.stft(x, F, (n_fft, win, hop))
        assert np.max(np.abs(audio._stft(x, hp).T - X)) < 1e-11 * max(1.0, np.max(np.abs(X)))
        M = (np.abs(X) ** hp.magnitude_power) @ audio._build_mel_basis(hp).astype(np.float64).T
        mel = audio._normalize(audio._amp_to_db(M, hp) - hp.ref_level_db, hp).T
        assert np.max(np.abs(mel - MU.reference(x, hp))) < 1e-9


def test_reference_inverse_of_the_forward_is_the_identity():
    for name, geo in R.GEOMETRIES.items():
        for F in ((2, 33) if name == 'P' else R.FRAMES):
            x = R.signal('noise', R.num_samples(F, geo[2]), F, geo[0]).astype(np.float64)
            assert np.max(np.abs(R.istft(R.stft(x, F, geo), F, geo) - x)) < 1e-12, (name, F)


def test_reference_against_scipy_where_the_conventions_coincide():
    from scipy import signal
    for geo in (R.GEOMETRIES['A'], R.GEOMETRIES['B'], R.GEOMETRIES['C'], (1024, 800, 200)):
        n_fft, win, hop = geo
        F = 8
        n = R.num_samples(F, hop)                                     # a multiple of hop: scipy's zero boundary then frames as the reference does
        x = R.signal('tones', n, 2, n_fft).astype(np.float64)
        w = R.window(n_fft, win)
        _, _, Z = signal.stft(x, window=w, nperseg=n_fft, noverlap=n_fft - hop, nfft=n_fft, boundary='zeros', padded=False, return_onesided=True)
        X = R.stft(x, F, geo)
        assert Z.shape[1] == F and np.max(np.abs(Z.T * w.sum() - X)) < 1e-10
        Y = R.project(X, np.abs(X) * 0.7 + 0.05)
        _, y = signal.istft(Y.T / w.sum(), window=w, nperseg=n_fft, noverlap=n_fft - hop, nfft=n_fft, boundary=True)
        assert len(y) == n and np.max(np.abs(y - R.istft(Y, F, geo))) < 1e-10


def test_window_square_sum_is_positive_for_every_trimmed_sample():
    """hop <= win_size / 4 keeps it positive; at the test geometries its smallest value is 1.25 (the first sample: frame 0 at the window's centre, frame 1 a
    quarter window away)"""
    for name in SMALL:
        geo = R.GEOMETRIES[name]
        m = min(float(R.window_square_sum(F, geo).min()) for F in R.FRAMES)
        assert abs(m - 1.25) < 1e-12, (name, m)
    assert min(float(R.window_square_sum(F, R.GEOMETRIES['P']).min()) for F in (2, 40)) > 1.0
    assert float(R.window_square_sum(9, (32, 30, 7)).min()) > 0.5 and float(R.window_square_sum(2, (32, 4, 1)).min()) > 0.5


# ---- the host hook under the staged rule of the device tests
def _case(kind, frames, geo, seed, pad=3):
    B, Fm, nb = len(frames), max(frames) + pad, 1 + geo[0] // 2
    S = np.zeros((B, Fm, nb), np.float32)
    u = np.zeros((B, Fm, nb), np.float32)
    y0 = np.zeros((B, geo[2] * (Fm - 1)), np.float32)
    for b, F in enumerate(frames):
        S[b, :F], x = R.target(kind, F, seed + 7 * b, geo)
        u[b, :F] = R.uniforms(F, geo, seed + 100 + b)
        y0[b, :len(x)] = 0.0 if kind == 'zeros' else R.signal('noise', len(x), seed + 50 + b, geo[0])
    return S, u, y0


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', SMALL)
def test_host_hook_stage_by_stage(name, kind):
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES[name]
    cfg = _ext.griffin_config(*geo)
    worst = [0.0, 0.0, 0.0]
    for i, frames in enumerate(([65], [2], [31, 65, 2], [33, 32, 31])):
        S, u, y0 = _case(kind, frames, geo, 10 * i + 1)
        out, mag, X = _ext.griffin_host(cfg, S, frames, y0=y0, iters=1, return_all=True, fill=-7.25)
        st = _ext.griffin_host(cfg, S, frames, u=u, iters=0, fill=-7.25)
        zp, z0 = _ext.griffin_host(cfg, S, frames, iters=0), _ext.griffin_host(cfg, S, frames, u=np.zeros_like(u), iters=0)
        assert np.array_equal(zp, z0)                                  # the zero-phase start is the start from u = 0
        for b, F in enumerate(frames):
            n = R.num_samples(F, geo[2])
            assert np.array_equal(mag[b, :F], S[b, :F]) and np.all(out[b, n:] == -7.25) and np.all(st[b, n:] == -7.25)
            if kind == 'zeros':
                assert np.all(out[b, :n] == 0.0) and np.all(st[b, :n] == 0.0)
            for j, w in enumerate((R.check_spectrum(X[b, :F], y0[b, :n], F, geo)[0], R.check_output(out[b, :n], X[b, :F], S[b, :F], F, geo)[0],
                                   R.check_start(st[b, :n], S[b, :F], u[b, :F], F, geo)[0])):
                worst[j] = max(worst[j], w)
    print('%s %-8s spectrum %.3f output %.3f start %.3f (error / bound)' % (name, kind, *worst))
    assert max(worst) <= 1.0, worst


def test_host_hook_production_geometry():
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES['P']
    frames = [33, 2]
    S, u, y0 = _case('tones', frames, geo, 3, pad=0)
    out, _, X = _ext.griffin_host(_ext.griffin_config(*geo), S, frames, y0=y0, iters=1, return_all=True)
    for b, F in enumerate(frames):
        n = R.num_samples(F, geo[2])
        assert R.check_spectrum(X[b, :F], y0[b, :n], F, geo)[0] <= 1.0 and R.check_output(out[b, :n], X[b, :F], S[b, :F], F, geo)[0] <= 1.0


def _mel_case(name, variant, frames, seed, num_mels=12):
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES[name]
    lv = R.mel_level(variant)
    basis = R.mel_basis(num_mels, geo[0])
    pinv = R.pinv_of(basis)
    mel = np.zeros((len(frames), max(frames) + 2, num_mels), np.float32)
    for b, F in enumerate(frames):
        S, _ = R.target('tones' if b % 2 == 0 else 'noise', F, seed + b, geo)
        mel[b, :F] = R.normalised_mel(S, basis, lv)
    if lv['clip']:
        mel[0, 0, :3] = (9.0, -9.0, 4.0)
    cfg = _ext.griffin_config(*geo, num_mels=num_mels, magnitude_power=lv['magnitude_power'], power=lv['power'], min_level_db=lv['lo'], ref_level_db=lv['ref'],
                              max_abs_value=lv['maxabs'], signal_normalization=lv['norm'], allow_clipping=lv['clip'], symmetric_mels=lv['sym'])
    return geo, lv, pinv, mel, cfg


@pytest.mark.parametrize('variant', sorted(R.MEL_VARIANTS))
def test_host_hook_magnitudes_from_a_mel(variant):
    from wavenet_vocoder import _ext
    frames = [33, 2, 9]
    for name in ('A', 'B'):
        geo, lv, pinv, mel, cfg = _mel_case(name, variant, frames, 5)
        _, mag, _ = _ext.griffin_host(cfg, mel, frames, kind='mel', pinv=pinv, return_all=True)
        _, mag_cf, _ = _ext.griffin_host(cfg, np.ascontiguousarray(mel.transpose(0, 2, 1)), frames, kind='mel_cf', pinv=pinv, return_all=True)
        for b, F in enumerate(frames):
            assert np.array_equal(mag[b, :F], mag_cf[b, :F])
            assert R.check_magnitudes(mag[b, :F], mel[b, :F], pinv, lv)[0] <= 1.0, (name, b)
            assert np.all(mag[b, :F] >= np.float32(1e-10) ** np.float32(lv['power']) * 0.99)


@pytest.mark.parametrize('name', ['A', 'B'])
def test_host_hook_whole_runs_converge_like_float64(name):
    """c(k) does not increase, and float32 after 2 k iterations is at least as converged as float64 after k"""
    from wavenet_vocoder import _ext
    geo = R.GEOMETRIES[name]
    F = 40
    S, u, _ = _case('tones', [F], geo, 21, pad=0)
    cfg = _ext.griffin_config(*geo)
    ks = (1, 2, 4, 8, 16, 32)
    c32 = {k: R.convergence(_ext.griffin_host(cfg, S, [F], u=u, iters=k)[0], S[0], F, geo) for k in ks}
    y64, c64, done = R.start(S[0], u[0], F, geo), {}, 0
    for k in ks[:-1]:
        y64 = R.iterate(y64, S[0].astype(np.float64), F, geo, k - done); done = k
        c64[k] = R.convergence(y64, S[0], F, geo)
    print(name, ['%.4f' % c32[k] for k in ks], ['%.4f' % c64[k] for k in ks[:-1]])
    for a, c in zip(ks[:-1], ks[1:]):
        assert c32[c] <= c32[a] and c32[c] <= c64[a]
    # run(a) followed by b more iterations from its y equals run(a + b): the host's continuation is a start from y0
    ya = _ext.griffin_host(cfg, S, [F], u=u, iters=3)
    assert np.array_equal(_ext.griffin_host(cfg, S, [F], y0=ya, iters=4), _ext.griffin_host(cfg, S, [F], u=u, iters=7))


# ---- five seeded faults, each caught by the staged rule
@pytest.mark.parametrize('fault', R.FAULTS)
def test_seeded_fault_is_caught_by_the_staged_rule(fault):
    caught = []
    for name in ('A', 'B'):      # win_size < n_fft: the window's offset matters
        geo = R.GEOMETRIES[name]
        F = 33
        S, x = R.target('noise', F, 3, geo)
        y0 = R.signal('noise', len(x), 4, geo[0])
        if fault == 'magnitude_before_power':
            lv, basis = R.mel_level('clip_sym'), R.mel_basis(12, geo[0])
            pinv, mel = R.pinv_of(basis), R.normalised_mel(S, basis, R.mel_level('clip_sym'))
            w = R.check_magnitudes(R.magnitudes(mel, pinv, lv, np.float32, fault=fault), mel, pinv, lv)[0]
        elif fault == 'window_not_centred':
            w = R.check_spectrum(R.standin_spectrum(y0, F, geo, fault=fault), y0, F, geo)[0]
        else:
            X = R.standin_spectrum(y0, F, geo)
            w = R.check_output(R.standin_output(X, S, F, geo, fault=fault), X, S, F, geo)[0]
        caught.append(w > 1.0)
    assert all(caught), fault


def test_the_rule_passes_the_unfaulted_stand_in():
    geo = R.GEOMETRIES['A']
    F = 33
    S, x = R.target('tones', F, 3, geo)
    y0 = R.signal('noise', len(x), 4, geo[0])
    X = R.standin_spectrum(y0, F, geo)
    assert R.check_spectrum(X, y0, F, geo)[0] <= 1.0 / R.FACTOR + 1e-12 and R.check_output(R.standin_output(X, S, F, geo), X, S, F, geo)[0] <= 1.0 / R.FACTOR + 1e-12


# ---- the stand-alone host program
@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/griffin_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('griffin') / 'griffin_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'griffin_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    r = host_program
    assert r.returncode == 0 and 'griffin ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    wss = {tuple(int(v) for v in l.split()[1:4]): float(l.split()[4]) for l in r.stdout.splitlines() if l.startswith('wss ')}
    assert wss[(64, 48, 12)] == wss[(96, 80, 20)] == wss[(64, 64, 16)] == 1.25 and min(wss.values()) > 0


def test_every_validation_code_through_the_host_program(host_program):
    codes = {l.split()[1]: int(l.split()[2]) for l in host_program.stdout.splitlines() if l.startswith('code ')}
    want = {'cfg_null': WN_E_ARG, 'cfg_ok': 0, 'cfg_abi': WN_E_ARG, 'cfg_batch_neg': WN_E_ARG, 'cfg_geometry_only': 0, 'cfg_frames_neg': WN_E_ARG,
            'cfg_frames_one': WN_E_SHAPE, 'cfg_mels_neg': WN_E_ARG, 'cfg_mels_over': WN_E_ARG, 'cfg_mels_zero': 0, 'cfg_mp_zero': WN_E_ARG, 'cfg_mp_nan': WN_E_ARG,
            'cfg_power_neg': WN_E_ARG, 'cfg_power_inf': WN_E_ARG, 'cfg_level_zero': WN_E_ARG, 'cfg_level_zero_unnormalised': 0, 'cfg_fft_odd': WN_E_SHAPE,
            'cfg_fft_small': WN_E_SHAPE, 'cfg_win_over': WN_E_SHAPE, 'cfg_win_small': WN_E_SHAPE, 'cfg_hop_zero': WN_E_SHAPE, 'cfg_hop_over': WN_E_SHAPE,
            'cfg_hop_quarter': 0, 'cfg_fft_not_32': WN_E_UNSUPPORTED, 'cfg_fft_large': WN_E_UNSUPPORTED, 'cfg_4096_1024': 0, 'cfg_hop_256': 0,
            'run_ok': 0, 'run_src_null': WN_E_ARG, 'run_frames_null': WN_E_ARG, 'run_kind_bad': WN_E_ARG, 'run_mel_without_pinv': WN_E_ARG,
            'run_magnitude_without_pinv': 0, 'run_b_zero': WN_E_ARG, 'run_iters_negative': WN_E_ARG, 'run_iters_zero': 0, 'run_pitch_negative': WN_E_ARG,
            'run_b_over': WN_E_SHAPE, 'run_one_frame': WN_E_SHAPE, 'run_frames_over_fmax': WN_E_SHAPE, 'run_frames_over_max': WN_E_SHAPE,
            'run_out_pitch_short': WN_E_SHAPE, 'run_y0_pitch_short': WN_E_SHAPE, 'run_out_null': 0}
    assert codes == want


# ---- datasets.audio: the numpy inversion
def _tone_hp(**over):
    import mel_util as MU
    kw = dict(griffin_lim_iters=30)
    kw.update(over)
    return MU.mel_hparams(**kw)


def test_numpy_inversion_of_a_steady_tone_keeps_its_pitch():
    from datasets import audio
    hp = _tone_hp()
    sr, hop = hp.sample_rate, audio.get_hop_size(hp)
    F = 30
    t = np.arange(hop * (F - 1))
    for freq in (220.0, 440.0):
        x = 0.5 * np.sin(2 * np.pi * freq * t / sr)
        mel = audio.melspectrogram(x, hp)
        y = audio.inv_mel_spectrogram(mel, hp, rng=np.random.default_rng(1))
        assert y.shape == (hop * (F - 1),) and np.all(np.isfinite(y))
        lo, hi = R.mel_band(hp, freq)
        peak = R.spectral_peak(y, sr)
        assert lo <= peak <= hi, (freq, peak, lo, hi)
        again = audio.inv_mel_spectrogram(mel, hp, rng=np.random.default_rng(1))
        assert np.array_equal(y, again)                                   # the start is seeded through rng
    raw = audio.inv_mel_spectrogram_host([mel], hp, seed=1, deemphasize=False)[0]
    assert np.allclose(audio.inv_preemphasis(raw.astype(np.float64), hp.preemphasis), audio.inv_mel_spectrogram_host([mel], hp, seed=1)[0], atol=1e-4)


def test_numpy_inversion_matches_the_reference_module_and_refuses_lws():
    from datasets import audio
    hp = _tone_hp(n_fft=96, win_size=80, hop_size=20, num_mels=12, sample_rate=8000, fmin=50, fmax=3800, griffin_lim_iters=4)
    geo = R.GEOMETRIES['B']
    F = 20
    S, x = R.target('tones', F, 2, geo)
    X = R.stft(x, F, geo)
    assert np.max(np.abs(audio._istft(X.T, hp) - x)) < 1e-12                 # librosa's istft restated twice, independently
    mel = audio.melspectrogram(x.astype(np.float64), hp)
    mag = audio.mel_to_magnitude(mel, hp)
    lv = R.mel_level('clip_sym', magnitude_power=hp.magnitude_power, power=hp.power, min_level_db=hp.min_level_db, ref_level_db=hp.ref_level_db, max_abs_value=hp.max_abs_value)
    pinv64 = np.linalg.pinv(audio._build_mel_basis(hp).astype(np.float64))
    ref = R.magnitudes(mel.T, pinv64.astype(np.float32), lv)                 # (the float32 rounding of mel and pinv: 1e-6 relative)
    assert np.max(np.abs(mag.T - ref)) <= 2e-5 * np.max(ref)
    rng = np.random.default_rng(3)
    u = np.random.default_rng(3).random(mag.shape)
    y = audio._griffin_lim(mag, hp, rng)
    y_ref = R.iterate(R.start(mag.T, u.T, F, geo), mag.T, F, geo, 4)
    assert np.max(np.abs(y - y_ref)) < 1e-9 * max(1.0, np.max(np.abs(y_ref)))
    hp.use_lws = True
    for call in (lambda: audio.inv_mel_spectrogram(mel, hp), lambda: audio.inv_mel_spectrogram_host([mel], hp), lambda: audio.inv_mel_spectrogram_device([mel], None, hp)):
        with pytest.raises(NotImplementedError):
            call()


# ---- the Python plumbing: hparams, the Synthesizer's baseline on stand-ins, the command line
def test_hparams_keys_keep_todays_behaviour_by_default():
    import hparams as H
    hp = H._build()
    assert hp.mi355_griffin_lim_baseline is False and hp.power == 1.5 and hp.griffin_lim_iters == 60 and hp.GL_on_GPU is True
    hp.parse('mi355_griffin_lim_baseline=True,griffin_lim_iters=5')
    assert hp.mi355_griffin_lim_baseline is True and hp.griffin_lim_iters == 5


class _Griffin(object):
    """stand-in for _ext.GriffinLim: records its calls, returns silence"""
    made = []

    def __init__(self, rows, max_frames, hop):
        self.rows, self.max_frames, self.hop, self.calls = rows, max_frames, hop, []
        _Griffin.made.append(self)

    def run_mel(self, mel, frames, iters=60, channels_first=False, seed=0, **kw):
        self.calls.append((tuple(mel.shape), list(frames), iters, channels_first, seed))
        return torch.full((len(frames), self.hop * (max(frames) - 1)), 0.25)

    def close(self):
        pass


class _Recon(object):
    def __init__(self, rows, max_samples):
        self.rows, self.max_samples, self.calls = rows, max_samples, []

    def score(self, wav, lengths, c, frames=None, c_channels_first=True):
        self.calls.append((tuple(wav.shape), list(lengths), tuple(c.shape), list(frames), c_channels_first))
        t = np.zeros((len(lengths), 9), np.float32); t[:, 4] = 2.5
        return t

    def close(self):
        pass


class _Pitch(_Recon):
    def score(self, generated, reference, lengths):
        self.calls.append((tuple(generated.shape), tuple(reference.shape), list(lengths)))
        t = np.zeros((len(lengths), 9), np.float32); t[:, 4] = 0.125
        return t


class _Model(object):
    device = torch.device('cpu')

    def __init__(self, hop):
        self.hop, self.made = hop, []

    def griffin_lim(self, rows, max_frames):
        self.made.append(('griffin', rows, max_frames))
        return _Griffin(rows, max_frames, self.hop)

    def reconstruction_check(self, rows, max_samples):
        self.made.append(('recon', rows, max_samples))
        return _Recon(rows, max_samples)

    def pitch_check(self, rows, max_samples):
        self.made.append(('pitch', rows, max_samples))
        return _Pitch(rows, max_samples)


def _synth(monkeypatch, **over):
    import mel_util as MU
    from datasets import audio
    from wavenet_vocoder.synthesizer import Synthesizer
    hp = MU.mel_hparams(n_fft=96, win_size=80, hop_size=20, num_mels=12, cin_channels=12, sample_rate=8000, fmin=50, fmax=3800, griffin_lim_iters=3, **over)
    s = Synthesizer(); s._hparams = hp; s.model = _Model(20); s._recon = None
    # the device batch path with the stand-in handle: OutputStage is not needed (deemphasize=False) and .cuda() is the identity here
    monkeypatch.setattr(torch.Tensor, 'cuda', lambda self, *a, **k: self, raising=False)
    return s, hp, audio


def _written(path):
    return sorted(os.listdir(path))


def test_baseline_off_creates_no_handle_and_writes_nothing(tmp_path, monkeypatch):
    s, hp, _ = _synth(monkeypatch, mi355_reconstruction_check=True, mi355_pitch_check=True)
    mels = [np.zeros((10, 12), np.float32), np.zeros((6, 12), np.float32)]
    wavs = [np.zeros(200, np.float32), np.zeros(120, np.float32)]
    out = str(tmp_path)
    before = s._write(wavs, [np.zeros((12, 0))] * 2, mels, ['a', 'b'], out, None)
    assert _written(out) == ['wavenet-audio-a.wav', 'wavenet-audio-b.wav'] and s.model.made == [] and not hasattr(s, '_griffin')
    blobs = [open(p, 'rb').read() for p in before]
    hp.mi355_griffin_lim_baseline = True; hp.mi355_reconstruction_check = False; hp.mi355_pitch_check = False
    out2 = str(tmp_path / 'on'); os.makedirs(out2)
    after = s._write(wavs, [np.zeros((12, 0))] * 2, mels, ['a', 'b'], out2, None)
    assert [open(p, 'rb').read() for p in after] == blobs              # the generated wavs are byte-identical with the baseline on
    assert _written(out2) == ['griffin-lim-a.wav', 'griffin-lim-b.wav', 'wavenet-audio-a.wav', 'wavenet-audio-b.wav']
    assert s.model.made == [('griffin', 2, 10)]                        # no check handle: the checks are off


def test_baseline_on_writes_the_wavs_and_the_two_new_tsv_files(tmp_path, monkeypatch):
    from scipy.io import wavfile
    from wavenet_vocoder import pitch as P, reconstruction as RC
    s, hp, _ = _synth(monkeypatch, mi355_griffin_lim_baseline=True, mi355_reconstruction_check=True, mi355_pitch_check=True)
    out = str(tmp_path)
    mels = [np.zeros((10, 12), np.float32), np.zeros((1, 12), np.float32), np.zeros((6, 12), np.float32)]      # the one-frame mel has no Griffin-Lim signal
    wavs = [np.zeros(200, np.float32), np.zeros(20, np.float32), np.zeros(120, np.float32)]
    cond = np.zeros((3, 10, 12), np.float32)
    s.pitch_references = [np.zeros(150, np.float32), np.zeros(20, np.float32), np.zeros(500, np.float32)]
    s._reconstruction(None, wavs, cond, [10, 1, 6], list('abc'), out)
    s._pitch(None, wavs, list('abc'), out)
    model_files = {n: open(os.path.join(out, n), 'rb').read() for n in ('reconstruction.tsv', 'pitch.tsv')}
    s._write(wavs, [np.zeros((12, 0))] * 3, mels, list('abc'), out, None)
    assert _written(out) == ['griffin-lim-a.wav', 'griffin-lim-c.wav', 'pitch.tsv', 'pitch_griffin_lim.tsv', 'reconstruction.tsv', 'reconstruction_griffin_lim.tsv',
                             'wavenet-audio-a.wav', 'wavenet-audio-b.wav', 'wavenet-audio-c.wav']
    assert {n: open(os.path.join(out, n), 'rb').read() for n in model_files} == model_files                  # the existing files stay untouched
    rate, w = wavfile.read(os.path.join(out, 'griffin-lim-a.wav'))
    assert rate == 8000 and w.dtype == np.int16 and len(w) == 20 * 9
    g = _Griffin.made[-1]
    assert g.calls == [((2, 12, 10), [6, 10], 3, True, hp.wavenet_random_seed)]                               # one ragged batch, shortest first, channels first
    # the SAME check handles as the model's scores (made once each), fed the signal before the de-emphasis and hop (F - 1) samples per row
    assert [m[0] for m in s.model.made] == ['recon', 'pitch', 'griffin']
    assert s._recon.calls[-1] == ((2, 180), [180, 100], (2, 10, 12), [10, 6], False)
    assert s._pitch_chk.calls[-1] == ((2, 180), (2, 150), [150, 100])
    rows = RC.read_tsv(os.path.join(out, 'reconstruction_griffin_lim.tsv'))
    assert [r['name'] for r in rows] == ['a', 'c'] and [int(r['frames']) for r in rows] == [10, 6] and rows[0]['l1c_db'] == '2.5000'
    assert [r['name'] for r in P.read_tsv(os.path.join(out, 'pitch_griffin_lim.tsv'))] == ['a', 'c']
    # a second call without recordings: the pitch file does not grow, the reconstruction file does
    s._write(wavs[:1], [np.zeros((12, 0))], mels[:1], ['d'], out, None)
    assert len(RC.read_tsv(os.path.join(out, 'reconstruction_griffin_lim.tsv'))) == 3 and len(P.read_tsv(os.path.join(out, 'pitch_griffin_lim.tsv'))) == 2


def test_baseline_on_the_host_path_needs_no_handle(tmp_path, monkeypatch):
    s, hp, _ = _synth(monkeypatch, mi355_griffin_lim_baseline=True, GL_on_GPU=False)
    t = np.arange(20 * 11)
    from datasets import audio
    mel = audio.melspectrogram(0.5 * np.sin(2 * np.pi * 440.0 * t / 8000), hp).T.astype(np.float32)
    s._write([np.zeros(240, np.float32)], [np.zeros((12, 0))], [mel], ['tone'], str(tmp_path), None)
    assert s.model.made == [] and _written(str(tmp_path)) == ['griffin-lim-tone.wav', 'wavenet-audio-tone.wav']


def test_command_line_host_path_end_to_end(tmp_path):
    """--host on a synthetic mel folder, once through --mels and once through --map: one wav per mel, hop (frames - 1) samples, the tone's pitch kept"""
    from scipy.io import wavfile
    import mel_util as MU
    from datasets import audio
    hp = MU.mel_hparams()
    sr, hop = hp.sample_rate, audio.get_hop_size(hp)
    data = tmp_path / 'training_data'
    (data / 'mels').mkdir(parents=True)
    frames = {'low': 7, 'tone': 12}      # (sorted: --mels walks the folder in this order too, and mel b starts from seed + b)
    with open(data / 'map.txt', 'w') as f:
        for name, F in frames.items():
            t = np.arange(hop * (F - 1))
            mel = audio.melspectrogram(0.5 * np.sin(2 * np.pi * (440.0 if name == 'tone' else 220.0) * t / sr), hp).T.astype(np.float32)
            np.save(data / 'mels' / ('mel-%s.npy' % name), mel)
            f.write('|'.join(['audio-%s.npy' % name, 'mel-%s.npy' % name, 'mel-%s.npy' % name, '<no_g>', str(len(t)), str(F)]) + '\n')
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'tacotron-2_amd'), os.environ.get('PYTHONPATH', '')]))
    for src, out in ((['--mels', str(data / 'mels')], tmp_path / 'a'), (['--map', str(data / 'map.txt')], tmp_path / 'b')):
        r = subprocess.run([sys.executable, '-m', 'wavenet_vocoder.griffin_lim'] + src + ['--output_dir', str(out), '--iters', '8', '--seed', '3', '--host'],
                           capture_output=True, text=True, timeout=300, env=env, cwd=os.path.join(ROOT, 'tacotron-2_amd'))
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        assert 'numpy' in r.stdout and sorted(os.listdir(out)) == ['griffin-lim-low.wav', 'griffin-lim-tone.wav']
        for name, F in frames.items():
            rate, w = wavfile.read(out / ('griffin-lim-%s.wav' % name))
            assert rate == sr and len(w) == hop * (F - 1)
        lo, hi = R.mel_band(hp, 440.0)
        rate, w = wavfile.read(out / 'griffin-lim-tone.wav')
        assert lo <= R.spectral_peak(w.astype(np.float64), sr) <= hi
    assert open(tmp_path / 'a' / 'griffin-lim-tone.wav', 'rb').read() == open(tmp_path / 'b' / 'griffin-lim-tone.wav', 'rb').read()      # one seed, one result
