"""Pitch check, host side (no GPU): the C ABI names, the validation of a configuration and of a call, the float64 reference of tests/pitch_ref.py against
a brute-force loop and the energy / autocorrelation identity, the estimator evaluated on the host through wn_test_pitch_host (the very functions the
kernels inline, csrc/wn_pitch.h) against that reference under exactly the assertions of tests/test_hip_pitch.py, steady tones, noise and silence at the
production geometry, the semantics of the comparison, the host functions under ASAN + UBSAN in a stand-alone program, and the Python surface (hparams,
PitchCheck, the Synthesizer's plumbing, the TSV helpers, the command line in --host mode)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import pitch_ref as PR
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED = -1, -2, -4
P = PR.GEOMETRIES['P']


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    names = ('wn_pitch_create', 'wn_pitch_frame_tile', 'wn_pitch_run', 'wn_pitch_compare', 'wn_test_pitch_host', 'wn_test_pitch_compare_host')
    for name in names + ('wn_pitch_destroy', 'wn_pitch_last_error', 'wn_pitch_num_frames'):
        assert name in _ext.exported_symbols() and hasattr(lib, name), name
    for name in names:
        assert name in declared, name
    assert 'void wn_pitch_destroy(' in text and 'const char* wn_pitch_last_error(' in text and 'int64_t wn_pitch_num_frames(' in text
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert 'wn_test_pitch_host(' in hooks and 'wn_test_pitch_compare_host(' in hooks                 # the hooks alone are fenced
    assert 'wn_pitch_run(' not in hooks and 'wn_pitch_create(' not in hooks and 'wn_pitch_compare(' not in hooks
    assert ctypes.sizeof(_ext.WnPitchConfig) == 40


def _create(geo=P, rows=2, max_samples=4000, **kw):
    from wavenet_vocoder import _ext
    cfg = _ext.pitch_config(dict(geo), rows, max_samples)
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    lib = _ext.load_library()
    rc = lib.wn_pitch_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = (lib.wn_pitch_last_error(None) or b'').decode()
    if rc == 0:
        lib.wn_pitch_destroy(h)
    return rc, msg


def test_create_validates_before_any_device_call():
    """every configuration error is WN_E_ARG with a text that names the field, a tile beyond the LDS budget WN_E_UNSUPPORTED; a valid handle needs no device"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    assert lib.wn_pitch_create(None, ctypes.byref(h)) == WN_E_ARG and b'null argument' in lib.wn_pitch_last_error(None)
    assert lib.wn_pitch_create(ctypes.byref(_ext.pitch_config(dict(P), 1, 10)), None) == WN_E_ARG
    nan = float('nan')
    bad = [(dict(abi_version=5), 'abi_version'), (dict(sample_rate=0), 'sample_rate'), (dict(hop=0), 'hop'), (dict(hop=-3), 'hop'), (dict(window=0), 'window'),
           (dict(tau_min=1), 'tau_min'), (dict(tau_min=-2), 'tau_min'), (dict(tau_max=45), 'tau_max'), (dict(tau_max=44), 'tau_max'), (dict(tau_max=-1), 'tau_max'),
           (dict(threshold=0.0), 'threshold'), (dict(threshold=-0.1), 'threshold'), (dict(threshold=1.0001), 'threshold'), (dict(threshold=nan), 'threshold'),
           (dict(max_batch=0), 'max_batch'), (dict(max_batch=-1), 'max_batch'), (dict(max_samples=-1), 'max_samples')]
    for kw, field in bad:
        rc, msg = _create(**kw)
        assert rc == WN_E_ARG and msg.startswith('wn_pitch_create: ') and field in msg, (kw, rc, msg)
    for kw in (dict(window=16384), dict(hop=2048), dict(tau_max=1600)):
        rc, msg = _create(**kw)
        assert rc == WN_E_UNSUPPORTED and 'LDS' in msg, (kw, rc, msg)
    for kw in (dict(), dict(threshold=1.0), dict(tau_min=2), dict(tau_max=46), dict(max_samples=0), dict(max_batch=1)):
        assert _create(**kw)[0] == 0, kw
    for name in ('A', 'M'):
        assert _create(PR.GEOMETRIES[name])[0] == 0
    lib.wn_pitch_destroy(None)
    assert lib.wn_pitch_num_frames(None, 5) == WN_E_ARG and lib.wn_pitch_frame_tile(None) == WN_E_ARG


def test_every_validation_code_of_a_call_on_a_handle():
    """argument errors as WN_E_ARG first, then WN_E_SHAPE, each with its message; every one is refused before any device call, so this runs without a device"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.pitch_config(dict(P), 3, 4000)
    h = ctypes.c_void_p()
    assert lib.wn_pitch_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert lib.wn_pitch_frame_tile(h) == PR.TILE and lib.wn_pitch_num_frames(h, 4000) == 15 and lib.wn_pitch_num_frames(h, 0) == 1 and lib.wn_pitch_num_frames(h, -1) == WN_E_ARG
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    i3 = ctypes.c_int32 * 3
    n, neg, lng, four = i3(3000, 0, 4000), i3(3000, -1, 4000), i3(3000, 0, 4001), (ctypes.c_int32 * 4)(1, 1, 1, 1)
    run, err = lib.wn_pitch_run, lambda: lib.wn_pitch_last_error(h)
    assert run(None, p, 4000, n, 3, 15, p, p, p, None) == WN_E_ARG
    for args in ((None, 4000, n, 3, 15, p), (p, 4000, None, 3, 15, p), (p, 4000, n, 3, 15, None)):
        assert run(h, *args, None, None, None) == WN_E_ARG and b'null argument' in err()
    assert run(h, p, 4000, n, 0, 15, p, None, None, None) == WN_E_ARG and b'B (0)' in err()
    assert run(h, p, 4000, n, 3, -1, p, None, None, None) == WN_E_ARG and b'F_max' in err()
    assert run(h, p, -1, n, 3, 15, p, None, None, None) == WN_E_ARG and b'ld' in err()
    assert run(h, p, 4000, neg, 3, 15, p, None, None, None) == WN_E_ARG and b'lengths[1]' in err()
    assert run(h, p, 4000, four, 4, 15, p, None, None, None) == WN_E_SHAPE and b'max_batch = 3' in err()
    assert run(h, p, 4000, n, 3, 16, p, None, None, None) == WN_E_SHAPE and b'F_max (16)' in err()
    assert run(h, p, 4000, n, 3, 14, p, None, None, None) == WN_E_SHAPE and b'F_max (14)' in err() and b'lengths[2]' in err()
    assert run(h, p, 3999, n, 3, 15, p, None, None, None) == WN_E_SHAPE and b'ld = 3999' in err()
    assert run(h, p, 4100, lng, 3, 15, p, None, None, None) == WN_E_SHAPE and b'max_samples = 4000' in err()
    cmp = lib.wn_pitch_compare
    fr, frneg, frlng = i3(15, 0, 7), i3(15, -1, 7), i3(16, 0, 7)
    assert cmp(None, p, p, 15, fr, 3, p, None) == WN_E_ARG
    for args in ((None, p, 15, fr, 3, p), (p, None, 15, fr, 3, p), (p, p, 15, None, 3, p), (p, p, 15, fr, 3, None)):
        assert cmp(h, *args, None) == WN_E_ARG and b'null argument' in err()
    assert cmp(h, p, p, 15, fr, 0, p, None) == WN_E_ARG and b'B (0)' in err()
    assert cmp(h, p, p, -1, fr, 3, p, None) == WN_E_ARG and b'pitch' in err()
    assert cmp(h, p, p, 15, frneg, 3, p, None) == WN_E_ARG and b'frames[1]' in err()
    assert cmp(h, p, p, 15, four, 4, p, None) == WN_E_SHAPE and b'max_batch = 3' in err()
    assert cmp(h, p, p, 14, fr, 3, p, None) == WN_E_SHAPE and b'pitch = 14' in err()
    assert cmp(h, p, p, 16, frlng, 3, p, None) == WN_E_SHAPE and b'frames[0] = 16' in err()
    lib.wn_pitch_destroy(h)
    # the hooks validate the same configuration and call
    x = np.zeros((1, 300), np.float32)
    with pytest.raises(_ext.WnError) as ei:
        _ext.pitch_host(dict(P, tau_min=1), x, [300])
    assert ei.value.code == WN_E_ARG and 'wn_test_pitch_host: tau_min' in str(ei.value)
    with pytest.raises(_ext.WnError) as ei:
        _ext.pitch_host(dict(P), x, [300], frames=1)
    assert ei.value.code == WN_E_SHAPE
    with pytest.raises(_ext.WnError) as ei:
        _ext.pitch_host(dict(P), x, [-1])
    assert ei.value.code == WN_E_ARG
    with pytest.raises(_ext.WnError) as ei:
        _ext.pitch_compare_host(np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), [4])
    assert ei.value.code == WN_E_SHAPE
    with pytest.raises(ValueError):
        _ext.pitch_config(dict(P, fmin=60.0), 1, 10)


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/pitch_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('pitch') / 'pitch_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'pitch_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """the estimator over the three geometries x n in {0, 1, hop - 1, hop, L - 1, L, 3 L + 1} x {tone, noise, silence} in heap blocks of exactly the row's
    size, with and without the optional outputs, and the comparison; the program checks silence, d'(0) and the comparison's counts itself"""
    r = host_program
    assert r.returncode == 0 and 'pitch ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = dict(l.split()[1:] for l in host_program.stdout.splitlines() if l.startswith('code '))
    got = {k: int(v) for k, v in got.items()}
    A, S, N = WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED
    want = dict(cfg_null=A, cfg_ok=0, cfg_abi=A, cfg_rate_zero=A, cfg_hop_zero=A, cfg_window_zero=A, cfg_tau_min_one=A, cfg_tau_min_two=0, cfg_tau_max_tight=A,
                cfg_tau_max_least=0, cfg_threshold_zero=A, cfg_threshold_one=0, cfg_threshold_over=A, cfg_threshold_nan=A, cfg_batch_zero=A, cfg_samples_neg=A,
                cfg_samples_zero=0, cfg_lds_window=N, cfg_lds_hop=N, cfg_lds_tau=N,
                run_ok=0, run_wav_null=A, run_lengths_null=A, run_f0_null=A, run_b_zero=A, run_f_negative=A, run_length_negative=A, run_b_over=S, run_f_over=S,
                run_f_short=S, run_ld_short=S, run_length_over=S,
                cmp_ok=0, cmp_a_null=A, cmp_b_null=A, cmp_frames_null=A, cmp_table_null=A, cmp_b_zero=A, cmp_frames_negative=A, cmp_b_over=S, cmp_pitch_short=S,
                cmp_frames_over=S)
    assert got == want


# ---- the reference against itself
@pytest.mark.parametrize('name,n', [('A', 333), ('M', 500)])
def test_reference_against_a_brute_force_loop_and_the_autocorrelation_identity(name, n):
    geo = PR.GEOMETRIES[name]
    x = PR.signal(geo, n, 7)
    ref = PR.dprime(x, geo)
    assert ref.shape == (1 + n // geo['hop'], geo['tau_max'] + 1)
    assert np.abs(ref - PR.dprime_brute(x, geo)).max() <= 1e-9
    assert np.abs(ref - PR.dprime_autocorr(x, geo)).max() <= 1e-9


def test_reference_identity_at_the_production_geometry():
    x = PR.signal(P, 3000, 8)
    assert np.abs(PR.dprime(x, P) - PR.dprime_autocorr(x, P)).max() <= 1e-9


# ---- the host hook against the reference: exactly the assertions of the GPU file
@pytest.mark.parametrize('name', ['A', 'P', 'M'])
def test_hook_against_float64_under_the_device_assertions(name):
    """every d' within beta |ref|; on decidable frames tau*, the voiced flag and f0 inside its tolerance; at most 1 % of the frames excused -- and a plain
    float32 numpy evaluation (the yardstick) under the same assertions with the same picks.  NaN beyond every row's length changes nothing and cells
    beyond a row's frames keep their fill."""
    from wavenet_vocoder import _ext
    geo, lengths, rows, refs = PR.case(name)
    wav = PR.batch(rows, ld=max(lengths) + 13)
    h = _ext.pitch_host(geo, wav, lengths, return_dprime=True, fill=-7.25)
    worst, frames, excused = PR.check_case(name, h['dprime'], h['f0'], h['ap'], 'hook')
    for b, n in enumerate(lengths):
        F = PR.num_frames(n, geo)
        assert np.all(h['f0'][b, F:] == -7.25) and np.all(h['ap'][b, F:] == -7.25) and np.all(h['dprime'][b, F:] == -7.25)
        assert np.all(np.isfinite(h['f0'][b, :F])) and np.all(np.isfinite(h['dprime'][b, :F]))
    yard_worst, disagree = 0.0, 0
    for b, x in enumerate(rows):
        y = PR.dprime(x, geo, np.float32)
        f0 = np.zeros(len(y)); ap = np.zeros(len(y))
        for f in range(len(y)):
            p = PR.pick(y[f].astype(np.float64), geo)
            f0[f], ap[f] = p['f0'], p['ap']
            disagree += refs[b][1][f]['decidable'] and (p['voiced'] != refs[b][1][f]['voiced'] or p['tau'] != refs[b][1][f]['tau'])
        yard_worst = max(yard_worst, PR.check_row(geo, refs[b][0], refs[b][1], y, f0, ap, ('yardstick', name, b))[0])
    print('geometry %s: %d frames, %d excused; worst d\' error / beta: hook %.3f, numpy float32 %.3f; float32 picks that disagree on a decidable frame: %d'
          % (name, frames, excused, worst, yard_worst, disagree))
    assert disagree == 0
    voiced = sum(p['voiced'] for _, picks in refs for p in picks)
    assert 0.15 * frames < voiced < 0.85 * frames                                                      # the signals exercise both outcomes


def test_hook_bit_identity_across_batch_position_and_pitch():
    from wavenet_vocoder import _ext
    geo, lengths, rows, _ = PR.case('A')
    base = _ext.pitch_host(geo, PR.batch(rows), lengths, return_dprime=True)
    order = [11, 3, 7, 0, 9]
    got = _ext.pitch_host(geo, PR.batch(rows, ld=4099, order=order), [lengths[i] for i in order], return_dprime=True)
    for b, i in enumerate(order):
        F = PR.num_frames(lengths[i], geo)
        for k in ('f0', 'ap', 'dprime'):
            assert np.array_equal(PR.bits(got[k][b, :F]), PR.bits(base[k][i, :F])), (k, i)
    alone = _ext.pitch_host(geo, rows[10][None], [lengths[10]])
    F = PR.num_frames(lengths[10], geo)
    assert np.array_equal(PR.bits(alone['f0'][0, :F]), PR.bits(base['f0'][10, :F])) and 'dprime' not in alone


def test_the_walk_stops_at_an_exact_tie():
    from wavenet_vocoder import _ext
    h = _ext.pitch_host(PR.TIE_GEO, PR.TIE_SIGNAL[None], [len(PR.TIE_SIGNAL)], return_dprime=True)
    PR.check_tie(h['f0'][0], h['dprime'][0], 'hook')


# ---- what the estimator says about known signals (the production geometry)
@pytest.mark.parametrize('f0', [70, 110, 196.3, 233.1, 330, 440])
def test_steady_three_harmonic_tones(f0):
    """interior frames are voiced and f0 is within 1e-3 relative of the truth; the float64 reference reaches 2.3e-4"""
    from wavenet_vocoder import _ext
    x = PR.tone(P, 22050 // 2, float(f0))
    h = _ext.pitch_host(P, x[None], [len(x)])
    _, picks = PR.track(x, P)
    F = len(picks)
    inner = slice(4, F - 4)                                                                            # frames whose span lies inside the signal
    assert all(p['voiced'] for p in picks[inner]) and np.all(h['f0'][0, inner] > 0)
    ref_err = max(abs(p['f0'] / f0 - 1.0) for p in picks[inner])
    hook_err = float(np.abs(h['f0'][0, inner].astype(np.float64) / f0 - 1.0).max())
    print('tone %.1f Hz: worst relative f0 error of the reference %.2e, of the hook %.2e' % (f0, ref_err, hook_err))
    assert ref_err <= 2.3e-4 and hook_err <= 1e-3


def test_white_noise_is_unvoiced_and_silence_has_ap_one():
    from wavenet_vocoder import _ext
    x = (0.2 * np.random.RandomState(42).randn(22050 // 2)).astype(np.float32)
    h = _ext.pitch_host(P, x[None], [len(x)])
    F = h['f0'].shape[1]
    assert np.all(h['f0'][0, 4:F - 4] == 0.0) and np.all(h['ap'][0, 4:F - 4] > P['threshold'])
    z = _ext.pitch_host(P, np.zeros((1, 5000), np.float32), [5000], return_dprime=True)
    assert np.all(z['f0'] == 0.0) and np.all(z['ap'] == 1.0) and np.all(z['dprime'] == 1.0)
    e = _ext.pitch_host(P, np.zeros((1, 1), np.float32), [0])                                          # an empty row has its one frame, unvoiced
    assert e['f0'].shape == (1, 1) and e['f0'][0, 0] == 0.0 and e['ap'][0, 0] == 1.0


# ---- the comparison
def test_comparison_semantics():
    from wavenet_vocoder import _ext
    n = 22050 // 2
    a = _ext.pitch_host(P, PR.tone(P, n, 200.0)[None], [n])['f0']
    b = _ext.pitch_host(P, PR.tone(P, n, 200.0 * 2 ** (50 / 1200.0))[None], [n])['f0']
    F = a.shape[1]
    same = _ext.pitch_compare_host(a, a.copy(), [F])[0]
    nv = int((a[0] > 0).sum())
    assert same[0] == F and same[1] == same[2] == same[3] == nv > F - 8 and np.all(same[4:] == 0.0)   # identical tracks give zeros
    t = _ext.pitch_compare_host(a[:, 4:F - 4].copy(), b[:, 4:F - 4].copy(), [F - 8])[0]              # 50 cents apart: rmse and bias of 50 within 1
    assert t[3] == F - 8 and t[4] == 0.0 and t[5] == 0.0 and abs(t[6] - 50.0) < 1.0 and abs(t[7] - 50.0) < 1.0 and abs(t[8] - 50.0) < 1.0
    noise = _ext.pitch_host(P, (0.2 * np.random.RandomState(1).randn(1, n)).astype(np.float32), [n])['f0']
    noise[0, :4] = 0.0; noise[0, F - 4:] = 0.0                                                          # (edge frames, half zeros, may do anything)
    v = _ext.pitch_compare_host(a, noise, [F])[0]                                                      # voiced against noise: the error is the voiced share
    assert v[2] == 0 and v[3] == 0 and v[4] == np.float32(nv / F) and np.all(v[5:] == 0.0)
    # every kind of frame, against the float64 comparison; gross errors leave the fine RMSE; an empty row gives zeros
    fa = np.array([[100, 0, 200, 0, 100, 150, 220, 0], [0] * 8], np.float32)
    fb = np.array([[100, 120, 0, 0, 200, 151, 180, 0], [0] * 8], np.float32)
    got = _ext.pitch_compare_host(fa, fb, [7, 0])
    ref = PR.compare(fa, fb, [7, 0])
    assert np.all(np.abs(got - ref) <= 2 * np.spacing(np.abs(ref).astype(np.float32))) and np.all(got[1] == 0.0)
    assert got[0, 0] == 7 and got[0, 3] == 4 and got[0, 5] == 0.25 and abs(got[0, 8] - np.sqrt((0 + (1200 * np.log2(151 / 150)) ** 2 + (1200 * np.log2(180 / 220)) ** 2) / 3)) < 1e-3


# ---- hparams, PitchCheck, the Synthesizer's plumbing, the TSV, the command line
def test_hparams_keys_keep_todays_behaviour_by_default():
    import hparams as H
    from wavenet_vocoder import _ext
    hp = H._build()
    assert hp.mi355_pitch_check is False and hp.mi355_pitch_fmin == 60.0 and hp.mi355_pitch_fmax == 500.0 and hp.mi355_pitch_threshold == 0.15 and hp.mi355_pitch_window == 1024
    assert _ext.pitch_geometry(hp) == dict(P, threshold=0.15)                                          # 22 050 / 275 / 1024 / lags 44 ... 368
    hp.parse('mi355_pitch_check=True,mi355_pitch_fmin=80,mi355_pitch_fmax=400,mi355_pitch_threshold=0.1,mi355_pitch_window=512')
    assert hp.mi355_pitch_check is True
    assert _ext.pitch_geometry(hp) == dict(sample_rate=22050, hop=275, window=512, tau_min=55, tau_max=276, threshold=0.1)


class _Tracker(object):
    """stands in for _ext.PitchTracker: records the calls; the table's row b is b + j / 16"""
    def __init__(self, hop):
        self.hop, self.calls, self.closed = hop, [], False

    def run(self, wav, lengths, return_dprime=False):
        self.calls.append(('run', tuple(wav.shape), list(lengths)))
        F = max(1 + n // self.hop for n in lengths)
        return torch.full((wav.shape[0], F), float(len(self.calls))), torch.zeros(wav.shape[0], F)

    def compare(self, f0_a, f0_b, frames):
        self.calls.append(('compare', float(f0_a[0, 0]), float(f0_b[0, 0]), list(frames)))
        B = f0_a.shape[0]
        return torch.arange(B, dtype=torch.float32)[:, None] + torch.arange(9, dtype=torch.float32)[None, :] / 16

    def close(self):
        self.closed = True


HP16 = dict(cin_channels=16, num_mels=16, hop_size=16, upsample_scales=[4, 4])


def test_pitch_check_plumbing_and_tsv(tmp_path):
    from wavenet_vocoder import pitch as PT
    hp = make_hp(**HP16)
    chk = PT.PitchCheck(hp, 3, 200, tracker=_Tracker(16))
    assert chk.hop == 16 and chk.geometry['tau_max'] == 368
    table = chk.score(torch.zeros(2, 200), torch.zeros(2, 160), [160, 95])
    assert table.shape == (2, 9) and table.dtype == np.float32 and table[1, 4] == 1.25
    # the generated signal is tracked first, the recording second, and the comparison takes the recording's track as its reference
    assert chk.tracker.calls == [('run', (2, 200), [160, 95]), ('run', (2, 160), [160, 95]), ('compare', 2.0, 1.0, [11, 6])]
    chk.close()
    assert chk.tracker.closed
    path = str(tmp_path / 'pitch.tsv')
    PT.append_tsv(path, ['a', 'b'], table)
    PT.append_tsv(path, ['c'], table[:1])
    rows = PT.read_tsv(path)
    assert [r['name'] for r in rows] == ['a', 'b', 'c'] and rows[1]['vuv_error'] == '1.2500' and rows[1]['frames'] == '1' and rows[1]['f0_rmse_cents'] == '1.38'
    assert open(path).read().count('name\tframes') == 1
    assert 'worst b' in PT.log_line(['a', 'b'], table) and '2 utterance(s)' in PT.log_line(['a', 'b'], table)
    pre = 'Wavenet_eval_model/eval_stats/wavenet_eval_'
    assert PT.scalars(table[1]) == {pre + 'f0_rmse_cents': 1.375, pre + 'vuv_error': 1.25, pre + 'gpe': 1.3125}


def test_synthesizer_scores_only_with_the_key_on_and_recordings_at_hand(tmp_path):
    from wavenet_vocoder import pitch as PT
    from wavenet_vocoder.synthesizer import Synthesizer

    class _Model(object):
        device = torch.device('cpu')

        def __init__(self, hp):
            self.hp, self.made = hp, []

        def pitch_check(self, rows, max_samples):
            self.made.append((rows, max_samples))
            return PT.PitchCheck(self.hp, rows, max_samples, tracker=_Tracker(16))

    out = str(tmp_path)
    wavs = [np.zeros(160, np.float32), np.zeros(96, np.float32)]
    refs = [np.zeros(150, np.float32), np.zeros(100, np.float32)]
    s = Synthesizer(); s._hparams = make_hp(**HP16); s.model = _Model(s._hparams)
    s.pitch_references = list(refs)
    assert s._pitch(None, wavs, ['a', 'b'], out) is None and os.listdir(out) == [] and s.model.made == []      # the key is off: nothing happens
    s._hparams = make_hp(mi355_pitch_check=True, **HP16); s.model = _Model(s._hparams)
    assert s._pitch(None, wavs, ['a', 'b'], out) is None and os.listdir(out) == []                              # no recordings: nothing to compare with
    s.pitch_references = list(refs)
    t = s._pitch(None, wavs, ['a', 'b'], out)                                                                  # the host path: what is about to be written is uploaded
    assert t.shape == (2, 9) and s.model.made == [(2, 150)] and s.pitch_references is None
    assert s._pitch_chk.tracker.calls[0] == ('run', (2, 150), [150, 96]) and s._pitch_chk.tracker.calls[2][3] == [10, 7]
    s.pitch_references = [np.zeros(300, np.float32)]
    s._pitch(torch.zeros(1, 256), None, ['c'], out)                                                            # the device path; outgrown: a larger check replaces it
    assert s.model.made == [(2, 150), (2, 256)] and s._pitch_chk.tracker.calls[0] == ('run', (1, 256), [256])
    assert [r['name'] for r in PT.read_tsv(os.path.join(out, 'pitch.tsv'))] == ['a', 'b', 'c']
    s.pitch_references = [np.zeros(10, np.float32)] * 3                                                        # a failure logs one line and never fails the run
    assert s._pitch(None, wavs, ['a', 'b'], out) is None
    assert len(PT.read_tsv(os.path.join(out, 'pitch.tsv'))) == 3


def test_command_line_in_host_mode(tmp_path, capsys):
    """a pair whose generated wav is the recording scores zero; a tone 50 cents up scores 50 cents; a wav without a recording is skipped, and said so"""
    from scipy.io import wavfile
    from wavenet_vocoder import pitch as PT
    gen, ref = str(tmp_path / 'gen'), str(tmp_path / 'ref')
    os.makedirs(gen); os.makedirs(ref)
    geo = dict(P, sample_rate=8000, hop=100)
    n = 4000

    def pcm(f):
        return (PR.tone(geo, n, f) * 32767 / 0.6).astype(np.int16)

    wavfile.write(os.path.join(ref, 'u0.wav'), 8000, pcm(150.0)); wavfile.write(os.path.join(gen, 'wavenet-audio-u0.wav'), 8000, pcm(150.0))
    wavfile.write(os.path.join(ref, 'u1.wav'), 8000, pcm(150.0)); wavfile.write(os.path.join(gen, 'u1.wav'), 8000, pcm(150.0 * 2 ** (50 / 1200.0)))
    wavfile.write(os.path.join(gen, 'orphan.wav'), 8000, pcm(99.0))
    over = 'sample_rate=8000,hop_size=100,mi355_pitch_window=400'
    names, table = PT.main(['--generated', gen, '--reference', ref, '--host', '--hparams', over, '--tsv', str(tmp_path / 't.tsv')])
    text = capsys.readouterr().out.splitlines()
    assert names == ['u1', 'u0'] or names == ['u0', 'u1']
    t = dict(zip(names, table))
    assert 'skipped 1 generated wav file(s)' in text[0] and text[1].split('\t') == list(PT.TSV_HEADER) and text[-1].startswith('Pitch check: 2 utterance(s)')
    assert t['u0'][0] == 41 and t['u0'][3] > 30 and np.all(t['u0'][4:] == 0.0)
    assert t['u1'][4] == 0.0 and t['u1'][5] == 0.0 and abs(t['u1'][6] - 50.0) < 1.5 and abs(t['u1'][7] - 50.0) < 1.5
    assert sorted(r['name'] for r in PT.read_tsv(str(tmp_path / 't.tsv'))) == ['u0', 'u1']
