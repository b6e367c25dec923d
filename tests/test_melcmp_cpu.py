"""Reconstruction check, host side (no GPU): the C ABI names, the validation of a configuration and of a call, the check's arithmetic evaluated on the
host through wn_test_melcmp_host (the very functions the kernels inline, csrc/wn_melcmp.h) against the float64 reference of tests/melcmp_util.py on every
element inside the derived bound, its bit identity across layouts, pitches, batch composition and per_frame, the host functions under ASAN + UBSAN in a
stand-alone program, and the Python surface (hparams, ReconstructionCheck, the Synthesizer's plumbing, the TSV writer, the command line) against
stand-in stages."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import melcmp_util as MU
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
NAMES = ('wn_melcmp_create', 'wn_melcmp_run', 'wn_test_melcmp_host')
WN_E_ARG, WN_E_SHAPE, WN_E_HIP = -1, -2, -3
UNIT, ALARM = 12.5, 30.0
CASES = [(M, nc) for M in (1, 13, 80, 128) for nc in sorted({0, min(13, M - 1), M - 1})]
FRAMES = (0, 1, 63, 65, 300)


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    for name in NAMES + ('wn_melcmp_destroy', 'wn_melcmp_last_error'):
        assert name in _ext.exported_symbols() and hasattr(lib, name), name
    for name in NAMES:
        assert name in declared, name
    assert 'void wn_melcmp_destroy(' in text and 'const char* wn_melcmp_last_error(' in text
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert 'wn_test_melcmp_host(' in hooks and 'wn_melcmp_run(' not in hooks and 'wn_melcmp_create(' not in hooks      # the hook alone is fenced
    assert ctypes.sizeof(_ext.WnMelcmpConfig) == 28


def _create(**kw):
    from wavenet_vocoder import _ext
    cfg = _ext.melcmp_config(80, 13, UNIT, 3.0, kw.pop('max_batch', 0), kw.pop('max_frames', 8))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = _ext.load_library().wn_melcmp_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == 0:
        _ext.load_library().wn_melcmp_destroy(h)
    return rc


def test_create_validates_before_any_device_call():
    """every configuration error is WN_E_ARG with a text, on a machine without a device too; a validation-only handle (max_batch = 0) needs no device; a
    real one gets as far as the device (WN_E_HIP without one)"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    assert lib.wn_melcmp_create(None, ctypes.byref(h)) == WN_E_ARG
    assert lib.wn_melcmp_create(ctypes.byref(_ext.melcmp_config(80)), None) == WN_E_ARG
    nan, inf = float('nan'), float('inf')
    bad = [dict(abi_version=5), dict(num_mels=0), dict(num_mels=129), dict(num_mels=-1), dict(n_cep=-1), dict(n_cep=80), dict(num_mels=13, n_cep=13), dict(unit_db=0.0),
           dict(unit_db=-1.0), dict(unit_db=inf), dict(unit_db=nan), dict(alarm_db=-0.5), dict(alarm_db=inf), dict(alarm_db=nan), dict(max_batch=-1), dict(max_frames=-1)]
    for kw in bad:
        assert _create(**kw) == WN_E_ARG, kw
        assert (lib.wn_melcmp_last_error(None) or b'').startswith(b'wn_melcmp_create: '), kw
    for kw in (dict(), dict(num_mels=128, n_cep=127), dict(num_mels=1, n_cep=0), dict(alarm_db=0.0), dict(max_frames=0)):
        assert _create(**kw) == 0, kw                                                          # max_batch = 0: no device is touched
    assert _create(max_batch=2) == (0 if torch.cuda.is_available() else WN_E_HIP)
    lib.wn_melcmp_destroy(None)


def test_every_validation_code_of_a_call_through_a_validation_only_handle():
    """max_batch = 0: every run is refused -- argument errors as WN_E_ARG first, then WN_E_SHAPE for any B >= 1 -- and nothing touches a device"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    cfg = _ext.melcmp_config(80, 13, UNIT, 3.0, 0, 8)
    h = ctypes.c_void_p()
    assert lib.wn_melcmp_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    n, neg = (ctypes.c_int32 * 2)(3, 0), (ctypes.c_int32 * 2)(3, -1)
    run = lib.wn_melcmp_run
    assert run(None, p, 1, 8, p, 1, 8, n, 2, p, 8, p, p, None) == WN_E_ARG
    assert run(h, None, 1, 8, p, 1, 8, n, 2, p, 8, p, p, None) == WN_E_ARG
    assert run(h, p, 1, 8, None, 1, 8, n, 2, p, 8, p, p, None) == WN_E_ARG
    assert run(h, p, 1, 8, p, 1, 8, None, 2, p, 8, p, p, None) == WN_E_ARG
    assert run(h, p, 1, 8, p, 1, 8, n, 2, p, 8, None, p, None) == WN_E_ARG
    assert run(h, p, 1, 8, p, 1, 8, n, 2, p, 8, p, None, None) == WN_E_ARG
    assert run(h, p, 1, 8, p, 1, 8, n, 0, p, 8, p, p, None) == WN_E_ARG
    assert b'B (0)' in lib.wn_melcmp_last_error(h)
    assert run(h, p, 1, 8, p, 1, 8, neg, 2, p, 8, p, p, None) == WN_E_ARG
    assert b'frames[1]' in lib.wn_melcmp_last_error(h)
    assert run(h, p, 1, 8, p, 1, 8, n, 2, p, 8, p, p, None) == WN_E_SHAPE
    assert b'max_batch = 0' in lib.wn_melcmp_last_error(h)
    assert run(h, p, 1, 8, p, 1, 8, n, 1, None, 0, p, p, None) == WN_E_SHAPE
    lib.wn_melcmp_destroy(h)
    # the hook validates the same configuration and call (its own limits: max_batch / max_frames 0 = none)
    with pytest.raises(_ext.WnError) as ei:
        _ext.melcmp_host(np.zeros((1, 80, 4), np.float32), np.zeros((1, 80, 4), np.float32), [4], n_cep=80)
    assert ei.value.code == WN_E_ARG
    with pytest.raises(_ext.WnError) as ei:
        _ext.melcmp_host(np.zeros((1, 80, 4), np.float32), np.zeros((1, 80, 4), np.float32), [5])
    assert ei.value.code == WN_E_SHAPE
    with pytest.raises(_ext.WnError) as ei:
        _ext.melcmp_host(np.zeros((1, 80, 4), np.float32), np.zeros((1, 80, 4), np.float32), [4], out_pitch=3)
    assert ei.value.code == WN_E_SHAPE
    with pytest.raises(_ext.WnError) as ei:
        _ext.melcmp_host(np.zeros((1, 80, 4), np.float32), np.zeros((1, 80, 4), np.float32), [-1])
    assert ei.value.code == WN_E_ARG


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/melcmp_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('melcmp') / 'melcmp_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'melcmp_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """the per-frame code, the reductions and the table over M in {1, 13, 80, 128} x n_cep in {0, 1, 13, M - 1} x frames in {0, 1, 63, 64, 65, 129} x the four
    layout pairs in heap blocks of exactly the needed size; the program checks the layouts' bit identity, the marks and the exact zero of equal inputs itself"""
    r = host_program
    assert r.returncode == 0 and 'melcmp ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_through_the_host_program(host_program):
    got = dict(l.split()[1:] for l in host_program.stdout.splitlines() if l.startswith('code '))
    got = {k: int(v) for k, v in got.items()}
    A, S = WN_E_ARG, WN_E_SHAPE
    want = dict(cfg_null=A, cfg_ok=0, cfg_abi=A, cfg_mels_zero=A, cfg_mels_over=A, cfg_mels_top=0, cfg_cep_neg=A, cfg_cep_over=A, cfg_cep_top=0, cfg_cep_zero=0,
                cfg_unit_zero=A, cfg_unit_neg=A, cfg_unit_inf=A, cfg_unit_nan=A, cfg_alarm_neg=A, cfg_alarm_inf=A, cfg_alarm_nan=A, cfg_alarm_zero=0,
                cfg_batch_neg=A, cfg_batch_zero=0, cfg_frames_neg=A, cfg_frames_zero=0,
                run_ok=0, run_ok_no_per_frame=0, run_a_null=A, run_b_null=A, run_frames_null=A, run_summary_null=A, run_marks_null=A, run_b_zero=A,
                run_frames_negative=A, run_b_over=S, run_frames_over=S, run_a_pitch=S, run_b_pitch=S, run_out_pitch=S, run_out_pitch_unused=0)
    assert got == want


def _inputs(M, seed=1):
    return MU.mels(len(FRAMES), M, max(FRAMES), seed), MU.mels(len(FRAMES), M, max(FRAMES), seed + 1)


@pytest.mark.parametrize('M,n_cep', CASES)
def test_hook_and_yardstick_against_float64_inside_the_derived_bound(M, n_cep):
    """every element of every row: the hook (the device's arithmetic and order) and plain numpy float32 (the yardstick) both lie inside the bound derived in
    tests/melcmp_util.py from the float64 values alone; elements beyond frames[b] are NaN and change nothing"""
    from wavenet_vocoder import _ext
    a, b = _inputs(M)
    ref = MU.reference(a, b, FRAMES, n_cep, UNIT, ALARM)
    bnd = MU.bounds(a, b, FRAMES, n_cep, UNIT)
    yard = MU.reference(a, b, FRAMES, n_cep, UNIT, ALARM, dtype=np.float32)
    h = _ext.melcmp_host(MU.poison(a, FRAMES), MU.poison(b, FRAMES), FRAMES, n_cep=n_cep, unit_db=UNIT, alarm_db=ALARM)
    for r in range(len(FRAMES)):
        rh = MU.check_row(h['per_frame'][r], h['summary'][r], h['marks'][r], ref[r], bnd[r], ALARM, ('hook', M, n_cep, r))
        ry = MU.check_row(yard[r]['per_frame'], yard[r]['summary'], yard[r]['marks'], ref[r], bnd[r], ALARM, ('yardstick', M, n_cep, r))
        print('M %d n_cep %d row %d: hook worst err / bound %.3f, yardstick %.3f' % (M, n_cep, r, max(rh.values()), max(ry.values())))
    MU.check_against_yardstick([(h['per_frame'][r], h['summary'][r]) for r in range(len(FRAMES))], [(yard[r]['per_frame'], yard[r]['summary']) for r in range(len(FRAMES))],
                               ref, bnd, (M, n_cep))
    assert np.all(np.isnan(h['per_frame'][1][:, 1:])) and np.all(np.isfinite(h['summary']))      # nothing is written beyond a row's frames


@pytest.mark.parametrize('M,n_cep', CASES)
def test_identical_inputs_give_exact_zero(M, n_cep):
    from wavenet_vocoder import _ext
    a, _ = _inputs(M)
    h = _ext.melcmp_host(a, a.copy(), FRAMES, n_cep=n_cep, unit_db=UNIT, alarm_db=0.0)
    for r, F in enumerate(FRAMES):
        assert np.all(h['per_frame'][r][:, :F] == 0.0) and np.all(h['summary'][r] == 0.0)
        assert tuple(h['marks'][r]) == ((0, 0) if F else (-1, 0))


@pytest.mark.parametrize('M,n_cep', CASES)
def test_a_constant_offset_is_all_bias(M, n_cep):
    """a = b + delta: bias = l1 = lsd = unit_db * delta within the bound; l1c, lsdc and mcd within their bounds of 0"""
    from wavenet_vocoder import _ext
    _, b = _inputs(M)
    delta = np.float32(0.375)
    a = (b + delta).astype(np.float32)
    ref = MU.reference(a, b, FRAMES, n_cep, UNIT, ALARM)
    bnd = MU.bounds(a, b, FRAMES, n_cep, UNIT)
    h = _ext.melcmp_host(a, b, FRAMES, n_cep=n_cep, unit_db=UNIT, alarm_db=ALARM)
    want = float(np.float32(UNIT)) * float(delta)
    for r, F in enumerate(FRAMES):
        if F == 0:
            continue
        MU.check_row(h['per_frame'][r], h['summary'][r], h['marks'][r], ref[r], bnd[r], ALARM, (M, n_cep, r))
        pf, bd = h['per_frame'][r][:, :F].astype(np.float64), bnd[r]['per_frame']
        # the reference itself: a - b is delta up to the rounding of b + delta, u |a| per element, which the float64 reference carries
        slack = float(np.float32(UNIT)) * MU.U * float(np.abs(a).max())
        for j in (0, 1):
            assert np.all(np.abs(pf[j] - want) <= bd[j] + slack), (r, j)
        assert np.all(np.abs(pf[2] ** 2 - want ** 2) <= bd[2] + 2 * want * slack + slack ** 2), r
        assert np.all(pf[4] <= bd[4] + 2 * slack) and np.all(pf[5] ** 2 <= bd[5] + 4 * slack ** 2), r
        A = np.abs(MU.dct_table(M, n_cep)).sum(axis=1) * slack if n_cep else np.zeros(1)
        assert np.all(pf[3] ** 2 <= bd[3] + 0.5 * np.sum(A * A) * 4), r


def _same(x, y, frames):
    for r, F in enumerate(frames):
        assert np.array_equal(MU.bits(x['per_frame'][r][:, :F]), MU.bits(y['per_frame'][r][:, :F])), r
    assert np.array_equal(MU.bits(x['summary']), MU.bits(y['summary'])) and np.array_equal(x['marks'], y['marks'])


@pytest.mark.parametrize('M,n_cep', [(13, 12), (80, 13)])
def test_hook_bit_identity(M, n_cep):
    """across the two layouts of either input, across pitches, of a row alone against the same row inside a batch at another index, with and without per_frame"""
    from wavenet_vocoder import _ext
    a, b = _inputs(M)
    kw = dict(n_cep=n_cep, unit_db=UNIT, alarm_db=ALARM)
    base = _ext.melcmp_host(a, b, FRAMES, **kw)
    for a_cf in (True, False):
        for b_cf in (True, False):
            for ap, bp, op in ((300, 300, 300), (301, 517, 333)):
                got = _ext.melcmp_host(MU.layout(a, a_cf, ap), MU.layout(b, b_cf, bp), FRAMES, a_channels_first=a_cf, b_channels_first=b_cf, out_pitch=op, **kw)
                _same(base, got, FRAMES)
    for r in (2, 4):
        alone = _ext.melcmp_host(a[r:r + 1], b[r:r + 1], [FRAMES[r]], **kw)
        F = FRAMES[r]
        assert np.array_equal(MU.bits(alone['per_frame'][0][:, :F]), MU.bits(base['per_frame'][r][:, :F]))
        assert np.array_equal(MU.bits(alone['summary'][0]), MU.bits(base['summary'][r])) and np.array_equal(alone['marks'][0], base['marks'][r])
    order = [4, 0, 2, 1, 3]
    perm = _ext.melcmp_host(a[order], b[order], [FRAMES[i] for i in order], **kw)
    assert np.array_equal(MU.bits(perm['summary']), MU.bits(base['summary'][order])) and np.array_equal(perm['marks'], base['marks'][order])
    bare = _ext.melcmp_host(a, b, FRAMES, per_frame=False, **kw)
    assert np.array_equal(MU.bits(bare['summary']), MU.bits(base['summary'])) and np.array_equal(bare['marks'], base['marks']) and 'per_frame' not in bare


def test_poison_beyond_a_rows_frames_changes_nothing():
    from wavenet_vocoder import _ext
    a, b = _inputs(80)
    kw = dict(n_cep=13, unit_db=UNIT, alarm_db=ALARM)
    base = _ext.melcmp_host(a, b, FRAMES, **kw)
    for cf in (True, False):
        got = _ext.melcmp_host(MU.layout(MU.poison(a, FRAMES), cf, 311), MU.layout(MU.poison(b, FRAMES), cf, 302), FRAMES, a_channels_first=cf, b_channels_first=cf, **kw)
        _same(base, got, FRAMES)


def test_worst_frame_is_the_first_maximum_and_alarms_are_counted():
    from wavenet_vocoder import _ext
    M, F = 13, 600                                 # more than two strides of the 256 lanes
    b = MU.mels(1, M, F, 3)
    a = b.copy()
    a[0, ::2, 400] += 1.0; a[0, ::2, 70] += 1.0    # the same disturbance twice: equal l1c up to rounding is not guaranteed, so make frame 70 exactly frame 400
    a[0, :, 400] = a[0, :, 70]; b[0, :, 400] = b[0, :, 70]
    h = _ext.melcmp_host(a, b, [F], n_cep=12, unit_db=UNIT, alarm_db=1.0)
    assert tuple(h['marks'][0]) == (70, 2)
    assert h['summary'][0, 6] == h['per_frame'][0, 4, 70] == h['per_frame'][0, 4, 400]


# ---- hparams, ReconstructionCheck, the Synthesizer's plumbing, the TSV, the command line
def test_hparams_keys_keep_todays_behaviour_by_default():
    import hparams as H
    hp = H._build()
    assert hp.mi355_reconstruction_check is False and hp.mi355_reconstruction_alarm_db > 0
    hp.parse('mi355_reconstruction_check=True,mi355_reconstruction_alarm_db=2.5')
    assert hp.mi355_reconstruction_check is True and hp.mi355_reconstruction_alarm_db == 2.5
    from wavenet_vocoder import _ext
    assert _ext.melcmp_unit_db(H._build()) == 12.5                                        # 100 dB over [-4, 4]
    assert _ext.melcmp_unit_db(make_hp(symmetric_mels=False)) == 25.0 and _ext.melcmp_unit_db(make_hp(signal_normalization=False)) == 1.0


class _Analyzer(object):
    """stands in for _ext.MelAnalyzer: records the calls, returns a channels-first mel of ones"""
    def __init__(self, M, hop):
        self.M, self.hop, self.calls = M, hop, []

    def run(self, wav, lengths, channels_first=False, **kw):
        self.calls.append((tuple(wav.shape), list(lengths), channels_first))
        return torch.ones(wav.shape[0], self.M, 1 + max(lengths) // self.hop)


class _Compare(object):
    """stands in for _ext.MelCompare: records the calls; summary row b = b + j / 8, marks (b, 2 b)"""
    def __init__(self):
        self.calls = []

    def run(self, a, b, frames, a_channels_first=True, b_channels_first=True, per_frame=False):
        self.calls.append((tuple(a.shape), tuple(b.shape), list(frames), a_channels_first, b_channels_first, per_frame))
        B = a.shape[0]
        res = {'summary': torch.arange(B, dtype=torch.float32)[:, None] + torch.arange(7, dtype=torch.float32)[None, :] / 8,
               'marks': torch.stack((torch.arange(B, dtype=torch.int32), 2 * torch.arange(B, dtype=torch.int32)), 1)}
        if per_frame:
            res['per_frame'] = torch.zeros(B, 6, max(frames))
        return res


def _check(hp, rows=3, max_samples=160):
    from wavenet_vocoder.reconstruction import ReconstructionCheck
    return ReconstructionCheck(hp, rows, max_samples, analyzer=_Analyzer(int(hp.num_mels), int(hp.hop_size)), compare=_Compare())


HP16 = dict(cin_channels=16, num_mels=16, hop_size=16, upsample_scales=[4, 4])


def test_reconstruction_check_plumbing():
    hp = make_hp(**HP16)
    chk = _check(hp)
    assert chk.unit_db == 12.5 and chk.preemphasis == pytest.approx(0.97) and chk.alarm_db == hp.mi355_reconstruction_alarm_db
    table = chk.score(torch.zeros(2, 160), [160, 96], torch.zeros(2, 16, 10))
    assert table.shape == (2, 9) and table.dtype == np.float32
    assert np.array_equal(table[1], np.array([1, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1, 2], np.float32))
    assert chk.analyzer.calls == [((2, 160), [160, 96], True)]
    assert chk.compare.calls == [((2, 16, 11), (2, 16, 10), [10, 6], True, True, False)]      # Tc + 1 analysed frames, Tc compared
    table, pf = chk.score(torch.zeros(1, 160), [160], torch.zeros(1, 10, 16), frames=[7], per_frame=True, c_channels_first=False)
    assert pf.shape == (1, 6, 7) and chk.compare.calls[-1][2:] == ([7], True, False, True)
    with pytest.raises(ValueError):
        chk.score(torch.zeros(1, 160), [160], torch.zeros(1, 16, 9))                     # fewer frames of conditioning than are compared
    with pytest.raises(ValueError):
        chk.score(torch.zeros(1, 160), [160], torch.zeros(1, 15, 10))
    assert _check(make_hp(preemphasize=False, **HP16)).preemphasis == 0.0
    from wavenet_vocoder.reconstruction import ReconstructionCheck
    assert ReconstructionCheck(hp, 1, 16, preemphasis=0.5, alarm_db=1.5, analyzer=_Analyzer(16, 16), compare=_Compare()).alarm_db == 1.5
    from wavenet_vocoder.models.wavenet import WaveNet
    m = WaveNet(hp)
    m._hparams = make_hp(**dict(HP16, cin_channels=20))                                  # (the constructor asserts the same of a locally conditioned model)
    with pytest.raises(ValueError, match='cin_channels'):
        m.reconstruction_check(1, 160)


def test_synthesizer_scores_every_utterance_and_appends_the_tsv(tmp_path):
    from wavenet_vocoder import reconstruction as R
    from wavenet_vocoder.synthesizer import Synthesizer

    class _Model(object):
        device = torch.device('cpu')

        def __init__(self, hp):
            self.hp, self.made = hp, []

        def reconstruction_check(self, rows, max_samples):
            self.made.append((rows, max_samples))
            return _check(self.hp, rows, max_samples)

    out = str(tmp_path)
    cond = np.zeros((3, 10, 16), np.float32)
    wavs = [np.zeros(160, np.float32), np.zeros(96, np.float32), np.zeros(128, np.float32)]
    s = Synthesizer(); s._hparams = make_hp(**HP16); s.model = _Model(s._hparams); s._recon = None
    assert s._reconstruction(None, wavs, cond, [10, 6, 8], ['a', 'b', 'c'], out) is None and os.listdir(out) == []      # the switch is off: nothing happens
    s._hparams = make_hp(mi355_reconstruction_check=True, **HP16); s.model = _Model(s._hparams)
    t = s._reconstruction(None, wavs, cond, [10, 6, 8], ['a', 'b', 'c'], out)                                           # the host path: what is about to be written is uploaded
    assert t.shape == (3, 9) and s.model.made == [(3, 160)]
    assert s._recon.analyzer.calls == [((3, 160), [160, 96, 128], True)] and s._recon.compare.calls[0][2:5] == ([10, 6, 8], True, False)
    s._reconstruction(torch.zeros(2, 200), None, cond[:2], [10, 6], ['d', 'e'], out)                                     # the device path: the decoded tensor as it is
    assert s.model.made == [(3, 160)] and s._recon.analyzer.calls[-1] == ((2, 200), [160, 96], True)
    s._reconstruction(torch.zeros(4, 320), None, np.zeros((4, 20, 16), np.float32), [20, 1, 1, 1], list('fghi'), out)    # outgrown: a larger check replaces it
    assert s.model.made == [(3, 160), (4, 320)]
    rows = R.read_tsv(os.path.join(out, 'reconstruction.tsv'))
    assert [r['name'] for r in rows] == list('abcdefghi') and [int(r['frames']) for r in rows] == [10, 6, 8, 10, 6, 20, 1, 1, 1]
    assert rows[1]['l1c_db'] == '1.5000' and rows[1]['worst_frame'] == '1' and rows[1]['alarm_frames'] == '2' and rows[1]['bias_db'] == '1.0000'
    assert open(os.path.join(out, 'reconstruction.tsv')).read().count('name\tframes') == 1                               # one header, rows appended
    line = R.log_line(['a', 'b', 'c'], t)
    assert 'worst c' in line and '3 utterance(s)' in line


def test_command_line_table_on_two_synthetic_pairs(tmp_path, capsys):
    """--host: numpy analysis and the host hook.  A pair whose wav is the signal the mel was made of scores (near) zero and sorts first; a disturbed one last."""
    from datasets import audio
    from scipy.io import wavfile
    from wavenet_vocoder import reconstruction as R
    hp = make_hp(num_mels=20, cin_channels=20, n_fft=256, hop_size=64, win_size=256, sample_rate=8000, fmin=50, fmax=3800, rescale=False)
    rng = np.random.RandomState(0)
    wav_dir, mel_dir = str(tmp_path / 'wavs'), str(tmp_path / 'mels')
    os.makedirs(wav_dir); os.makedirs(mel_dir)
    lines = []
    for i, noise in enumerate((0.0, 0.2)):
        x = 0.3 * np.sin(2 * np.pi * 440 * np.arange(64 * 30) / 8000.0) + 0.05 * rng.randn(64 * 30)
        pcm = (x * 32767 / np.abs(x).max()).astype(np.int16)
        mel = audio.melspectrogram(audio.preemphasis(pcm.astype(np.float32).astype(np.float64) / 32768.0, hp.preemphasis, hp.preemphasize), hp).T[:30]
        if noise:
            pcm = np.clip(pcm + noise * 32767 * rng.randn(pcm.size), -32767, 32767).astype(np.int16)
        wavfile.write(os.path.join(wav_dir, 'wavenet-audio-mel-u%d.wav' % i), 8000, pcm)
        np.save(os.path.join(mel_dir, 'mel-u%d.npy' % i), mel.astype(np.float32))
        lines.append('%s|%s|%s' % ('rec-%d.wav' % i, os.path.join(mel_dir, 'mel-u%d.npy' % i), os.path.join(wav_dir, 'wavenet-audio-mel-u%d.wav' % i)))
    with open(os.path.join(wav_dir, 'map.txt'), 'w') as f:
        f.write('\n'.join(lines) + '\n')
    over = 'num_mels=20,cin_channels=20,n_fft=256,hop_size=64,win_size=256,sample_rate=8000,fmin=50,fmax=3800'
    names, frames, table = R.main(['--map', os.path.join(wav_dir, 'map.txt'), '--host', '--hparams', over, '--tsv', str(tmp_path / 't.tsv')])
    text = capsys.readouterr().out.splitlines()
    assert names == ['mel-u0', 'mel-u1'] and frames == [30, 30]
    assert text[0].split('\t') == list(R.TSV_HEADER) and text[1].startswith('mel-u0\t30\t') and text[2].startswith('mel-u1\t30\t')
    assert 'Worst utterances' in '\n'.join(text) and text[-2].strip().endswith('mel-u1')
    assert abs(table[0, 4]) < 1e-3 and abs(table[0, 0]) < 1e-3 and table[1, 4] > 1.0 and table[1, 3] > table[0, 3]
    assert [r['name'] for r in R.read_tsv(str(tmp_path / 't.tsv'))] == names
    wavfile.write(os.path.join(wav_dir, 'wavenet-audio-orphan.wav'), 8000, np.zeros(64, np.int16))      # no mel for it: skipped, and said so
    n2, f2, t2 = R.main(['--wavs', wav_dir, '--mels', mel_dir, '--host', '--hparams', over, '--worst', '1'])
    assert 'skipped 1 wav file(s)' in capsys.readouterr().out
    with open(os.path.join(wav_dir, 'map.txt'), 'a') as f:
        f.write('some text|0\n')
    pairs, skipped = R.read_pairs(os.path.join(wav_dir, 'map.txt'))
    assert [p[0] for p in pairs] == names and skipped == 1
    assert n2 == names and np.array_equal(t2, table)
