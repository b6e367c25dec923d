"""Output stage, host side (no GPU): the C ABI names, the validation of a configuration and of a call, the stage's arithmetic evaluated on the host
through wn_test_post_host (the very functions the kernels inline, csrc/wn_post.h) against the numpy mirror of tests/post_util.py bit for bit, its
independence of how a row is cut, its accuracy against float64 by a derived bound, the PCM conversion against save_wavenet_wav and the host driver
path, the host functions under ASAN + UBSAN in a stand-alone program, and the façade's post= plumbing against stand-in engines."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import post_util as PU
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
NAMES = ('wn_post_create', 'wn_post_push', 'wn_post_finish', 'wn_test_post_host')
WN_E_ARG, WN_E_SHAPE, WN_E_HIP = -1, -2, -3
KS = (0.0, 0.85, 0.97)
SIZES = (1, 63, 64, 65, 1025, 4099)


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    for name in NAMES + ('wn_post_destroy', 'wn_post_last_error'):
        assert name in _ext.exported_symbols() and hasattr(lib, name), name
    for name in NAMES:
        assert name in declared, name
    assert 'void wn_post_destroy(' in text and 'const char* wn_post_last_error(' in text
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert 'wn_test_post_host(' in hooks and 'wn_post_push(' not in hooks and 'wn_post_create(' not in hooks      # the hook alone is fenced
    assert ctypes.sizeof(_ext.WnPostConfig) == 20


def _create(**kw):
    from wavenet_vocoder import _ext
    cfg = _ext.post_config(kw.pop('max_rows', 2), kw.pop('in_type', 0), kw.pop('deemphasis', 0.97), kw.pop('gain', 1.0))
    for k, v in kw.items():
        setattr(cfg, k, v)
    h = ctypes.c_void_p()
    rc = _ext.load_library().wn_post_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == 0:
        _ext.load_library().wn_post_destroy(h)
    return rc


def test_create_validates_before_any_device_call():
    """every configuration error is WN_E_ARG with a text, on a machine without a device too; a valid one gets as far as the device (WN_E_HIP without one)"""
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    h = ctypes.c_void_p()
    assert lib.wn_post_create(None, ctypes.byref(h)) == WN_E_ARG
    assert lib.wn_post_create(ctypes.byref(_ext.post_config(1, 0)), None) == WN_E_ARG
    bad = [dict(abi_version=5), dict(max_rows=0), dict(max_rows=-3), dict(in_type=3), dict(in_type=-1), dict(deemphasis=1.0), dict(deemphasis=-0.01),
           dict(deemphasis=float('nan')), dict(deemphasis=float('inf')), dict(gain=0.0), dict(gain=-1.0), dict(gain=float('inf')), dict(gain=float('nan'))]
    for kw in bad:
        assert _create(**kw) == WN_E_ARG, kw
        assert (lib.wn_post_last_error(None) or b'').startswith(b'wn_post_create: '), kw
    assert _create() == (0 if torch.cuda.is_available() else WN_E_HIP)
    assert _create(deemphasis=0.0, in_type=2, gain=0.001) == (0 if torch.cuda.is_available() else WN_E_HIP)
    # a call without a handle is an argument error, never a crash
    buf = (ctypes.c_float * 4)(); n = (ctypes.c_int32 * 1)(4)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.wn_post_push(None, p, 4, n, None, 1, p, None, 4, None, None) == WN_E_ARG
    assert lib.wn_post_finish(None, p, 4, n, 1, p, None, 4, None, None) == WN_E_ARG
    lib.wn_post_destroy(None)
    # the hook validates the same configuration
    for kw in (dict(in_type=3), dict(deemphasis=1.0), dict(gain=0.0), dict(max_rows=0)):
        cfg = _ext.post_config(1, 0, 0.5)
        for k, v in kw.items():
            setattr(cfg, k, v)
        assert lib.wn_test_post_host(ctypes.byref(cfg), p, 4, 0.0, 1.0, p, None, None) == WN_E_ARG, kw
    cfg = _ext.post_config(1, 0, 0.5)
    assert lib.wn_test_post_host(ctypes.byref(cfg), None, 4, 0.0, 1.0, p, None, None) == WN_E_ARG
    assert lib.wn_test_post_host(ctypes.byref(cfg), p, -1, 0.0, 1.0, p, None, None) == WN_E_ARG
    assert lib.wn_test_post_host(None, p, 4, 0.0, 1.0, p, None, None) == WN_E_ARG
    assert lib.wn_test_post_host(ctypes.byref(cfg), None, 0, 0.0, 1.0, None, None, None) == 0


@pytest.fixture(scope='module')
def host_program(tmp_path_factory):
    """tests/host/post_main.cpp built with ASAN + UBSAN, run once as an ordinary child process"""
    exe = str(tmp_path_factory.mktemp('post') / 'post_main')
    r = subprocess.run(['hipcc', '-std=c++20', '-O1', '-g', '-Wall', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=undefined',
                        '-I', os.path.join(ROOT, 'tacotron-2_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'post_main.cpp'), '-o', exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    return subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)


def test_host_functions_under_address_and_ub_sanitizers(host_program):
    """decode, chain, conversion and the row loop of the hook over n in {0, 1, 63, 64, 65, 1025, 4099} x 3 input types x 3 coefficients in heap blocks of
    exactly the row's size; the program checks the carry, the clip count, the peak and the independence of a cut itself"""
    r = host_program
    assert r.returncode == 0 and 'post ok' in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_every_validation_code_of_a_call(host_program):
    """wn_post_push / wn_post_finish run wn_post_check_call (csrc/wn_post.h) before any device call; a handle needs a device, so the function is exercised
    in the stand-alone host program (B <= max_rows = 4 there).  The same cases run against a real handle in tests/test_hip_post.py."""
    got = dict(l.split()[1:] for l in host_program.stdout.splitlines() if l.startswith('code '))
    got = {k: int(v) for k, v in got.items()}
    want = dict(cfg_null=WN_E_ARG, cfg_ok=0, cfg_abi=WN_E_ARG, cfg_rows=WN_E_ARG, cfg_type_hi=WN_E_ARG, cfg_type_lo=WN_E_ARG, cfg_k_one=WN_E_ARG, cfg_k_neg=WN_E_ARG,
                cfg_k_nan=WN_E_ARG, cfg_k_zero=0, cfg_gain_zero=WN_E_ARG, cfg_gain_neg=WN_E_ARG, cfg_gain_inf=WN_E_ARG, cfg_gain_nan=WN_E_ARG,
                push_ok=0, push_ok_pcm_only=0, push_ok_float_only=0, push_in_null=WN_E_ARG, push_n_null=WN_E_ARG, push_no_output=WN_E_ARG, push_b_zero=WN_E_ARG,
                push_n_negative=WN_E_ARG, push_b_over=WN_E_SHAPE, push_in_pitch=WN_E_SHAPE, push_out_pitch=WN_E_SHAPE,
                finish_ok=0, finish_no_float=WN_E_ARG, finish_b_over=WN_E_SHAPE, finish_out_pitch=WN_E_SHAPE)
    assert got == want


@pytest.mark.parametrize('in_type', [0, 1, 2])
@pytest.mark.parametrize('k', KS)
def test_hook_equals_the_mirror_bit_for_bit(in_type, k):
    from wavenet_vocoder import _ext
    for n in SIZES:
        a = PU.samples(in_type, n, seed=100 * in_type + n)
        y, q, carry = _ext.post_host(a, in_type, k, carry_in=-0.3125, pcm_scale=PU.push_scale(1.0))
        my, mq, _, mc = PU.mirror_push(in_type, a, k, carry=-0.3125)
        assert np.array_equal(PU.bits(y), PU.bits(my)), n
        assert np.array_equal(q, mq) and PU.bits(carry) == PU.bits(mc), n


@pytest.mark.parametrize('in_type', [0, 1, 2])
def test_a_row_cut_into_pushes_equals_the_uncut_row(in_type):
    """n = 4099 as 7 + 1018 + 0 + 3074 through carry_out -> carry_in"""
    from wavenet_vocoder import _ext
    a = PU.samples(in_type, 4099, seed=7)
    whole, wq, wc = _ext.post_host(a, in_type, 0.97)
    parts, pq, carry, t0 = [], [], 0.0, 0
    for n in (7, 1018, 0, 3074):
        y, q, carry = _ext.post_host(a[t0:t0 + n], in_type, 0.97, carry_in=carry)
        parts.append(y); pq.append(q); t0 += n
    assert t0 == 4099
    assert np.array_equal(PU.bits(np.concatenate(parts)), PU.bits(whole)) and np.array_equal(np.concatenate(pq), wq) and PU.bits(carry) == PU.bits(wc)


def test_coefficient_zero_returns_the_bits_of_the_decode():
    from wavenet_vocoder import _ext
    x = PU.samples(0, 257, seed=1)
    x[0], x[5], x[256] = np.float32(-0.0), np.float32(1e-42), np.float32(-0.0)       # no arithmetic: the sign of zero and a denormal stay what they are
    y, _, carry = _ext.post_host(x, 0, 0.0, carry_in=0.75)
    assert np.array_equal(PU.bits(y), PU.bits(x)) and PU.bits(carry) == PU.bits(np.float32(-0.0))
    y, _, _ = _ext.post_host(np.zeros(4, np.float32), 1, 0.0)                          # mu-law 0 decodes to sign(0) * ... = +0.0
    assert np.array_equal(PU.bits(y), PU.bits(PU.decode(1, np.zeros(4, np.float32))))
    q = np.arange(-4, 262, dtype=np.int32)
    y, _, _ = _ext.post_host(q, 2, 0.0)
    assert np.array_equal(PU.bits(y), PU.bits(PU.DECODE_TABLE[np.clip(q, 0, 255)]))
    assert _ext.post_host(np.zeros(0, np.float32), 0, 0.0, carry_in=0.75)[2] == np.float32(0.75)      # an empty push leaves the state alone


def test_accuracy_against_float64_by_the_derived_bound():
    """Each step commits at most two roundings of at most 2^-24 max|y| each (the product and the sum), and an error made at step t reaches step t + j
    scaled by k^j: |y32 - y64| <= 2 / (1 - k) 2^-24 max|y64|.  Speech-like input (pre-emphasised integrated noise, peak 0.9), 20 000 samples, 6 seeds.
    Measured: the hook's worst err / bound over the 6 seeds is 0.099 (the mirror's, the same bits, too); profiles/post_parity.json."""
    from wavenet_vocoder import _ext
    k = 0.97
    worst = 0.0
    for seed in range(6):
        x = PU.speech_like(20000, seed, k)
        y, _, _ = _ext.post_host(x, 0, k)
        ref = PU.lfilter64(x, k)
        bound = 2.0 / (1.0 - float(np.float32(k))) * 2.0 ** -24 * np.max(np.abs(ref))
        err = np.max(np.abs(y.astype(np.float64) - ref))
        print('seed %d: err %.3e bound %.3e ratio %.3f' % (seed, err, bound, err / bound))
        worst = max(worst, err / bound)
        assert err <= bound, (seed, err, bound)
    path = os.path.join(ROOT, 'profiles', 'post_parity.json')
    if os.path.exists(path):
        rec = json.load(open(path))
        assert abs(rec['hook_worst_err_over_bound'] - worst) < 1e-6, (rec, worst)      # the arithmetic is exact to reproduce: so is the record


def test_finish_pcm_is_save_wavenet_wav_arithmetic():
    """int16 of the finish arithmetic (s = fl32(32767 / max(0.01, peak)) in double, fl32(y s), truncation) on a float32 y == save_wavenet_wav's cast"""
    from wavenet_vocoder import _ext
    for seed, amp in ((0, 1.0), (1, 0.3), (2, 0.004), (3, 7.0)):      # a peak above 1, and one below the 0.01 floor
        x = (PU.speech_like(4099, seed) * np.float32(amp)).astype(np.float32)
        y, mq, peak = PU.mirror_finish(0, x, 0.97)
        want = PU.save_wavenet_wav_pcm(y)
        assert np.array_equal(mq, want), seed
        _, hq, _ = _ext.post_host(y, 0, 0.0, pcm_scale=PU.peak_scale(peak))              # the hook's conversion at the same scale
        assert np.array_equal(hq, want), seed
        if amp >= 0.01:
            assert np.abs(want).max() == 32767                  # normalised to full scale (below the 0.01 floor the scale is capped instead)


def test_pcm_against_the_host_driver_path():
    """pcm(float32 chain) against pcm(float64 lfilter), the 'host' path of the driver (audio.inv_preemphasis + save_wavenet_wav): at most 1 LSB apart, on at
    most 2 % of the samples.  Measured on these inputs: 0.085 - 0.175 % of the samples differ, by one."""
    from datasets import audio
    k = 0.97
    for seed in range(6):
        x = PU.speech_like(20000, seed, k)
        dev = PU.mirror_finish(0, x, k)[1].astype(np.int32)
        host = PU.save_wavenet_wav_pcm(PU.lfilter64(x, k)).astype(np.int32)
        d = np.abs(dev - host)
        print('seed %d: %.3f %% of the samples differ, max %d' % (seed, 100.0 * np.mean(d > 0), d.max()))
        assert d.max() <= 1 and np.mean(d > 0) <= 0.02, seed
        # the driver's own expression: audio.inv_preemphasis at the float32 coefficient is this reference
        assert np.array_equal(PU.save_wavenet_wav_pcm(audio.inv_preemphasis(x, float(np.float32(k)))).astype(np.int32), host)


def test_decay_below_the_normal_range():
    """an impulse and 4000 zeros at k = 0.97: bit equality wherever the mirror's |y| >= 2^-126 (the first 2868 samples), |difference| <= 2^-126 below
    (flushed or gradual: unspecified).  The only test that excludes an element."""
    from wavenet_vocoder import _ext
    x = np.zeros(4001, np.float32); x[0] = 1.0
    y, _, _ = _ext.post_host(x, 0, 0.97)
    my, _ = PU.chain(x, 0.97)
    normal = np.abs(my) >= PU.TINY
    assert int(normal.sum()) == 2868 and normal[:2868].all()
    assert np.array_equal(PU.bits(y[normal]), PU.bits(my[normal]))
    assert np.max(np.abs(y[~normal].astype(np.float64) - my[~normal])) <= float(PU.TINY)


# ---- façade and hparams
def test_hparams_keys_keep_todays_behaviour_by_default():
    import hparams as H
    hp = H._build()
    assert hp.mi355_output_deemphasis is False and hp.mi355_output_stage == 'host' and hp.mi355_output_gain == 1.0
    hp.parse('mi355_output_deemphasis=True,mi355_output_stage=device,mi355_output_gain=0.5')
    assert hp.mi355_output_deemphasis is True and hp.mi355_output_stage == 'device' and hp.mi355_output_gain == 0.5
    from wavenet_vocoder.synthesizer import Synthesizer
    s = Synthesizer(); s._hparams = H._build()
    assert s._output_mode() == (False, 0.0)
    s._hparams.parse('mi355_output_deemphasis=True,mi355_output_stage=device')
    assert s._output_mode() == (True, float(np.float32(0.97)))       # the coefficient the device multiplies by, on the host path too
    s._hparams.parse('preemphasize=False')
    assert s._output_mode() == (True, 0.0)                      # nothing was pre-emphasised: nothing to undo
    s._hparams.parse('mi355_output_stage=gpu')
    with pytest.raises(ValueError):
        s._output_mode()


class _Engine(object):
    """stands in for _ext.Engine: pushes report the scheduled sample counts, everything else is recorded"""
    hop = 4

    def __init__(self):
        self.calls = []

    def stream_lookahead(self):
        return (0, 0)

    def stream_push(self, cc, out, raw, noise, ti, final=False):
        self.calls.append(('stream_push',))
        return 0 if cc is None else int(cc.shape[-1]) * self.hop

    def slots_push(self, cc, frames, final, out, raw):
        self.calls.append(('slots_push',))
        return [f * self.hop for f in frames]

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


class _Stage(object):
    """stands in for _ext.OutputStage: records (n, restart) of every push"""
    in_type = 0

    def __init__(self):
        self.pushes, self.finishes = [], []

    def push(self, samples, n=None, restart=None, pcm=True, float_out=False, clipped=False):
        self.pushes.append((tuple(samples.shape), list(n), restart if restart in (None, True) else list(restart), pcm, float_out))
        q, y = torch.full(samples.shape, 7, dtype=torch.int16), torch.full(samples.shape, 0.5)
        res = tuple(t for t, on in ((q, pcm), (y, float_out)) if on)
        return res[0] if len(res) == 1 else res

    def finish(self, samples, lengths, pcm=True):
        self.finishes.append((tuple(samples.shape), list(lengths)))
        return torch.zeros(samples.shape), torch.zeros(samples.shape, dtype=torch.int16)


def _model(**kw):
    from wavenet_vocoder.models.wavenet import WaveNet
    m = WaveNet(make_hp(**dict(dict(out_channels=30, cin_channels=16, num_mels=16, hop_size=4, upsample_scales=[2, 2]), **kw)))
    m.engine, m._dirty, m.device = _Engine(), False, torch.device('cpu')
    return m


def test_stream_push_with_a_stage_restarts_once_and_returns_the_chunk():
    m = _model()
    st, post = m.stream(2, seed=1), _Stage()
    c = torch.zeros(2, 16, 3)
    out, chunk = st.push(c, post=post)
    assert out.shape == (2, 12) and chunk.shape == (2, 12) and chunk.dtype == torch.int16
    out, raw, (q, y) = st.push(c[:, :, :1], return_raw=True, post=post, post_output='both')
    assert q.shape == (2, 4) and y.dtype == torch.float32 and raw.shape == (2, 30, 4)
    out, y = st.push(None, post=post, post_output='float')                  # no new frames: an empty chunk, and the state runs on
    assert out.shape == (2, 0) and y.shape == (2, 0)
    assert [(p[1], p[2]) for p in post.pushes] == [([12, 12], True), ([4, 4], None), ([0, 0], None)]
    assert isinstance(st.push(c), torch.Tensor) and len(post.pushes) == 3      # without post= the call is what it was
    with pytest.raises(ValueError):
        st.push(c, post=post, post_output='wav')


def test_slot_session_marks_a_slot_for_restart_at_its_next_push():
    m = _model()
    sess, post = m.slots(3), _Stage()
    sess.open(0, seed=1); sess.open(2, seed=2)
    c = torch.zeros(16, 2)
    r = sess.push({0: c}, post=post)                                        # slot 2 was opened and is not pushed: its restart waits
    assert r[0][0].shape == (8,) and r[0][1].shape == (8,) and r[0][1].dtype == torch.int16
    r = sess.push({0: (c, True), 2: c[:, :1]}, post=post)
    r = sess.push({2: c}, post=post)
    sess.open(0, seed=3)                                                    # reopened: restarted again at its next push
    r = sess.push({0: c, 2: c}, return_raw=True, post=post, post_output='float')
    assert len(r[0]) == 3 and r[0][2].dtype == torch.float32 and r[2][1].shape == (30, 8)
    assert [(p[1], p[2]) for p in post.pushes] == [([8, 0, 0], [1, 0, 0]), ([8, 0, 4], [0, 0, 1]), ([0, 0, 8], [0, 0, 0]), ([8, 0, 8], [1, 0, 0])]
    assert isinstance(sess.push({2: c}), dict) and isinstance(sess.push({2: c})[2], torch.Tensor) and len(post.pushes) == 4


def test_folded_refuses_a_stage_that_would_decode_twice():
    m = _model(input_type='mulaw-quantize', quantize_channels=256, out_channels=256)
    post = _Stage(); post.in_type = 2
    with pytest.raises(ValueError, match='raw'):
        m.folded([torch.zeros(16, 50)], rows=1, post=post)
    assert not [c for c in m.engine.calls if c[0] == 'synthesize_folded']


def test_output_stage_defaults_follow_the_hparams():
    from wavenet_vocoder import _ext
    seen = []

    class Probe(_ext.OutputStage):
        def __init__(self, hparams, rows, deemphasis=None, gain=1.0, in_type=None):
            try:
                super().__init__(hparams, rows, deemphasis, gain, in_type)
            except _ext.WnError as e:
                assert e.code == WN_E_HIP                                # (no device on this machine: the configuration was accepted)
            seen.append((self.cfg.max_rows, self.cfg.in_type, round(float(self.cfg.deemphasis), 6), float(self.cfg.gain)))

    Probe(make_hp(), 3)
    Probe(make_hp(input_type='mulaw-quantize', quantize_channels=256, out_channels=256, preemphasize=False), 1)
    Probe(make_hp(input_type='mulaw'), 2, deemphasis=0.5, gain=2.0, in_type='raw')
    assert seen == [(3, 0, 0.97, 1.0), (1, 2, 0.0, 1.0), (2, 0, 0.5, 2.0)]
    with pytest.raises(ValueError):
        _ext.OutputStage(make_hp(), 1, in_type='pcm')
    with pytest.raises(_ext.WnError) as ei:
        _ext.OutputStage(make_hp(), 0)
    assert ei.value.code == WN_E_ARG
