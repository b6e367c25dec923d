"""Sampling temperature, host side (no GPU): the C ABI names, argument validation, the exact cases of the tempering function (evaluated on the
host through wn_test_temper_noise: the very function the noise kernels inline), its accuracy against the float64 restatement of
tests/temper_util.py, and the façade's temperature arguments against a recording stand-in engine."""
import ctypes
import os
import re

import numpy as np
import pytest

import temper_util as TU
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
NAMES = ('wn_synth_set_temperature', 'wn_synth_get_temperature', 'wn_synth_set_slot_temperature', 'wn_temper_noise', 'wn_test_temper_noise')
WN_E_ARG = -1
HEADS = {'mol': dict(out_channels=30), 'gauss': dict(out_channels=2),
         'softmax': dict(input_type='mulaw-quantize', quantize_channels=256, out_channels=256)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in _ext.exported_symbols()
        assert hasattr(lib, name)
    assert '#define WN_ABI_VERSION 4' in text and _ext.WN_ABI_VERSION == 4
    hooks = text[text.index('#ifndef WN_NO_TEST_HOOKS'):]
    assert 'wn_test_temper_noise' in hooks and 'wn_temper_noise(' not in hooks.replace('wn_test_temper_noise(', '')      # the hook alone is fenced


def test_null_context_is_an_argument_error():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    a, b = ctypes.c_float(), ctypes.c_float()
    buf = (ctypes.c_float * 4)()
    assert lib.wn_synth_set_temperature(None, 1.0, 1.0) == WN_E_ARG
    assert lib.wn_synth_get_temperature(None, ctypes.byref(a), ctypes.byref(b)) == WN_E_ARG
    assert lib.wn_synth_set_slot_temperature(None, 0, 1.0, 1.0) == WN_E_ARG
    assert lib.wn_temper_noise(None, ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf, ctypes.c_void_p), 1, 1, 1.0, 1.0, None) == WN_E_ARG


def test_hook_rejects_bad_arguments():
    from wavenet_vocoder import _ext
    x = np.full((3, 4), 0.25, np.float32)
    for bad in (float('nan'), -0.1, 2.5, float('inf')):
        for pair in ((bad, 1.0), (1.0, bad)):
            with pytest.raises(_ext.WnError) as ei:
                _ext.temper_noise_host(TU.MOL, x, *pair)
            assert ei.value.code == WN_E_ARG
    with pytest.raises(_ext.WnError) as ei:
        _ext.temper_noise_host(TU.SOFTMAX, np.zeros((3, 0), np.float32), 0.5, 0.5)          # nps < 1
    assert ei.value.code == WN_E_ARG
    lib = _ext.load_library()
    p = x.ctypes.data_as(ctypes.c_void_p)
    assert lib.wn_test_temper_noise(0, 0, p, p, 3, 0.5, 0.5) == WN_E_ARG
    assert lib.wn_test_temper_noise(0, -1, p, p, 3, 0.5, 0.5) == WN_E_ARG
    assert lib.wn_test_temper_noise(3, 4, p, p, 3, 0.5, 0.5) == WN_E_ARG
    assert lib.wn_test_temper_noise(0, 4, None, p, 3, 0.5, 0.5) == WN_E_ARG
    for ok in (0.0, 2.0, -0.0):
        _ext.temper_noise_host(TU.MOL, x, ok, ok)


def _rows(mode, nps, rows=4099, seed=3):
    if mode == TU.GAUSS:
        return np.random.RandomState(seed).randn(rows, nps).astype(np.float32)
    from hip_util import device_uniform_noise
    return device_uniform_noise(rows * nps, seed).reshape(rows, nps)


@pytest.mark.parametrize('mode,nps', [(TU.MOL, 11), (TU.GAUSS, 1), (TU.SOFTMAX, 256)])
def test_temperature_one_returns_the_input_bits(mode, nps):
    from wavenet_vocoder import _ext
    x = _rows(mode, nps, rows=257)
    x[0, 0] = TU.LO if mode != TU.GAUSS else np.float32(-0.0)
    x[1, nps - 1] = TU.HI if mode != TU.GAUSS else np.float32(1e-42)          # (a denormal stays what it is: no arithmetic is done)
    assert np.array_equal(_bits(_ext.temper_noise_host(mode, x, 1.0, 1.0)), _bits(x))


def test_temperature_zero_gives_the_three_literals():
    from wavenet_vocoder import _ext
    y = _ext.temper_noise_host(TU.MOL, _rows(TU.MOL, 11), 0.0, 0.0)
    assert np.array_equal(_bits(y[:, :10]), np.full(y[:, :10].shape, _bits(TU.SELECT_AT_ZERO)))
    assert np.array_equal(_bits(y[:, 10]), np.full(y.shape[0], _bits(TU.LOGISTIC_AT_ZERO)))
    y = _ext.temper_noise_host(TU.SOFTMAX, _rows(TU.SOFTMAX, 256, rows=33), 1.0, 0.0)
    assert np.array_equal(_bits(y), np.full(y.shape, _bits(TU.SELECT_AT_ZERO)))
    y = _ext.temper_noise_host(TU.GAUSS, _rows(TU.GAUSS, 1), 0.0, 1.0)
    assert np.array_equal(_bits(y), np.zeros(y.shape, np.uint32))                                # +0.0 whatever the sign of the draw
    assert float(np.log(np.float32(0.5)) - np.log(np.float32(1.0) - np.float32(0.5))) == 0.0     # the sampler's logit of 0.5f is exactly 0: x = clip(mu)


@pytest.mark.parametrize('tau', [0.3, 0.7, 0.95, 1.5, 2.0])
def test_normal_entries_are_one_float32_product(tau):
    from wavenet_vocoder import _ext
    x = _rows(TU.GAUSS, 1)
    y = _ext.temper_noise_host(TU.GAUSS, x, tau, 1.0)
    assert np.array_equal(_bits(y), _bits(np.float32(tau) * x))
    assert np.array_equal(_bits(_ext.temper_noise_host(TU.GAUSS, x, 1.0, tau)), _bits(x))        # the Gaussian head has no select entry


def test_mol_row_each_temperature_touches_its_own_entries():
    from wavenet_vocoder import _ext
    M = 10
    x = _rows(TU.MOL, M + 1)
    a = _ext.temper_noise_host(TU.MOL, x, 0.6, 1.0)
    assert np.array_equal(_bits(a[:, :M]), _bits(x[:, :M])) and not np.any(_bits(a[:, M]) == _bits(x[:, M]))
    b = _ext.temper_noise_host(TU.MOL, x, 1.0, 0.6)
    assert np.array_equal(_bits(b[:, M]), _bits(x[:, M])) and np.mean(_bits(b[:, :M]) == _bits(x[:, :M])) < 1e-3
    both = _ext.temper_noise_host(TU.MOL, x, 0.6, 0.6)
    assert np.array_equal(_bits(both[:, :M]), _bits(b[:, :M])) and np.array_equal(_bits(both[:, M]), _bits(a[:, M]))
    assert both.min() >= TU.LO and both.max() <= TU.HI
    sm = _ext.temper_noise_host(TU.SOFTMAX, x, 0.6, 1.0)                                         # softmax: tau_scale has nothing to act on
    assert np.array_equal(_bits(sm), _bits(x))


def test_accuracy_against_the_float64_mirror():
    """Measured where the sampler reads the noise (the Gumbel term of a select entry, the logit of a logistic entry), normalised by the float32
    floor of temper_util, on the 2^20 clamped uniforms of the device stream plus both ends of the clamp.  Limit: 8 x the worst normalised error of
    the same formulas in plain numpy float32 on the same inputs (the project's margin for library transcendentals that are not correctly rounded)."""
    from wavenet_vocoder import _ext
    u = TU.hardest_inputs()
    worst = {TU.SELECT: [0.0, 0.0], TU.LOGISTIC: [0.0, 0.0]}
    col = u.reshape(-1, 1)
    for tau in TU.TAUS:
        got = {TU.SELECT: _ext.temper_noise_host(TU.SOFTMAX, col, 1.0, tau)[:, 0],                # (one entry per row: softmax rows are select entries,
               TU.LOGISTIC: _ext.temper_noise_host(TU.MOL, col, tau, 1.0)[:, 0]}                 # the last entry of a MoL row is the logistic draw)
        for kind in worst:
            assert got[kind].min() >= TU.LO and got[kind].max() <= TU.HI
            worst[kind][0] = max(worst[kind][0], TU.worst_error(u, got[kind], kind, tau))
            worst[kind][1] = max(worst[kind][1], TU.worst_error(u, TU.temper_kind(u, kind, tau, np.float32), kind, tau))
    print('\nworst normalised error (library, numpy float32 yardstick): select %.3f %.3f, logistic %.3f %.3f'
          % (worst[TU.SELECT][0], worst[TU.SELECT][1], worst[TU.LOGISTIC][0], worst[TU.LOGISTIC][1]))
    for kind, name in ((TU.SELECT, 'select'), (TU.LOGISTIC, 'logistic')):
        lib, yard = worst[kind]
        assert lib <= 8.0 * yard, '%s entries: worst normalised error %.3f of the library exceeds 8 x %.3f of the float32 yardstick' % (name, lib, yard)


def test_float64_mirror_reproduces_tempering_of_the_sampler():
    """the identity the feature rests on: the sampler's term of the tempered entry is tau x the term of the entry (inside the clamp)"""
    u = TU.hardest_inputs(1 << 12)
    for tau in (0.1, 0.8, 1.0):
        assert np.allclose(TU.gumbel(TU.temper_kind(u, TU.SELECT, tau)), np.float64(np.float32(tau)) * TU.gumbel(u), rtol=0, atol=1e-9)
        assert np.allclose(TU.logit(TU.temper_kind(u, TU.LOGISTIC, tau)), np.float64(np.float32(tau)) * TU.logit(u), rtol=0, atol=1e-9)


# ---- façade and hparams
def test_hparams_keys_default_to_one():
    import hparams as H
    hp = H._build()
    assert hp.mi355_synthesis_temperature == 1.0 and hp.mi355_synthesis_mixture_temperature == 1.0
    hp.parse('mi355_synthesis_temperature=0.7,mi355_synthesis_mixture_temperature=0.9')
    assert hp.mi355_synthesis_temperature == 0.7 and hp.mi355_synthesis_mixture_temperature == 0.9


def test_temperature_pair_per_head():
    from wavenet_vocoder.models.wavenet import temperature_pair
    mol, gauss, soft = (make_hp(**HEADS[k]) for k in ('mol', 'gauss', 'softmax'))
    assert temperature_pair(mol) == (1.0, 1.0) and temperature_pair(gauss) == (1.0, 1.0) and temperature_pair(soft) == (1.0, 1.0)
    assert temperature_pair(mol, 0.7) == (0.7, 1.0)
    assert temperature_pair(mol, 0.7, 0.9) == (0.7, 0.9)
    assert temperature_pair(mol, None, 0.0) == (1.0, 0.0)
    assert temperature_pair(gauss, 0.7) == (0.7, 1.0)                      # tau_scale of the normal draw
    assert temperature_pair(soft, 0.7) == (1.0, 0.7)                       # the softmax head's only noise is the class choice
    for hp in (gauss, soft):
        with pytest.raises(ValueError):
            temperature_pair(hp, 0.7, 0.9)
        with pytest.raises(ValueError):
            temperature_pair(hp, None, 1.0)
    # None means the hparams value
    mol.set_hparam('mi355_synthesis_temperature', 0.6); mol.set_hparam('mi355_synthesis_mixture_temperature', 0.8)
    assert temperature_pair(mol) == (0.6, 0.8) and temperature_pair(mol, 0.9) == (0.9, 0.8) and temperature_pair(mol, None, 1.0) == (0.6, 1.0)
    soft.set_hparam('mi355_synthesis_temperature', 0.0)
    assert temperature_pair(soft) == (1.0, 0.0)
    gauss.set_hparam('mi355_synthesis_mixture_temperature', 0.8)
    with pytest.raises(ValueError):
        temperature_pair(gauss)


class _Recorder(object):
    """stands in for _ext.Engine: records every call"""
    hop = 16

    def __init__(self):
        self.calls = []

    def stream_lookahead(self):
        return (0, 0)

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call

    def names(self):
        return [c[0] for c in self.calls]


def _model(head, **kw):
    from wavenet_vocoder.models.wavenet import WaveNet
    m = WaveNet(make_hp(**dict(HEADS[head], **kw)))
    m.engine, m._dirty = _Recorder(), False
    return m


def test_slot_session_open_forwards_the_pair():
    m = _model('mol', mi355_synthesis_temperature=0.8)
    sess = m.slots(3)
    sess.open(0, seed=5)
    sess.open(1, seed=6, temperature=0.6, mixture_temperature=0.9)
    sess.open(2, seed=7, mixture_temperature=0.0)
    calls = [c for c in m.engine.calls if c[0] in ('slot_open', 'slot_temperature')]
    assert [c[0] for c in calls] == ['slot_open', 'slot_temperature'] * 3                 # the override follows the open of ITS slot
    assert [c[1] for c in calls if c[0] == 'slot_temperature'] == [(0, 0.8, 1.0), (1, 0.6, 0.9), (2, 0.8, 0.0)]
    g = _model('gauss')
    with pytest.raises(ValueError):
        g.slots(2).open(0, seed=1, mixture_temperature=0.5)
    assert 'slot_open' not in g.engine.names()                                             # rejected before anything reaches the engine


def test_synthesis_stream_forwards_the_pair():
    m = _model('softmax')
    m.stream(2, seed=9, temperature=0.7)
    names = m.engine.names()
    assert ('set_temperature', (1.0, 0.7), {}) in m.engine.calls
    assert names.index('set_temperature') < names.index('stream_begin')
    m = _model('mol', mi355_synthesis_temperature=0.5, mi355_synthesis_mixture_temperature=0.75)
    m.stream(1, seed=9)
    assert ('set_temperature', (0.5, 0.75), {}) in m.engine.calls
    m.stream(1, seed=9, temperature=1.0, mixture_temperature=1.0)
    assert m.engine.calls[-2][:2] == ('set_temperature', (1.0, 1.0)) and m.engine.calls[-1][0] == 'stream_begin'
    with pytest.raises(ValueError):
        _model('softmax').stream(1, seed=1, mixture_temperature=0.5)
