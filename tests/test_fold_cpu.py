"""Folded synthesis, host side (no GPU): the C ABI names, the planner (wn_fold_plan through ctypes) against every rule of the header, the fade tables,
the numpy mirror of the unfold (tests/fold_util.py, which tests/test_hip_fold.py holds the device kernel to), and the rejections of a plan through the
façade against a recording stand-in engine."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import fold_util as FU
from hip_util import make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
NAMES = ('wn_fold_plan', 'wn_fold_check', 'wn_fold_weights', 'wn_synthesize_folded')
WN_E_ARG, WN_E_SHAPE = -1, -2


def test_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    for name in NAMES:
        assert name in declared, name
        assert name in _ext.exported_symbols()
        assert hasattr(lib, name)
    assert 'typedef struct wn_fold_row { int32_t utt, first, frames, keep, fade; } wn_fold_row;' in text
    assert ctypes.sizeof(_ext.WnFoldRow) == 20
    assert hasattr(_ext.Engine, 'synthesize_folded') and callable(_ext.fold_plan)


def _random_case(rnd):
    U = rnd.randint(1, 6)
    frames = [rnd.randint(1, 900) for _ in range(U)]
    return frames, rnd.randint(U, 32), rnd.randint(0, 8), rnd.randint(0, 4), rnd.choice([1, 2, 3, 5, 17, 40, 100, 400])


def test_random_plans_obey_every_rule_and_cover_every_frame_once():
    from wavenet_vocoder import _ext
    rnd = random.Random(7)
    split = 0
    for case in range(600):
        frames, rows_max, warm, fade, min_keep = _random_case(rnd)
        plan = _ext.fold_plan(frames, rows_max, warm, fade, min_keep)
        assert len(frames) <= len(plan) <= rows_max, (case, frames, rows_max, plan)
        FU.check_rules(frames, plan)
        _ext.fold_check(frames, plan)                                  # the library's own validation accepts what its planner makes
        for got, want in zip(FU.coverage(frames, plan), FU.expected_coverage(frames, plan)):
            assert np.array_equal(got, want), (case, frames, plan)    # once outside the fades, by exactly two rows inside them
        for u, F in enumerate(frames):
            rows = [r for r in plan if r[0] == u]
            k = len(rows)
            if F < 2 * min_keep:
                assert k == 1 and rows[0] == (u, 0, F, 0, 0), (case, F, min_keep, rows)
            assert k == 1 or F // k >= min_keep, (case, F, k, min_keep)
            for j, (_, first, n, keep, fd) in enumerate(rows):          # the boundaries a_j = floor(j F / k), warm-up and fade as asked where they fit
                assert keep == j * F // k and first == max(0, keep - warm)
                assert fd == (0 if j == 0 else min(fade, (j + 1) * F // k - keep))
            split += k > 1
        # the remaining rows go to the longest rows first: no utterance that could still be split has rows longer than another's rows would become
        ks = [sum(1 for r in plan if r[0] == u) for u in range(len(frames))]
        if len(plan) < rows_max:
            assert all(F // (k + 1) < min_keep for F, k in zip(frames, ks)), (case, frames, ks, min_keep)
    assert split > 300


def test_planner_gives_rows_to_the_longest_and_breaks_ties_low():
    from wavenet_vocoder import _ext
    assert _ext.fold_plan([401], 12, 4, 2, 4) [1] == (0, 33 - 4, 4 + (66 - 33) + 2, 33, 2)
    assert len(_ext.fold_plan([401], 12, 4, 2, 40)) == 10              # 401 // 11 = 36 < 40: ten rows of >= 40 new frames
    assert _ext.fold_plan([79], 12) == [(0, 0, 79, 0, 0)]                # shorter than 2 * min_keep: the one-shot run
    ks = lambda plan, U: [sum(1 for r in plan if r[0] == u) for u in range(U)]
    assert ks(_ext.fold_plan([100, 100, 100], 5, 1, 1, 10), 3) == [2, 2, 1]      # ties: the lowest index
    assert ks(_ext.fold_plan([100, 300], 4, 1, 1, 10), 2) == [1, 3]
    assert ks(_ext.fold_plan([37, 9], 5, 1, 1, 4), 2) == [4, 1]                    # 9 // 2 == 4: a split would be allowed, but 37 / k stays longer


def test_planner_is_deterministic():
    from wavenet_vocoder import _ext
    rnd = random.Random(11)
    for _ in range(50):
        case = _random_case(rnd)
        assert _ext.fold_plan(*case) == _ext.fold_plan(*case)


def test_planner_rejects_bad_arguments():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()

    def code(*a):
        with pytest.raises(_ext.WnError) as ei:
            _ext.fold_plan(*a)
        return ei.value.code

    assert code([10, 0], 4) == WN_E_ARG and code([10], 4, -1) == WN_E_ARG and code([10], 4, 1, -1) == WN_E_ARG and code([10], 4, 1, 1, 0) == WN_E_ARG
    assert code([], 4) == WN_E_ARG
    assert code([10, 10], 1) == WN_E_SHAPE and code([10], 33) == WN_E_SHAPE
    uf = (ctypes.c_int32 * 1)(400)
    rows = (_ext.WnFoldRow * 32)()
    assert lib.wn_fold_plan(uf, 1, 8, 1, 1, 10, rows, 7) == WN_E_SHAPE           # cap too small
    assert lib.wn_fold_plan(uf, 1, 8, 1, 1, 10, rows, 8) == 8
    assert lib.wn_fold_plan(None, 1, 8, 1, 1, 10, rows, 8) == WN_E_ARG and lib.wn_fold_plan(uf, 1, 8, 1, 1, 10, None, 8) == WN_E_ARG
    assert lib.wn_synthesize_folded(None, None, uf, 1, rows, 1, 0, None, None, 0, None, None, 0, None, None, 0, 0, None) == WN_E_ARG


@pytest.mark.parametrize('kind', ['equal_power', 'linear'])
def test_fade_tables(kind):
    """the library's tables equal the float64 formulas rounded to float32, and keep power (equal power) / amplitude (linear) to float32 rounding"""
    from wavenet_vocoder import _ext
    eps = float(np.finfo(np.float32).eps)
    for n in (1, 2, 15, 16, 550, 1100):
        w_in, w_out = _ext.fold_weights(kind, n)
        r_in, r_out = FU.weights(kind, n)
        if kind == 'linear':
            assert np.array_equal(w_in, r_in) and np.array_equal(w_out, r_out)
            assert np.abs(w_in.astype(np.float64) + w_out.astype(np.float64) - 1.0).max() <= eps          # two roundings of values <= 1: half an ulp of 1 each
        else:
            # libm's double sin / cos are within an ulp of double: after rounding to float32 at most the last float32 bit can differ from numpy's
            assert np.abs(w_in.view(np.int32) - r_in.view(np.int32)).max() <= 1 and np.abs(w_out.view(np.int32) - r_out.view(np.int32)).max() <= 1
            assert np.abs(w_in.astype(np.float64) ** 2 + w_out.astype(np.float64) ** 2 - 1.0).max() <= 2 * eps
        assert w_in.min() > 0 and w_out.min() > 0 and w_in.max() < 1 and w_out.max() < 1
    lib = _ext.load_library()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.wn_fold_weights(0, 0, p, p) == WN_E_ARG and lib.wn_fold_weights(2, 4, p, p) == WN_E_ARG and lib.wn_fold_weights(0, 4, None, p) == WN_E_ARG


@pytest.mark.parametrize('kind', ['equal_power', 'linear'])
def test_unfold_mirror_on_rows_cut_from_one_signal(kind):
    """Rows that are slices of ONE signal (what a folded run would give if a cold start changed nothing): the mirror returns the signal itself outside the
    fades, bit for bit, and a (w_out + w_in) multiple of it inside them -- the signal to float32 rounding for the linear fade."""
    from wavenet_vocoder import _ext
    hop = 16
    rng = np.random.RandomState(5)
    frames = [37, 9, 64]
    plan = _ext.fold_plan(frames, 9, 1, 2, 4)
    assert len(plan) == 9
    sig = [rng.uniform(-1, 1, F * hop).astype(np.float32) for F in frames]
    n_max = max(r[2] for r in plan) * hop
    rows = np.full((len(plan), n_max + 3), np.nan, np.float32)
    for i, (u, first, n, _, _) in enumerate(plan):
        rows[i, :n * hop] = sig[u][first * hop:(first + n) * hop]
    wavs = FU.unfold(frames, plan, hop, rows, kind)
    infade = [np.repeat(c == 2, hop) for c in FU.expected_coverage(frames, plan)]
    for u, w in enumerate(wavs):
        assert w.shape == sig[u].shape and np.isfinite(w).all()
        assert np.array_equal(w[~infade[u]], sig[u][~infade[u]])
        assert infade[u].sum() == sum(r[4] for r in plan if r[0] == u) * hop
        if not infade[u].any():
            assert len([r for r in plan if r[0] == u]) == 1                                  # (the 9-frame utterance stays one row)
        elif kind == 'linear':
            assert np.abs(w[infade[u]] - sig[u][infade[u]]).max() <= 2 * np.finfo(np.float32).eps
        else:
            gain = np.abs(w[infade[u]]) / np.maximum(np.abs(sig[u][infade[u]]), 1e-30)
            assert gain.max() <= np.sqrt(2) * (1 + 1e-6) and gain.min() >= 1 - 1e-6        # coherent rows under an equal-power fade: up to + 3 dB


# ---- façade and hparams
def test_hparams_keys_and_defaults():
    import hparams as H
    hp = H._build()
    assert (hp.mi355_synthesis_fold_rows, hp.mi355_synthesis_fold_warm, hp.mi355_synthesis_fold_fade, hp.mi355_synthesis_fold_min_frames) == (0, 4, 2, 40)
    hp.parse('mi355_synthesis_fold_rows=12,mi355_synthesis_fold_warm=3')
    assert hp.mi355_synthesis_fold_rows == 12 and hp.mi355_synthesis_fold_warm == 3


class _Recorder(object):
    """stands in for _ext.Engine: records every call"""
    hop = 16

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a, **k):
            self.calls.append((name, a, k))
        return call


def _model(**kw):
    from wavenet_vocoder.models.wavenet import WaveNet
    from hip_util import SMALL
    m = WaveNet(make_hp(**dict(SMALL, **kw)))
    m.engine, m._dirty = _Recorder(), False
    return m


GOOD = [(0, 0, 13, 0, 0), (0, 11, 14, 12, 1), (0, 23, 14, 24, 1), (1, 0, 9, 0, 0)]            # utterances of 37 and 9 frames
BAD = {      # name -> (plan, what the message must name)
    'first row of an utterance starts late': ([(0, 1, 12, 1, 0)] + GOOD[1:], 'row 0'),
    'first row of an utterance fades': ([(0, 0, 13, 0, 1)] + GOOD[1:], 'row 0'),
    'last row stops short': (GOOD[:2] + [(0, 23, 13, 24, 1), GOOD[3]], 'row 2'),
    'last row of the last utterance stops short': (GOOD[:3] + [(1, 0, 8, 0, 0)], 'row 3'),
    'row runs past its utterance': (GOOD[:2] + [(0, 23, 15, 24, 1), GOOD[3]], 'row 2'),
    'seam does not meet the previous end': ([GOOD[0], (0, 11, 14, 12, 2)] + GOOD[2:], 'row 1'),
    'keep inside the previous fade': ([(0, 0, 13, 0, 0), (0, 8, 11, 10, 3), (0, 9, 28, 11, 8), GOOD[3]], 'row 2'),
    'keep before first': ([GOOD[0], (0, 12, 13, 11, 2)] + GOOD[2:], 'row 1'),
    'fade beyond the row': ([GOOD[0], (0, 11, 1, 11, 2)] + GOOD[2:], 'row 1'),
    'no frames': ([GOOD[0], (0, 12, 0, 12, 0)] + GOOD[2:], 'row 1'),
    'negative fade': ([GOOD[0], (0, 11, 14, 14, -1)] + GOOD[2:], 'row 1'),
    'negative first': ([(0, -1, 14, 0, 0)] + GOOD[1:], 'row 0'),
    'rows not sorted by utterance': ([GOOD[3], GOOD[0], GOOD[1], GOOD[2]], 'row 0'),
    'utterance without a row': (GOOD[:3], 'utterance 1'),
    'utterance index out of range': (GOOD + [(2, 0, 9, 0, 0)], 'row 4'),
    'utterance skipped': ([(0, 0, 37, 0, 0), (2, 0, 9, 0, 0)], 'row 1'),
}


def test_good_plan_passes_the_library_check():
    from wavenet_vocoder import _ext
    FU.check_rules([37, 9], GOOD)
    _ext.fold_check([37, 9], GOOD)


@pytest.mark.parametrize('name', sorted(BAD))
def test_facade_rejects_a_plan_that_breaks_a_rule(name):
    """every rejection of wn_synthesize_folded's validation (wn_fold_check, the function the device entry calls) reaches the caller of WaveNet.folded as a
    ValueError naming the row, before anything reaches the engine"""
    import torch
    from wavenet_vocoder import _ext
    plan, where = BAD[name]
    with pytest.raises(AssertionError):
        FU.check_rules([37, 9], plan)                                            # the mirror of the rules agrees that the plan is bad
    with pytest.raises(_ext.WnError) as ei:
        _ext.fold_check([37, 9], plan)
    assert ei.value.code == WN_E_ARG and where in str(ei.value), str(ei.value)
    m = _model()
    with pytest.raises(ValueError) as ev:
        m.folded([torch.zeros(16, 37), torch.zeros(16, 9)], rows=plan)
    assert where in str(ev.value)
    assert m.engine.calls == []


def test_facade_rejects_bad_arguments_before_the_engine():
    import torch
    m = _model()
    c = [torch.zeros(16, 37), torch.zeros(16, 9)]
    for kw in (dict(rows=1), dict(rows=33), dict(rows=[GOOD[0]] * 33), dict(fade_kind='cosine'), dict(warm=-1), dict(fade=-1), dict(min_keep=0),
               dict(test_inputs=[torch.zeros(37 * 16)])):
        with pytest.raises(ValueError):
            m.folded(c, **kw)
    for bad in ([], [torch.zeros(16, 0)], [torch.zeros(8, 5)], [torch.zeros(1, 16, 5)]):
        with pytest.raises(ValueError):
            m.folded(bad)
    with pytest.raises(ValueError):
        _model(out_channels=2).folded(c, mixture_temperature=0.5)
    with pytest.raises(ValueError):
        _model(gin_channels=8, use_speaker_embedding=False).folded(c)               # global conditioning without g
    assert m.engine.calls == []


def test_synthesizer_refuses_folding_and_slots_together(tmp_path):
    from wavenet_vocoder.synthesizer import Synthesizer
    from hip_util import SMALL
    hp = make_hp(**dict(SMALL, mi355_synthesis_fold_rows=4, mi355_synthesis_slots=4))
    s = Synthesizer()
    s.load(None, hp)
    with pytest.raises(ValueError) as ei:
        s.synthesize([np.zeros((10, 16), np.float32)], None, ['a'], str(tmp_path), None)
    assert 'mi355_synthesis_slots' in str(ei.value) and s.model.engine is None


def test_fold_capacity_and_feature_reassembly():
    import torch
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import fold_capacity, unfold_features
    frames, hop = [37, 9, 37], 16
    plan = _ext.fold_plan(frames, 7, 1, 1, 4)
    B, T = fold_capacity(frames, plan, hop)
    n_max = max(r[2] for r in plan) * hop
    assert B == len(plan) == 7 and T >= n_max and B * T >= 2 * 37 * hop                # the two 37-frame utterances are upsampled together
    whole = [torch.arange(F * hop, dtype=torch.float32).repeat(2, 1) + 1000 * u for u, F in enumerate(frames)]
    feats = torch.full((len(plan), 2, n_max), -1.0)
    for i, (u, first, n, _, _) in enumerate(plan):
        feats[i, :, :n * hop] = whole[u][:, first * hop:(first + n) * hop]
    for got, want in zip(unfold_features(plan, feats, hop), whole):
        assert torch.equal(got, want)
