"""Wide slot sessions, host side (no GPU): the C ABI name and its binding, slot_plan at widths beyond 32, the hparam and its exclusion with the
other routes, and the flag of SlotSession that selects the begin call."""
import os
import random
import re

import numpy as np
import pytest

from hip_util import SMALL, make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG = -1
ROUTES = ('mi355_synthesis_fold_rows', 'mi355_synthesis_slots', 'mi355_synthesis_wide_rows')


def test_symbol_declared_exported_and_bound():
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet
    text = open(HEADER).read()
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', text))
    lib = _ext.load_library()
    assert 'wn_synth_wide_slots_begin' in declared
    assert re.search(r'int\s+wn_synth_wide_slots_begin\(wn_ctx\*\s*ctx,\s*int32_t\s+B,\s*int32_t\s+steps_per_graph,\s*void\*\s*stream\);', text)
    assert 'wn_synth_wide_slots_begin' in _ext.exported_symbols() and hasattr(lib, 'wn_synth_wide_slots_begin')
    assert lib.wn_synth_wide_slots_begin.argtypes == lib.wn_synth_slots_begin.argtypes
    assert lib.wn_synth_wide_slots_begin.restype == lib.wn_synth_slots_begin.restype
    assert hasattr(_ext.Engine, 'wide_slots_begin') and hasattr(WaveNet, 'wide_slots')
    assert lib.wn_synth_wide_slots_begin(None, 40, 0, None) == WN_E_ARG


def _check_plan(lengths, B, tick):
    from wavenet_vocoder.models.wavenet import slot_plan
    owner, left, delivered, freed_at = [None] * B, [0] * B, [0] * len(lengths), [None] * B
    nxt = 0
    for k, (opens, frames, final) in enumerate(slot_plan(lengths, B, tick)):
        assert len(frames) == len(final) == B
        for b, u in opens:
            assert owner[b] is None, 'push %d: slot %d is double-booked' % (k, b)
            assert u == nxt, 'utterances are opened in input order'
            if freed_at[b] is not None:
                assert k > freed_at[b], 'slot %d is refilled in the push that ended its utterance' % b
            owner[b], left[b] = u, lengths[u]
            nxt += 1
        for b in range(B):
            if owner[b] is None:
                assert frames[b] == 0 and not final[b]
                if nxt < len(lengths):
                    assert freed_at[b] == k - 1 or k == 0, 'a free slot stayed idle while utterances waited'
                continue
            assert frames[b] == min(tick, left[b]) and frames[b] > 0
            left[b] -= frames[b]
            delivered[owner[b]] += frames[b]
            assert final[b] == (left[b] == 0)
            if final[b]:
                owner[b], freed_at[b] = None, k
    assert nxt == len(lengths) and delivered == list(lengths) and all(o is None for o in owner)      # every utterance delivered exactly once, whole


@pytest.mark.parametrize('B', [33, 70, 1024])
def test_slot_plan_beyond_32_slots(B):
    rnd = random.Random(B)
    for n in (1, B - 1, B, B + 1, 3 * B + 7):
        _check_plan([rnd.randint(1, 40) for _ in range(n)], B, rnd.randint(1, 9))
    _check_plan([1] * (2 * B + 1), B, 8)                     # every slot is refilled on every push
    _check_plan([5] * B, B, 5)                               # one push, all final
    _check_plan([100], B, 8)                                 # one slot busy, the rest idle throughout
    _check_plan([], B, 8)
    first = json_lengths()[:100]
    _check_plan(first, B, 8)


def json_lengths():
    import json
    return [int(v) for v in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'slot_lengths.json')))['frames']]


def test_hparam_defaults_to_off_and_is_a_route():
    import hparams as H
    hp = H._build()
    assert hp.mi355_synthesis_wide_slots == 0
    hp.parse('mi355_synthesis_wide_slots=256')
    assert hp.mi355_synthesis_wide_slots == 256


@pytest.mark.parametrize('other', ROUTES + (ROUTES[:2],))
def test_synthesizer_refuses_the_route_with_another(tmp_path, other):
    from wavenet_vocoder.synthesizer import Synthesizer
    on = (other if isinstance(other, tuple) else (other,)) + ('mi355_synthesis_wide_slots',)
    hp = make_hp(**dict(SMALL, **{k: 4 for k in on}))
    s = Synthesizer()
    s.load(None, hp)
    with pytest.raises(ValueError) as ei:
        s.synthesize([np.zeros((10, 16), np.float32)], None, ['a'], str(tmp_path), None)
    assert all(k in str(ei.value) for k in on) and 'choose one' in str(ei.value) and s.model.engine is None
    assert ('both' in str(ei.value)) == (len(on) == 2)


class _StubEngine(object):
    hop = 16

    def __init__(self):
        self.calls = []

    def stream_lookahead(self):
        return (0, 0)

    def slots_begin(self, B, steps_per_graph=0):
        self.calls.append(('slots_begin', B, steps_per_graph))

    def wide_slots_begin(self, B, steps_per_graph=0):
        self.calls.append(('wide_slots_begin', B, steps_per_graph))

    def slots_end(self):
        self.calls.append(('slots_end',))


class _StubModel(object):
    def __init__(self):
        self.engine = _StubEngine()

    def _ensure_packed(self):
        pass


def test_slot_session_flag_selects_the_begin_call():
    from wavenet_vocoder.models.wavenet import SlotSession
    m = _StubModel()
    s = SlotSession(m, 70, steps_per_graph=24, wide=True)
    assert s.wide and s.B == 70 and m.engine.calls == [('wide_slots_begin', 70, 24)]
    s.close()
    m = _StubModel()
    s = SlotSession(m, 8, steps_per_graph=0)
    assert not s.wide and m.engine.calls == [('slots_begin', 8, 0)]
    s.close()
    assert m.engine.calls[-1] == ('slots_end',)


def test_facade_slots_keeps_its_limit():
    """WaveNet.slots goes through wn_synth_slots_begin, whose limit of 32 slots and message are unchanged; without an engine it raises as before."""
    from wavenet_vocoder.models.wavenet import WaveNet
    model = WaveNet(make_hp(**SMALL))
    with pytest.raises(RuntimeError, match=r'WaveNet\.slots: call build\(\) / initialize\(\) first'):
        model.slots(33)
    with pytest.raises(RuntimeError, match=r'WaveNet\.wide_slots: call build\(\) / initialize\(\) first'):
        model.wide_slots(33)
    src = open(os.path.join(ROOT, 'tacotron-2_amd', 'csrc', 'wn_api.hip')).read()
    assert 'slot count %d outside (0, min(32, max_batch = %d)]' in src
