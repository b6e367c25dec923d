"""Wide synthesis, host side (no GPU): the C ABI name, the hparam and its exclusion with the slot and fold routes, and the planner wide_plan."""
import os
import random
import re

import numpy as np
import pytest

from hip_util import SMALL, make_hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
WN_E_ARG = -1


def test_symbol_declared_exported_and_bound():
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet
    declared = set(re.findall(r'\bint\s+(wn_\w+)\s*\(', open(HEADER).read()))
    lib = _ext.load_library()
    assert 'wn_synthesize_wide' in declared
    assert 'wn_synthesize_wide' in _ext.exported_symbols() and hasattr(lib, 'wn_synthesize_wide')
    assert lib.wn_synthesize_wide.argtypes == lib.wn_synthesize.argtypes
    assert hasattr(_ext.Engine, 'synthesize_wide') and hasattr(WaveNet, 'wide')
    assert '#define WN_ABI_VERSION 4' in open(HEADER).read()


def test_null_context_is_an_argument_error():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    assert lib.wn_synthesize_wide(None, None, 40, 4, None, 0, None, None, None, 0, None) == WN_E_ARG


def test_hparam_defaults_to_off():
    import hparams as H
    hp = H._build()
    assert hp.mi355_synthesis_wide_rows == 0
    hp.parse('mi355_synthesis_wide_rows=64')
    assert hp.mi355_synthesis_wide_rows == 64


@pytest.mark.parametrize('on', [('mi355_synthesis_wide_rows', 'mi355_synthesis_slots'), ('mi355_synthesis_wide_rows', 'mi355_synthesis_fold_rows'),
                                ('mi355_synthesis_wide_rows', 'mi355_synthesis_slots', 'mi355_synthesis_fold_rows')])
def test_synthesizer_refuses_two_routes_together(tmp_path, on):
    from wavenet_vocoder.synthesizer import Synthesizer
    hp = make_hp(**dict(SMALL, **{k: 4 for k in on}))
    s = Synthesizer()
    s.load(None, hp)
    with pytest.raises(ValueError) as ei:
        s.synthesize([np.zeros((10, 16), np.float32)], None, ['a'], str(tmp_path), None)
    assert all(k in str(ei.value) for k in on) and 'choose one' in str(ei.value) and s.model.engine is None


def _check_plan(frames, rows, max_cells):
    from wavenet_vocoder.models.wavenet import wide_plan, wide_padded_cells
    runs, perm = wide_plan(frames, rows, max_cells)
    flat = [u for r in runs for u in r]
    assert sorted(flat) == list(range(len(frames))), (frames, rows, runs)                        # every utterance exactly once
    assert [flat[perm[i]] for i in range(len(frames))] == list(range(len(frames)))               # the permutation restores the input order
    for r in runs:
        longest = max(frames[u] for u in r)
        assert 1 <= len(r) <= rows and len(r) * longest <= max_cells, (frames, rows, max_cells, r)
        assert frames[r[0]] == longest                                                          # padded to its own longest only: the first of the run
    lens = [frames[u] for u in flat]
    assert lens == sorted(lens, reverse=True)                                                   # longest first ...
    for a, b in zip(flat, flat[1:]):
        assert frames[a] > frames[b] or a < b                                                   # ... and stable
    arrival = [list(range(i, min(i + rows, len(frames)))) for i in range(0, len(frames), rows)]
    assert wide_padded_cells(frames, runs) <= wide_padded_cells(frames, arrival), (frames, rows, max_cells)
    return runs


def test_random_plans():
    rnd = random.Random(11)
    cut = 0
    for _ in range(200):
        n = rnd.randint(1, 90)
        frames = [rnd.choice([rnd.randint(1, 30), rnd.randint(1, 900)]) for _ in range(n)]
        rows = rnd.randint(1, 80)
        max_cells = max(frames) * rnd.randint(1, rows)
        runs = _check_plan(frames, rows, max_cells)
        cut += any(len(r) < rows and (len(r) + 1) * max(frames[u] for u in r) > max_cells for r in runs[:-1])
    assert cut > 20                                                                              # the cell bound, not only `rows`, cut some plans


def test_degenerate_plans():
    from wavenet_vocoder.models.wavenet import wide_plan
    assert _check_plan([7], 64, 64 * 7) == [[0]]
    assert _check_plan([3, 9, 5], 1, 1000) == [[1], [2], [0]]
    assert _check_plan([6] * 70, 64, 64 * 6) == [list(range(64)), list(range(64, 70))]
    assert _check_plan([5, 40, 5], 64, 40) == [[1], [0, 2]]                                      # the longest fills a run alone
    with pytest.raises(ValueError) as ei:
        wide_plan([5, 41, 5], 64, 40)                                                            # one utterance longer than max_cells / 1
    assert 'utterance 1' in str(ei.value)
    for bad in (dict(frames=[5], rows=0, max_cells=10), dict(frames=[5], rows=4, max_cells=0), dict(frames=[0], rows=4, max_cells=10)):
        with pytest.raises(ValueError):
            wide_plan(**bad)
