"""Synthesis slots, host side (no GPU): the C ABI names, the pure-Python scheduler slot_plan, and what the plan saves over padded batches on the
committed (synthetic) list of utterance lengths."""
import json
import os
import random
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'wavenet_mi355.h')
SLOT_NAMES = ('wn_synth_slots_begin', 'wn_synth_slot_open', 'wn_synth_slots_push', 'wn_synth_slot_abandon', 'wn_synth_slot_frames_done', 'wn_synth_slots_end')


def test_slot_symbols_declared_and_exported():
    from wavenet_vocoder import _ext
    text = open(HEADER).read()
    declared = set(re.findall(r'\b(wn_synth_slots?_\w+)\s*\(', text))
    assert declared == set(SLOT_NAMES), declared
    syms = _ext.exported_symbols()          # (loading the library resolves every name: a missing export raises here)
    for name in SLOT_NAMES:
        assert name in syms
    assert '#define WN_ABI_VERSION 4' in text


def _replay(lengths, B, tick, right):
    """Run the plan as a session would and check its invariants; returns (pushes, per-utterance generated frame counts per push)."""
    from wavenet_vocoder.models.wavenet import slot_plan, stream_schedule
    owner = [None] * B
    delivered = [0] * len(lengths)
    done = [0] * len(lengths)
    finished = [False] * len(lengths)
    opened_order = []
    freed_last = set()
    pushes = 0
    for opens, frames, final in slot_plan(lengths, B, tick):
        assert len(frames) == B and len(final) == B
        work_left = len(opened_order) < len(lengths)
        for b, u in opens:
            assert owner[b] is None, 'slot %d holds two utterances' % b
            owner[b] = u
            opened_order.append(u)
        # lowest free slot first, input order
        assert [u for _, u in opens] == sorted(u for _, u in opens)
        assert [b for b, _ in opens] == sorted(b for b, _ in opens)
        if work_left:      # a slot freed at push k is refilled at push k + 1 while work remains
            n_new = min(len(freed_last) if pushes else B, len(lengths) - (len(opened_order) - len(opens)))
            assert len(opens) == n_new, (pushes, opens, freed_last)
        freed_last = set()
        for b in range(B):
            u = owner[b]
            if u is None:
                assert frames[b] == 0 and not final[b]
                continue
            assert 0 < frames[b] <= tick
            delivered[u] += frames[b]
            assert delivered[u] <= lengths[u]
            assert bool(final[b]) == (delivered[u] == lengths[u]), 'final exactly on the last delivery'
            first, end = stream_schedule(done[u], delivered[u], right, bool(final[b]))
            assert first == done[u] and end >= first
            done[u] = end
            if final[b]:
                assert not finished[u]
                finished[u] = True
                owner[b] = None
                freed_last.add(b)
        pushes += 1
    assert opened_order == list(range(len(lengths))), 'every utterance once, in input order'
    assert delivered == list(lengths) and done == list(lengths) and all(finished)
    return pushes


@pytest.mark.parametrize('right', [0, 1, 2])
def test_slot_plan_invariants(right):
    rnd = random.Random(1234 + right)
    cases = [([1], 1, 8), ([1, 1, 1], 2, 8), ([5, 1, 2, 30, 1, 9], 4, 3), ([3, 7], 8, 8), ([40, 2, 2, 2, 2], 1, 8)]
    for _ in range(20):
        n = rnd.randint(1, 40)
        cases.append(([rnd.choice([1, 1, 2, rnd.randint(1, 60)]) for _ in range(n)], rnd.choice([1, 2, 5, 12, 20, 32]), rnd.choice([1, 3, 8, 16])))
    for lengths, B, tick in cases:
        pushes = _replay(lengths, B, tick, right)
        assert pushes >= -(-max(lengths) // tick)


def test_slot_plan_rejects_bad_arguments():
    from wavenet_vocoder.models.wavenet import slot_plan
    for args in (([3], 0, 8), ([3], 2, 0), ([3, 0], 2, 8)):
        with pytest.raises(ValueError):
            list(slot_plan(*args))


def test_plan_beats_padded_batches_on_committed_lengths():
    """Wall time per stream, in frames, of today's padded batches (groups of B in input order, each padded to its longest) vs one slot session, on
    the committed SYNTHETIC length list.  Asserted only as plan <= padded; the values are printed."""
    from wavenet_vocoder.models.wavenet import slot_plan
    d = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'slot_lengths.json')))
    assert 'SYNTHETIC' in d['note']
    lengths = d['frames']
    assert len(lengths) == 200 and min(lengths) >= 1
    mean = float(np.mean(lengths))
    for B in (12, 20):
        padded = sum(max(lengths[i:i + B]) for i in range(0, len(lengths), B))
        ideal = sum(lengths) / B
        for tick in (8, 16):
            plan = sum(1 for _ in slot_plan(lengths, B, tick)) * tick
            print('\nB=%d tick=%d: padded %d frames (x%.2f of mean len), plan %d (x%.2f), ideal %.0f; padded / plan = %.2f'
                  % (B, tick, padded, padded / mean, plan, plan / mean, ideal, padded / plan))
            assert plan <= padded
            assert plan >= ideal
