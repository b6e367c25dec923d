"""Held-out validation, host side (no GPU): the two C-ABI entry points, Feeder.validation_batches on an on-disk .npy data set, the
aggregation of per-utterance score rows into the loss, the all-reduce of the totals on two gloo ranks, and the hparam that turns it on."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 16


def test_validation_symbols_are_declared_and_exported():
    sys.path.insert(0, os.path.join(ROOT, 'tacotron-2_amd', 'csrc'))
    import build as B
    B.build(verbose=False)
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    header = open(os.path.join(ROOT, 'include', 'wavenet_mi355.h')).read()
    assert re.search(r'#define\s+WN_ABI_VERSION\s+4\b', header) and _ext.WN_ABI_VERSION == 4      # functions only: the ABI version stays
    for sym in ('wn_eval_fwd', 'wn_score'):
        assert re.search(r'\bint\s+%s\s*\(' % sym, header), '%s is not declared in include/wavenet_mi355.h' % sym
        assert hasattr(lib, sym) and sym in _ext.exported_symbols()
    null, buf = ctypes.c_void_p(0), ctypes.c_void_p(1)          # a NULL context is refused before anything is dereferenced
    assert lib.wn_eval_fwd(null, buf, buf, buf, buf, 1, 32, 2, buf, null, null, null) == -1       # WN_E_ARG
    assert lib.wn_score(null, buf, buf, buf, 1, 32, 1, buf, null, null) == -1


def test_validation_interval_defaults_to_off():
    import hparams as H
    assert H._build().mi355_validation_interval == 0
    assert H._build().parse('mi355_validation_interval=500').mi355_validation_interval == 500


# ---- Feeder.validation_batches ------------------------------------------------------------------------------------------------------
FRAMES = [20, 45, 12, 31, 60, 8, 25]          # utterances 1 and 4 are longer than max_time_steps = 512 (32 frames)


def _dataset(tmp):
    rng = np.random.RandomState(3)
    os.makedirs(os.path.join(tmp, 'audio')); os.makedirs(os.path.join(tmp, 'mels'))
    lines = []
    for i, frames in enumerate(FRAMES):
        wav = rng.uniform(-0.9, 0.9, size=frames * HOP).astype(np.float32)
        mel = rng.uniform(-4, 4, size=(frames, 16)).astype(np.float32)
        a, m = os.path.join(tmp, 'audio', 'audio-%03d.npy' % i), os.path.join(tmp, 'mels', 'mel-%03d.npy' % i)
        np.save(a, wav); np.save(m, mel)
        lines.append('|'.join([a, m, m, '<no_g>', 'text %d' % i]))
    meta = os.path.join(tmp, 'map.txt')
    with open(meta, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    return meta


def _hp():
    import hparams as H
    return H._build().parse('hop_size=16,num_mels=16,cin_channels=16,upsample_scales=[4,4],max_time_steps=512,wavenet_batch_size=2,'
                            'wavenet_test_size=2,wavenet_test_batches=1')


def _feeder(meta, tmp):
    from wavenet_vocoder.feeder import Feeder
    return Feeder(None, meta, tmp, _hp(), device=torch.device('cpu'))


def _same(a, b):
    return len(a) == len(b) and all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))


def test_validation_batches_cover_every_utterance_once_with_fixed_crops(tmp_path):
    meta = _dataset(str(tmp_path))
    fd = _feeder(meta, str(tmp_path))
    batches = list(fd.validation_batches('all'))
    assert [int(b[2].shape[0]) for b in batches] == [2, 2, 2, 1]                      # the last batch is smaller
    wavs = [np.load(os.path.join(str(tmp_path), 'audio', 'audio-%03d.npy' % i)) for i in range(7)]
    mels = [np.load(os.path.join(str(tmp_path), 'mels', 'mel-%03d.npy' % i)) for i in range(7)]
    seen = 0
    for bi, (x, y, lengths, c, g) in enumerate(batches):
        B, T = int(lengths.shape[0]), int(x.shape[-1])
        assert x.shape == (B, 1, T) and y.shape == (B, T, 1) and c.shape == (B, 16, T // HOP) and g is None and lengths.dtype == torch.int32
        assert T == int(lengths.max()) and T % HOP == 0 and T <= 512
        for j in range(B):
            i = 2 * bi + j                                                           # metadata order, every utterance exactly once
            n = int(lengths[j])
            assert n == min(FRAMES[i] * HOP, 512) and n % HOP == 0
            got = x[j, 0, :n].numpy()
            if FRAMES[i] * HOP > 512:                                                # a hop-aligned crop whose start depends on the utterance alone
                s = int(np.random.RandomState(_hp().wavenet_data_random_state + i).randint(0, FRAMES[i] - 32))
                assert np.array_equal(got, wavs[i][s * HOP:s * HOP + n])
                mel = mels[i][s:s + 32]
            else:
                assert np.array_equal(got, wavs[i])
                mel = mels[i]
            assert np.array_equal(y[j, :n, 0].numpy(), got)
            assert np.allclose(c[j, :, :n // HOP].numpy(), ((mel + 4.0) / 8.0).T, atol=1e-6)      # clip + [0, 1] normalisation as the training batches
            seen += 1
    assert seen == 7
    again = list(fd.validation_batches('all'))                                        # identical at every validation ...
    other = list(_feeder(meta, str(tmp_path)).validation_batches('all'))              # ... and in every run
    assert all(_same(a, b) for a, b in zip(batches, again)) and all(_same(a, b) for a, b in zip(batches, other))
    # the held-out split: the rows train_test_split set aside, in metadata order
    test = list(fd.validation_batches())
    rows = [r for grp in fd.validation_utterances() for r, _ in grp]
    assert rows == sorted(fd._test_indices) and len(rows) == 2 and [int(b[2].shape[0]) for b in test] == [2]
    assert [int(v) for v in test[0][2]] == [min(FRAMES[r] * HOP, 512) for r in rows]
    with pytest.raises(ValueError):
        list(fd.validation_batches('train'))


def test_validation_batches_rank_slices_are_disjoint_and_complete(tmp_path, monkeypatch):
    from wavenet_vocoder import feeder as F
    meta = _dataset(str(tmp_path))
    rows = {}
    for r in range(2):
        monkeypatch.setattr(F, '_ranks', lambda r=r: (r, 2))
        fd = F.Feeder(None, meta, str(tmp_path), _hp(), device=torch.device('cpu'))
        rows[r] = [i for grp in fd.validation_utterances('all') for i, _ in grp]
        assert [int(b[2].shape[0]) for b in fd.validation_batches('all')] == [1] * len(rows[r])
    assert rows[0] == [0, 2, 4, 6] and rows[1] == [1, 3, 5]


def test_validation_passes_do_not_move_the_training_or_eval_batches(tmp_path):
    meta = _dataset(str(tmp_path))

    def draw(validate):
        fd = _feeder(meta, str(tmp_path))
        out = []
        for k in range(3):                        # the producer's own code path, synchronously: offsets, shuffles and crop generators advance here
            group = fd._next_group(train=True)
            out += [fd._prepare_batch(b) for b in group[:3]]
            out.append(fd._prepare_batch(fd._next_group(train=False)[0]))
            if validate and k < 2:
                assert sum(int(b[2].shape[0]) for b in fd.validation_batches('all')) == 7
        return fd, out
    fa, a = draw(True)
    fb, b = draw(False)
    assert len(a) == len(b) == 12
    for u, v in zip(a, b):
        assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(u, v))
    assert (fa._train_offset, fa._test_offset) == (fb._train_offset, fb._test_offset)
    assert fa._train_q.empty() and fa._eval_q.empty()
    assert np.array_equal(fa._rng.get_state()[1], fb._rng.get_state()[1]) and np.array_equal(fa._order_rng.get_state()[1], fb._order_rng.get_state()[1])


# ---- aggregation ----------------------------------------------------------------------------------------------------------------------
def test_validation_summary_uses_the_training_definition_of_the_loss():
    from wavenet_vocoder.models.wavenet import validation_summary
    rows = [(120.5, 40.0, 40.0), (0.0, 0.0, 0.0), (-30.25, 25.0, 25.0), (64.0, 16.0, 10.0)]
    s = validation_summary(rows, quantized=False)
    assert s['count'] == 81 and s['nonzero'] == 75 and abs(s['sum'] - 154.25) < 1e-12
    assert abs(s['loss'] - 154.25 / 81) < 1e-12                                       # scalar heads: mean over the counted samples
    assert s['utterances'] == [(120.5, 40, 40), (0.0, 0, 0), (-30.25, 25, 25), (64.0, 16, 10)]
    q = validation_summary(rows, quantized=True)
    assert abs(q['loss'] - 154.25 / 75) < 1e-12                                       # softmax head: over the samples with a non-zero loss (modules.py:798)
    assert validation_summary(rows[:1] + rows[2:], False)['loss'] == s['loss']        # a row without a counted sample changes nothing
    empty = validation_summary([(0.0, 0.0, 0.0)], False)
    assert np.isnan(empty['loss']) and empty['count'] == 0 and validation_summary([], True)['utterances'] == []


def test_validation_totals_without_a_process_group_come_back_unchanged():
    from wavenet_vocoder.parallel import allreduce_validation_totals, validation_loss
    assert allreduce_validation_totals((1.5, 4, 3)) == (1.5, 4.0, 3.0)
    assert validation_loss(6.0, 4, 3, False) == 1.5 and validation_loss(6.0, 4, 3, True) == 2.0 and np.isnan(validation_loss(0.0, 0, 0, True))


_REDUCE_WORKER = r'''
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + '/tacotron-2_amd')
import torch.distributed as dist
from wavenet_vocoder.parallel import allreduce_validation_totals, validation_loss
rank = int(sys.argv[1])
dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%(port)d', rank=rank, world_size=2)
mine = [(1234.5678901234, 16777217, 16777216, 3), (-0.25, 5, 4, 1)][rank]
tot = allreduce_validation_totals(mine)
assert tot == (1234.5678901234 - 0.25, 16777222.0, 16777220.0, 4.0), tot          # fp64: exact beyond 2^24 samples
assert abs(validation_loss(*tot[:3], False) - tot[0] / 16777222.0) < 1e-15 and abs(validation_loss(*tot[:3], True) - tot[0] / 16777220.0) < 1e-15
dist.barrier(); dist.destroy_process_group()
print('rank ok')
'''


def test_validation_totals_allreduce_gloo(tmp_path):
    port = 37500 + (os.getpid() % 2000)
    script = tmp_path / 'validation_reduce_worker.py'
    script.write_text(_REDUCE_WORKER % {'root': ROOT, 'port': port})
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and 'rank ok' in o, o[-2000:]
