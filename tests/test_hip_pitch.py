"""Pitch check on the device (csrc/wn_pitch.hip): every element of d' from wn_pitch_run against the float64 reference of tests/pitch_ref.py inside the bound
beta, tau*, the voiced flag and f0 on every decidable frame, and d', f0, ap against the host hook bit for bit, over three geometries -- A (2000 Hz, hop 16,
W 64, lags 5 ... 40), P (the production geometry on signals below 0.3 s: lags 44 ... 368 are a stride loop with a partial last pass) and M (6400 Hz, hop 32,
W 128, lags 8 ... 128) -- and ragged batches whose row lengths sit at 0, 1, hop - 1, hop, hop + 1, L - 1, L and around the multiples of the frame tile,
with a pitch beyond the longest row, NaN beyond every row's length and a sentinel in the output cells beyond a row's frames; the comparison against its
hook and against float64; the invariance of a row's bits; and the drivers on a tiny model.  WN_PITCH_PARITY_OUT=<file> makes the session write the worst
d' error / bound per geometry there (profiles/pitch_parity.json is such a file)."""
import io
import json
import os

import numpy as np
import pytest
import torch

import pitch_ref as PR

pytestmark = pytest.mark.gpu
PARITY = {}
SENTINEL = -7.25
NAMES = ['A', 'P', 'M']


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    yield
    path = os.environ.get('WN_PITCH_PARITY_OUT')
    if path and PARITY:
        with open(path, 'w') as f:
            json.dump({'what': "wn_pitch_run on an MI355X against the float64 reference of tests/pitch_ref.py: worst |d' - ref| / (beta |ref|) over every element, the frames of "
                               'the case and how many of them the decidability test excused, of tests/test_hip_pitch.py::test_device_against_float64_and_the_hook',
                       'geometries': PARITY}, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _tracker(name, rows, max_samples):
    from wavenet_vocoder import _ext
    return _ext.PitchTracker(dict(PR.GEOMETRIES[name]), rows, max_samples)


def _run(trk, wav, lengths, frames=None, dprime=True):
    """one run into sentinel-filled outputs -> numpy (f0, ap[, dprime])"""
    B = len(lengths)
    F = frames if frames is not None else max(1 + n // trk.hop for n in lengths)
    out = (torch.full((B, F), SENTINEL, device='cuda'), torch.full((B, F), SENTINEL, device='cuda')) + ((torch.full((B, F, trk.tau_max + 1), SENTINEL, device='cuda'),) if dprime else ())
    trk.run(_dev(wav), lengths, return_dprime=dprime, frames=F, out=out)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize('name', NAMES)
def test_device_against_float64_and_the_hook(name):
    from wavenet_vocoder import _ext
    geo, lengths, rows, refs = PR.case(name)
    trk = _tracker(name, len(rows), max(lengths) + 3 * geo['hop'])                                    # capacity for F_max two frames beyond the longest row
    assert trk.frame_tile == PR.TILE
    wav = PR.batch(rows, ld=max(lengths) + 13)                                                        # NaN beyond every row's length
    F_max = PR.num_frames(max(lengths), geo) + 2
    f0, ap, dp = _run(trk, wav, lengths, frames=F_max)
    worst, frames, excused = PR.check_case(name, dp, f0, ap, 'device')
    print("geometry %s: %d frames, %d excused, worst d' error / beta %.3f" % (name, frames, excused, worst))
    PARITY[name] = {'worst_error_over_bound': worst, 'frames': frames, 'excused': excused, 'beta': PR.beta(geo)}
    hook = _ext.pitch_host(geo, wav, lengths, frames=F_max, return_dprime=True, fill=SENTINEL)       # bit for bit, the sentinel beyond every row's frames included
    for k, got in (('f0', f0), ('ap', ap), ('dprime', dp)):
        assert np.array_equal(PR.bits(got), PR.bits(hook[k])), (name, k)
    for b, n in enumerate(lengths):
        F = PR.num_frames(n, geo)
        assert np.all(f0[b, F:] == SENTINEL) and np.all(ap[b, F:] == SENTINEL) and np.all(dp[b, F:] == SENTINEL), (name, b)
        assert np.all(np.isfinite(f0[b, :F])) and np.all(np.isfinite(dp[b, :F])), (name, b)
    f0_only = _run(trk, wav, lengths, frames=F_max, dprime=False)[0]                                  # the optional outputs left out: the same track
    assert np.array_equal(PR.bits(f0_only), PR.bits(f0))
    t, w = torch.zeros(len(rows), F_max, device='cuda'), _dev(wav)
    trk.lib.wn_pitch_run(trk.h, _ext._ptr(w), wav.shape[1], (_ext.ctypes.c_int32 * len(lengths))(*lengths), len(lengths), F_max, _ext._ptr(t), None, None, _ext._stream())
    torch.cuda.synchronize()
    for b, n in enumerate(lengths):
        F = PR.num_frames(n, geo)
        assert np.array_equal(PR.bits(t[b, :F].cpu().numpy()), PR.bits(f0[b, :F]))                    # ap = NULL too
    trk.close()


@pytest.mark.parametrize('name', NAMES)
def test_a_rows_bits_do_not_depend_on_the_batch(name):
    """alone and in a batch, at another row index, at another ld, with other neighbours, and run to run"""
    geo, lengths, rows, _ = PR.case(name)
    trk = _tracker(name, len(rows), max(lengths) + 100)
    base = _run(trk, PR.batch(rows), lengths)
    again = _run(trk, PR.batch(rows), lengths)
    for x, y in zip(base, again):
        assert np.array_equal(PR.bits(x), PR.bits(y))
    order = [11, 3, 7, 0, 9] if name != 'P' else [9, 3, 11, 0]
    got = _run(trk, PR.batch(rows, ld=max(lengths) + 99, order=order), [lengths[i] for i in order])
    for b, i in enumerate(order):
        F = PR.num_frames(lengths[i], geo)
        for x, y in zip(got, base):
            assert np.array_equal(PR.bits(x[b, :F]), PR.bits(y[i, :F])), (name, i)
    for i in (10, 6):
        alone = _run(trk, rows[i][None], [lengths[i]])
        F = PR.num_frames(lengths[i], geo)
        for x, y in zip(alone, base):
            assert np.array_equal(PR.bits(x[0, :F]), PR.bits(y[i, :F])), (name, i)
    trk.close()


def test_the_walk_stops_at_an_exact_tie():
    from wavenet_vocoder import _ext
    trk = _ext.PitchTracker(dict(PR.TIE_GEO), 1, len(PR.TIE_SIGNAL))
    f0, ap, dp = _run(trk, PR.TIE_SIGNAL[None], [len(PR.TIE_SIGNAL)])
    PR.check_tie(f0[0], dp[0], 'device')
    trk.close()


def test_a_batch_beyond_one_launch_group():
    """70 rows: the rows of the second launch group (64 ...) equal the same rows computed alone"""
    geo, lengths, rows, _ = PR.case('A')
    pick = [(7 * b) % 11 for b in range(70)]
    trk = _tracker('A', 70, max(lengths))
    got = _run(trk, PR.batch(rows, order=pick), [lengths[i] for i in pick], dprime=False)
    base = _run(trk, PR.batch(rows), lengths, dprime=False)
    for b, i in enumerate(pick):
        F = PR.num_frames(lengths[i], geo)
        assert np.array_equal(PR.bits(got[0][b, :F]), PR.bits(base[0][i, :F])) and np.array_equal(PR.bits(got[1][b, :F]), PR.bits(base[1][i, :F])), b
    trk.close()


@pytest.mark.parametrize('name', NAMES)
def test_comparison_against_the_hook_and_float64(name):
    """the table of the device's own tracks: within 2 float32 ulps of the hook's, within 1e-6 relative of the float64 comparison; cells of other rows untouched"""
    from wavenet_vocoder import _ext
    geo, lengths, rows, _ = PR.case(name)
    trk = _tracker(name, len(rows), max(lengths))
    f0 = _run(trk, PR.batch(rows), lengths, dprime=False)[0]
    frames = [PR.num_frames(n, geo) for n in lengths]
    other = np.roll(f0, 1, axis=1) * np.float32(1.013)                                                # a second track: shifted in time, 22 cents up, so every kind of frame occurs
    other[:, ::3] *= np.float32(1.5)                                                                  # and some gross errors
    fa, fb = np.where(np.isfinite(f0), f0, 0).astype(np.float32), np.where(np.isfinite(other), other, 0).astype(np.float32)
    table = trk.compare(_dev(fa), _dev(fb), frames)
    torch.cuda.synchronize()
    table = table.cpu().numpy()
    hook = _ext.pitch_compare_host(fa, fb, frames)
    ref = PR.compare(fa, fb, frames)
    assert np.all(np.abs(table.astype(np.float64) - hook.astype(np.float64)) <= 2 * np.spacing(np.abs(hook))), name
    assert np.all(np.abs(table - ref) <= 1e-6 * np.abs(ref) + 1e-30), name
    assert np.array_equal(table[:, :4], ref[:, :4].astype(np.float32)) and ref[:, 3].sum() > 10 and 0 < ref[-1, 5] < 1 and 0 < ref[-1, 4] < 1
    same = trk.compare(_dev(fa), _dev(fa.copy()), frames).cpu().numpy()
    assert np.all(same[:, 4:] == 0.0) and np.array_equal(same[:, 1], same[:, 3])
    sub = trk.compare(_dev(fa[5:]), _dev(fb[5:]), frames[5:]).cpu().numpy()                             # a row's table does not depend on its index
    assert np.array_equal(PR.bits(sub), PR.bits(table[5:]))
    trk.close()


def test_long_rows_compare_in_chunks():
    """more frames than one pass of the comparison's workgroup (256), the count not a multiple of it"""
    from wavenet_vocoder import _ext
    rng = np.random.RandomState(3)
    F = 1000
    fa = np.where(rng.rand(2, F) < 0.7, rng.uniform(80, 400, (2, F)), 0).astype(np.float32)
    fb = np.where(rng.rand(2, F) < 0.7, fa * rng.uniform(0.9, 1.3, (2, F)), 0).astype(np.float32)
    trk = _tracker('A', 2, F * 16)
    for frames in ([F, 777], [256, 257]):
        table = trk.compare(_dev(fa), _dev(fb), frames).cpu().numpy()
        hook, ref = _ext.pitch_compare_host(fa, fb, frames), PR.compare(fa, fb, frames)
        assert np.all(np.abs(table.astype(np.float64) - hook.astype(np.float64)) <= 2 * np.spacing(np.abs(hook))) and np.all(np.abs(table - ref) <= 1e-6 * np.abs(ref))
    trk.close()


def test_pitch_check_scores_a_pair_like_the_host():
    """PitchCheck.score on the device equals the host evaluation of the same pair; a signal against itself scores zero"""
    import hparams as H
    from wavenet_vocoder import pitch as PT
    hp = H._build()
    n = 6000
    a, b = PR.signal(PR.GEOMETRIES['P'], n, 31), PR.signal(PR.GEOMETRIES['P'], n, 32)
    chk = PT.PitchCheck(hp, 2, n)
    table = chk.score(_dev(np.stack([a, a])), _dev(np.stack([a, b])), [n, n - 700])
    chk.close()
    host = PT.score_host([a, a[:n - 700]], [a, b[:n - 700]], hp)
    assert table.shape == (2, 9) and np.all(table[0, 4:] == 0.0) and table[0, 0] == 22 and table[1, 0] == 20
    assert np.all(np.abs(table.astype(np.float64) - host) <= 2 * np.spacing(np.abs(host)))


TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_pitch_window=64,mi355_pitch_fmin=552,mi355_pitch_fmax=4410')      # lags 5 ... 40 at hop 16: geometry A at 22.05 kHz
TINY_GEO = dict(PR.GEOMETRIES['A'], sample_rate=22050)
ROUTES = {'oneshot': '', 'slots': ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,input_type=mulaw-quantize,quantize_channels=256,out_channels=256',
          'fold': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4',
          'fold-device': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4,mi355_output_stage=device'}


def test_eval_step_writes_the_three_scalars_beside_the_eval_loss(tmp_path):
    """eval_step with the key on: the generated item is tracked next to its target and the three scalars equal an independent score of the same tensors;
    everything else of the row is what the key off writes"""
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.train import eval_step
    Tc, hop = 30, 16
    y = torch.from_numpy(PR.signal(PR.GEOMETRIES['A'], Tc * hop, 5)[None].clip(-0.99, 0.99)).cuda()
    c01 = torch.from_numpy(np.random.RandomState(3).uniform(0, 1, size=(1, 16, Tc)).astype(np.float32)).cuda()
    lines = {}
    for on in (False, True):
        plots, wavs = str(tmp_path / ('plots%d' % on)), str(tmp_path / ('wavs%d' % on))
        os.makedirs(plots); os.makedirs(wavs)
        hp = H._build(); hp.parse(TINY + (',mi355_pitch_check=True' if on else ''))
        model = WaveNet(hp)
        model.build(1, Tc * hop)
        out = io.StringIO()
        eval_step(model, (None, y, [Tc * hop], c01, None), 7, plots, wavs, out, hp, 'WaveNet')
        lines[on] = json.loads(out.getvalue())
        if on:
            chk = model.pitch_check(1, Tc * hop)
            assert chk.geometry == TINY_GEO
            t = chk.score(model.tower_y_hat[0].float().reshape(1, -1).contiguous(), model.tower_y_target[0].float().reshape(1, -1).contiguous(), [Tc * hop])[0]
            chk.close()
        model.engine.close()
    pre = 'Wavenet_eval_model/eval_stats/wavenet_eval_'
    assert set(lines[False]) == {'step', pre + 'loss'}
    assert set(lines[True]) == {'step', pre + 'loss', pre + 'f0_rmse_cents', pre + 'vuv_error', pre + 'gpe'}
    assert lines[True]['step'] == lines[False]['step'] and lines[True][pre + 'loss'] == lines[False][pre + 'loss']
    assert t[0] == Tc + 1 and t[1] > 3                                                                # the target has voiced frames
    assert lines[True][pre + 'f0_rmse_cents'] == float(t[6]) and lines[True][pre + 'vuv_error'] == float(t[4]) and lines[True][pre + 'gpe'] == float(t[5])


@pytest.mark.parametrize('route', ['oneshot', 'slots', 'fold', 'fold-device'])
def test_wavs_dir_writes_one_row_per_utterance(tmp_path, route):
    """synthesize.py --wavs_dir with the key on: wavs/pitch.tsv holds one row per recording, equal to the host evaluation of the written pair's signals; the
    wavs, mels and map.txt are byte-identical to the run with the key off, which writes no pitch.tsv"""
    import argparse
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder import pitch as PT
    from wavenet_vocoder import synthesize as S
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesizer import Synthesizer
    base = TINY + ',wavenet_synthesis_batch_size=2' + ROUTES[route]
    rec = str(tmp_path / 'rec'); os.makedirs(rec)
    lens = (480, 333, 700)
    for i, n in enumerate(lens):
        x = PR.signal(PR.GEOMETRIES['A'], n, 40 + i)
        wavfile.write(os.path.join(rec, 'r%d.wav' % i), 22050, (x * 32767 / max(np.abs(x).max(), 1e-3) * 0.9).astype(np.int16))
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(2, 800)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()
    seen = []
    inner = Synthesizer._pitch

    def spy(self, decoded, generated_wavs, basenames, out_dir):
        refs = self.pitch_references
        table = inner(self, decoded, generated_wavs, basenames, out_dir)
        if table is not None:
            gen = [decoded[b].float().cpu().numpy() for b in range(len(refs))] if decoded is not None else [np.asarray(w, np.float32) for w in generated_wavs]
            seen.append((gen, refs, table))
        return table

    outs = {}
    for on in (False, True):
        hp = H._build(); hp.parse(base + (',mi355_pitch_check=True' if on else ''))
        out = str(tmp_path / ('out%d' % on))
        Synthesizer._pitch = spy
        try:
            S.run_wav_synthesis(argparse.Namespace(wavs_dir=rec), ckpt, out, hp)
        finally:
            Synthesizer._pitch = inner
        outs[on] = os.path.join(out, 'wavs')
    off, on = sorted(os.listdir(outs[False])), sorted(os.listdir(outs[True]))
    assert 'pitch.tsv' not in off and on == sorted(off + ['pitch.tsv'])
    for n in off:
        a, b = open(os.path.join(outs[False], n), 'rb').read(), open(os.path.join(outs[True], n), 'rb').read()
        if n == 'map.txt':
            a, b = a.replace(b'out0', b'outX'), b.replace(b'out1', b'outX')
        assert a == b, n
    rows = PT.read_tsv(os.path.join(outs[True], 'pitch.tsv'))
    assert [r['name'] for r in rows] == ['r0', 'r1', 'r2'] and [int(r['frames']) for r in rows] == [1 + n // 16 for n in lens]
    assert len(seen) == 2                                                                             # two batches: 2 + 1 utterances
    k, hp = 0, H._build().parse(base)
    for gen, refs, table in seen:
        host = PT.score_host(gen, refs, hp)
        assert np.all(np.abs(table.astype(np.float64) - host) <= 2 * np.spacing(np.abs(host)))
        for row in table:
            assert rows[k] == dict(zip(PT.TSV_HEADER, PT.tsv_row('r%d' % k, row).split('\t')))
            k += 1
