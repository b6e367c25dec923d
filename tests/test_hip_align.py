"""Alignment check on the device (csrc/wn_align.hip): every stage of wn_align_run -- cepstra, cost matrix, Dm -- against the float64 reference of
tests/align_ref.py applied to the device's OWN previous stage, inside the bounds derived there; the path against the reference back-trace of the device's own
Dm and the near-optimality inequality; everything bit for bit against the host hook; the invariance of a row's bits; exact integer costs through
wn_test_align_dp; the composed score on two tones; the synthesize.py route on a tiny model.  Frame counts sit at 1, around the block height T and its
multiples (more than one block row, column and round of four blocks on a diagonal), with pitches larger than the rows, NaN beyond every row's frames and
sentinels in every output.  WN_ALIGN_PARITY_OUT=<file> makes the session write the worst error / bound per stage and case there
(profiles/align_parity.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch

import align_ref as R

pytestmark = pytest.mark.gpu
PARITY = {}
T = 64
SHAPES = [(1, 1), (1, 7), (7, 1), (T - 1, T), (T, T + 1), (T + 1, T - 1), (2 * T + 1, 40), (40, 2 * T + 1), (200, 200)]
FA, FB = [s[0] for s in SHAPES], [s[1] for s in SHAPES]
UNIT = 2.5
CASES = [(M, K, band) for M in (16, 80) for K in (1, 13) for band in (0, 1, 4)]


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    yield
    path = os.environ.get('WN_ALIGN_PARITY_OUT')
    if path and PARITY:
        with open(path, 'w') as f:
            json.dump({'what': 'wn_align_run on an MI355X against the float64 reference of tests/align_ref.py applied to the device\'s own previous stage: worst |error| / bound '
                               'over every element of the ragged batch of tests/test_hip_align.py::test_every_stage_against_float64_and_the_hook, and the path\'s cost over '
                               'its near-optimality limit', 'cases': PARITY}, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


_MELS = {}


def _mels(M):
    """the ragged batch: smooth random mel-like rows (b a warped, perturbed a, so that the path bends), NaN beyond every row's frames; a channels-first with
    a pitch of 211, b channels-last with a pitch of 205"""
    if M not in _MELS:
        rng = np.random.RandomState(100 + M)
        a, b = np.full((len(SHAPES), M, 211), np.nan, np.float32), np.full((len(SHAPES), 205, M), np.nan, np.float32)
        for r, (Fa, Fb) in enumerate(SHAPES):
            x = np.cumsum(rng.randn(Fa, M), axis=0).astype(np.float32) * 0.3 + rng.randn(1, M).astype(np.float32)
            pos = np.clip(np.round(np.linspace(0, Fa - 1, Fb) + 2.0 * np.sin(np.arange(Fb) / 9.0)).astype(int), 0, Fa - 1)
            a[r, :, :Fa] = x.T
            b[r, :Fb] = x[pos] + 0.1 * rng.randn(Fb, M).astype(np.float32) + 0.7
        _MELS[M] = (a, b)
    return _MELS[M]


def _run(al, a, b, fa, fb, a_cf=True, b_cf=False, want=('path', 'map_ab', 'map_ba'), pitches=(None, None, None)):
    out = al.run(_dev(a), _dev(b), fa, fb, a_channels_first=a_cf, b_channels_first=b_cf, want=want, pitches=pitches)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _same(x, y):
    return np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32))


@pytest.mark.parametrize('M,K,band', CASES)
def test_every_stage_against_float64_and_the_hook(M, K, band):
    from wavenet_vocoder import _ext
    a, b = _mels(M)
    al = _ext.Aligner(M, len(SHAPES), 203, 201, n_cep=K, unit_db=UNIT, band=band)
    assert al.tile == T
    al.store_matrix(True)
    got = _run(al, a, b, FA, FB, pitches=(411, 209, 207))
    cep_a, cep_b, cost, dm = (al.copy_stage(k) for k in _ext.ALIGN_STAGES)
    hook = _ext.align_host(a, b, FA, FB, n_cep=K, unit_db=UNIT, band=band, b_channels_first=False, stages=True, path_pitch=411, map_a_pitch=209, map_b_pitch=207)
    worst = {'cepstra': 0.0, 'cost': 0.0, 'recurrence': 0.0, 'near_optimal': 0.0}
    for r, (Fa, Fb) in enumerate(SHAPES):
        for side, x, c in (('a', a[r, :, :Fa].T, cep_a[r, :Fa]), ('b', b[r, :Fb], cep_b[r, :Fb])):
            c64, bound = R.cepstra(x, UNIT, K)
            err = np.abs(c - c64)
            assert np.all(err <= bound), (r, side, float(np.max(err / np.maximum(bound, 1e-300))))
            worst['cepstra'] = max(worst['cepstra'], float(np.max(err / np.maximum(bound, 1e-300))))
        k64, rel = R.cost_matrix(cep_a[r, :Fa], cep_b[r, :Fb])
        err = np.abs(cost[r, :Fa, :Fb] - k64)
        assert np.all(err <= rel * k64), (r, 'cost')
        worst['cost'] = max(worst['cost'], float(np.max(err / np.maximum(rel * k64, 1e-300))))
        d64 = R.recurrence(cost[r, :Fa, :Fb], band)
        d = dm[r, :Fa, :Fb]
        assert np.array_equal(np.isinf(d), np.isinf(d64)) and not np.any(np.isnan(d)), (r, 'admissible cells')
        fin = np.isfinite(d64)
        err, bound = np.abs(d[fin] - d64[fin]), R.recurrence_bound(d64)[fin]
        assert np.all(err <= bound), (r, 'recurrence')
        worst['recurrence'] = max(worst['recurrence'], float(np.max(err / np.maximum(bound, 1e-300))))
        ref_path = R.backtrace(d, band)
        n = int(got['summary'][r, 2])
        assert n == len(ref_path) and np.array_equal(got['path'][r, :, :n].T, ref_path), (r, 'path')
        assert R.is_valid_path(ref_path, Fa, Fb) and all(R.admissible(i, j, Fa, Fb, band) for i, j in ref_path)
        tc, lim = R.near_optimal(ref_path, cost[r, :Fa, :Fb], d64[-1, -1])
        assert tc <= lim, (r, tc, lim)
        worst['near_optimal'] = max(worst['near_optimal'], tc / lim)
        mab, mba = R.maps(ref_path, Fa, Fb)
        assert np.array_equal(got['map_ab'][r, :Fa], mab) and np.array_equal(got['map_ba'][r, :Fb], mba)
        s64 = R.summary(ref_path, cost[r, :Fa, :Fb], d[-1, -1])
        assert np.array_equal(got['summary'][r, :4], s64[:4].astype(np.float32)) and np.all(np.abs(got['summary'][r, 4:] - s64[4:]) <= 2.0 ** -23 * np.abs(s64[4:]))
        # sentinels: cells beyond the row's extent keep the caller's bytes
        assert np.all(got['path'][r, :, n:] == -7) and np.all(got['map_ab'][r, Fa:] == -7) and np.all(got['map_ba'][r, Fb:] == -7)
        # the host hook: the same bits at every stage
        assert _same(cep_a[r, :Fa], hook['cep_a'][r, :Fa]) and _same(cep_b[r, :Fb], hook['cep_b'][r, :Fb]), (r, 'hook cepstra')
        assert _same(cost[r, :Fa, :Fb], hook['cost'][r, :Fa, :Fb]) and _same(d, hook['dm'][r, :Fa, :Fb]), (r, 'hook matrices')
    for k in ('path', 'map_ab', 'map_ba'):
        assert np.array_equal(got[k], hook[k]), k
    assert _same(got['summary'], hook['summary'])
    print('M %d n_cep %d band %d: worst error / bound %r' % (M, K, band, worst))
    PARITY['M%d_ncep%d_band%d' % (M, K, band)] = worst
    al.close()


@pytest.mark.parametrize('band', [0, 1])
def test_a_rows_bits_do_not_depend_on_the_batch(band):
    """run to run, alone, at another row index with other neighbours, in the other layouts with other pitches, with outputs left out, without the Dm copy"""
    from wavenet_vocoder import _ext
    M, K = 16, 13
    a, b = _mels(M)
    al = _ext.Aligner(M, len(SHAPES), 203, 201, n_cep=K, unit_db=UNIT, band=band)
    al.store_matrix(True)
    base = _run(al, a, b, FA, FB)
    dm = al.copy_stage('dm')
    again = _run(al, a, b, FA, FB)
    for k in base:
        assert _same(base[k], again[k]), k
    al.store_matrix(False)
    order = [8, 3, 6, 0, 5, 7]
    a2 = np.full((len(order), 230, M), np.nan, np.float32)            # a channels-last, b channels-first, other pitches
    b2 = np.full((len(order), M, 240), np.nan, np.float32)
    for q, r in enumerate(order):
        a2[q, :FA[r]] = a[r, :, :FA[r]].T
        b2[q, :, :FB[r]] = b[r, :FB[r]].T
    moved = _run(al, a2, b2, [FA[r] for r in order], [FB[r] for r in order], a_cf=False, b_cf=True, pitches=(500, 300, 301))
    only = _run(al, a2, b2, [FA[r] for r in order], [FB[r] for r in order], a_cf=False, b_cf=True, want=())
    assert only['path'] is None and only['map_ab'] is None and _same(only['summary'], moved['summary'])
    for q, r in enumerate(order):
        n = int(base['summary'][r, 2])
        assert _same(moved['summary'][q], base['summary'][r]) and np.array_equal(moved['path'][q, :, :n], base['path'][r, :, :n]), r
        assert np.array_equal(moved['map_ab'][q, :FA[r]], base['map_ab'][r, :FA[r]]) and np.array_equal(moved['map_ba'][q, :FB[r]], base['map_ba'][r, :FB[r]]), r
        assert np.all(moved['path'][q, :, n:] == -7) and np.all(moved['map_ab'][q, FA[r]:] == -7) and np.all(moved['map_ba'][q, FB[r]:] == -7)
    al.store_matrix(True)
    for r in range(len(SHAPES)):
        alone = _run(al, a[r:r + 1], b[r:r + 1], [FA[r]], [FB[r]])
        n = int(base['summary'][r, 2])
        assert _same(alone['summary'][0], base['summary'][r]) and np.array_equal(alone['path'][0, :, :n], base['path'][r, :, :n]), r
        assert _same(al.copy_stage('dm')[0, :FA[r], :FB[r]], dm[r, :FA[r], :FB[r]]), r
    al.close()


def test_a_batch_beyond_one_launch_group():
    """35 rows: the rows of the second launch group (32 ...) equal the same rows of the base batch"""
    from wavenet_vocoder import _ext
    M, K = 16, 13
    a, b = _mels(M)
    pick = [(5 * q) % 8 for q in range(35)]                              # (the 200 x 200 row is left out: small rows keep this quick)
    al = _ext.Aligner(M, 35, 203, 201, n_cep=K, unit_db=UNIT, band=4)
    base = _run(al, a[:8], b[:8], FA[:8], FB[:8])
    got = _run(al, a[pick], b[pick], [FA[r] for r in pick], [FB[r] for r in pick])
    for q, r in enumerate(pick):
        n = int(base['summary'][r, 2])
        assert _same(got['summary'][q], base['summary'][r]) and np.array_equal(got['path'][q, :, :n], base['path'][r, :, :n]), q
    al.close()


@pytest.mark.parametrize('band', [0, 1, 4])
def test_exact_integer_costs_through_the_recurrence_alone(band):
    """small non-negative integer costs (every sum below 2^24, so float32 is exact): Dm equals float64 in EVERY cell and the path equals float64's, ties
    included -- the tie order is pinned -- and both equal the host twin bit for bit"""
    from wavenet_vocoder import _ext
    rng = np.random.RandomState(7 + band)
    cost = rng.randint(0, 4, size=(len(SHAPES), 203, 201)).astype(np.float32)       # few distinct values: ties everywhere
    al = _ext.Aligner(16, len(SHAPES), 203, 201, n_cep=1, band=band)
    al.store_matrix(True)
    out = al.run_dp(_dev(cost), FA, FB)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    dm = al.copy_stage('dm')
    host = _ext.align_dp_host(cost, FA, FB, band=band)
    for r, (Fa, Fb) in enumerate(SHAPES):
        d64 = R.recurrence(cost[r, :Fa, :Fb], band)
        assert np.array_equal(dm[r, :Fa, :Fb].astype(np.float64), d64), r
        p64 = R.backtrace(d64, band)
        n = int(got['summary'][r, 2])
        assert n == len(p64) and np.array_equal(got['path'][r, :, :n].T, p64), r
        assert got['summary'][r, 3] == d64[-1, -1] and _same(dm[r, :Fa, :Fb], host['dm'][r, :Fa, :Fb])
    for k in ('path', 'map_ab', 'map_ba'):
        assert np.array_equal(got[k], host[k]), k
    assert _same(got['summary'], host['summary'])
    al.close()


def test_non_finite_inputs_give_a_valid_path():
    """NaN and inf frames: the back-trace is bounded and its indices are clamped, so the path is a valid one whatever the values"""
    from wavenet_vocoder import _ext
    M = 16
    a, b = (x.copy() for x in _mels(M))
    r = 4                                                                # (T, T + 1)
    a[r, :, 10:20] = np.nan; b[r, 30:33] = np.inf; a[r, 3, 40] = -np.inf
    al = _ext.Aligner(M, 1, 203, 201, n_cep=13, band=1)
    got = _run(al, a[r:r + 1], b[r:r + 1], [FA[r]], [FB[r]])
    n = int(got['summary'][0, 2])
    assert 1 <= n <= FA[r] + FB[r] - 1 and R.is_valid_path(got['path'][0, :, :n].T, FA[r], FB[r])
    hook = _ext.align_host(a[r:r + 1], b[r:r + 1], [FA[r]], [FB[r]], n_cep=13, band=1, b_channels_first=False)
    assert np.array_equal(got['path'], hook['path'])
    al.close()


def test_reserve_limit_and_validation_on_a_device_handle():
    from wavenet_vocoder import _ext
    for kw in (dict(max_batch=1, max_frames_a=4097, max_frames_b=10), dict(max_batch=40, max_frames_a=2048, max_frames_b=2048)):
        with pytest.raises(_ext.WnError) as e:
            _ext.Aligner(16, kw['max_batch'], kw['max_frames_a'], kw['max_frames_b'])
        assert e.value.code == -4                                         # WN_E_UNSUPPORTED: above the reserve limit
    al = _ext.Aligner(16, 2, 50, 60)
    a, b = _dev(np.zeros((2, 16, 50), np.float32)), _dev(np.zeros((2, 16, 60), np.float32))
    for fa, fb in (([51, 1], [1, 1]), ([1, 1], [1, 61])):
        with pytest.raises(_ext.WnError) as e:
            al.run(a, b, fa, fb, b_channels_first=True)
        assert e.value.code == -2
    with pytest.raises(_ext.WnError) as e:
        al.run(a, b, [0, 1], [1, 1], b_channels_first=True)
    assert e.value.code == -1
    al.close()


# ---- the composed score and the synthesize.py route
TONE_HP = 'hop_size=256,n_fft=1024,win_size=1024,mi355_pitch_window=512,mi355_pitch_fmin=80'      # lags 44 ... 276: a pitch frame (788 samples) lies inside its mel frame (1024)
NOTES_REF = [(128, 10), (64, 8), (256, 12), (128, 9)]          # (period in samples, length in hops): 172, 345, 86, 172 Hz
NOTES_GEN = [(128, 10), (64, 16), (256, 6), (128, 9)]          # the same notes, the second stretched by 2, the third by 1 / 2


def notes(segments, hop=256):
    """three-harmonic tones back to back; every period divides the hop, so a frame's samples depend on its distance from the note boundaries alone"""
    out = []
    for period, hops in segments:
        k = np.arange(hops * hop, dtype=np.float64)
        out.append(sum(amp * np.sin(2 * np.pi * h * k / period) for h, amp in ((1, 0.5), (2, 0.25), (3, 0.15))))
    return np.concatenate(out).astype(np.float32)


def test_score_warps_the_f0_track_of_a_stretched_tone():
    """two three-harmonic tones, the second the first time-stretched by the known piecewise-constant factors 1, 2, 1 / 2, 1 over notes an octave apart.  Every
    frame of the one has a twin of identical samples in the other and a monotone path pairs twins throughout, so along the DTW path the F0 RMSE is below the
    pitch check's own tone accuracy (1 cent: tests/test_pitch_cpu.py::test_comparison_semantics), there is no gross error and no voicing error; without the
    warp (the plain pitch check of the same pair) the notes overlap an octave apart and the error is far above it (> 100 cents)"""
    import hparams as H
    from wavenet_vocoder import alignment as AL
    from wavenet_vocoder import pitch as PT
    hp = H._build().parse(TONE_HP)
    ref, gen = notes(NOTES_REF), notes(NOTES_GEN)
    chk = AL.AlignmentCheck(hp, 1, max(len(ref), len(gen)))
    table = chk.score(_dev(gen[None]), [len(gen)], _dev(ref[None]), [len(ref)])
    chk.close()
    row = dict(zip(AL.COLUMNS, table[0]))
    n = min(len(ref), len(gen))
    plain = PT.score_device([gen[:n]], [ref[:n]], hp)[0]
    print('warped F0 RMSE %.3f cents, gpe %.3f, vuv %.3f over %d voiced pairs; unwarped %.2f cents (gpe %.3f); mcd_dtw %.5f dB, stretch %.3f' % (
        row['f0_rmse_cents'], row['gpe'], row['vuv_error'], row['both'], plain[6], plain[5], row['mcd_dtw'], row['stretch']))
    assert row['frames_gen'] == 1 + len(gen) // 256 and row['frames_ref'] == 1 + len(ref) // 256 and row['stretch'] > 0.1
    # voiced in both: all but the frames whose 788-sample pitch window straddles one of the three note boundaries (a centre within 394 samples: three frames
    # each) and the two edge frames, half zeros
    assert row['both'] >= row['frames_ref'] - 11
    assert row['f0_rmse_cents'] < 1.0 and row['gpe'] == 0.0 and row['vuv_error'] == 0.0
    assert plain[6] > 100.0
    host = AL.score_host([gen], [ref], hp)[0]
    assert abs(host[4] - table[0][4]) <= 1e-3 and abs(host[10] - table[0][10]) < 1.0          # the host route analyses in float64 numpy: the same score to analysis roundoff


TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_pitch_window=64,mi355_pitch_fmin=552,mi355_pitch_fmax=4410')


def test_mels_dir_route_writes_one_row_per_utterance_with_a_recording(tmp_path):
    """synthesize.py --mels_dir with mi355_alignment_reference_dir set: wavs/alignment.tsv holds one row per utterance whose basename has a wav there (a mel-
    prefix does not count), every other file is byte-identical to the run with the key off, which writes no alignment.tsv"""
    import argparse
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder import alignment as AL
    from wavenet_vocoder import synthesize as S
    from wavenet_vocoder.models.wavenet import WaveNet
    base = TINY + ',wavenet_synthesis_batch_size=2'
    rec, mels = str(tmp_path / 'rec'), str(tmp_path / 'mels')
    os.makedirs(rec); os.makedirs(mels)
    rng = np.random.RandomState(5)
    for name, F, n in (('mel-u0', 30, 520), ('u1', 41, 700), ('u2', 25, 0)):          # u2 has no recording
        np.save(os.path.join(mels, name + '.npy'), rng.uniform(-3, 3, size=(F, 16)).astype(np.float32))
        if n:
            x = np.sin(2 * np.pi * 700.0 * np.arange(n) / 22050.0) * (0.3 + 0.2 * np.sin(np.arange(n) / 90.0))
            wavfile.write(os.path.join(rec, name.replace('mel-', '') + '.wav'), 22050, (x * 32767).astype(np.int16))
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(2, 800)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()
    outs = {}
    for on in (False, True):
        hp = H._build(); hp.parse(base + (',mi355_alignment_reference_dir=' + rec + ',mi355_alignment_band=4' if on else ''))
        out = str(tmp_path / ('out%d' % on))
        S.run_synthesis(argparse.Namespace(mels_dir=mels, model='WaveNet', speaker_id=None), ckpt, out, hp)
        outs[on] = os.path.join(out, 'wavs')
    off, on = sorted(os.listdir(outs[False])), sorted(os.listdir(outs[True]))
    assert 'alignment.tsv' not in off and on == sorted(off + ['alignment.tsv'])
    for n in off:
        x, y = open(os.path.join(outs[False], n), 'rb').read(), open(os.path.join(outs[True], n), 'rb').read()
        if n == 'map.txt':
            x, y = x.replace(b'out0', b'outX'), y.replace(b'out1', b'outX')
        assert x == y, n
    rows = AL.read_tsv(os.path.join(outs[True], 'alignment.tsv'))
    assert [r['name'] for r in rows] == ['mel-u0', 'u1']
    assert [int(r['frames_gen']) for r in rows] == [31, 42] and [int(r['frames_ref']) for r in rows] == [1 + 520 // 16, 1 + 700 // 16]
    assert all(np.isfinite(float(r['mcd_dtw'])) and float(r['mcd_dtw']) > 0 for r in rows)
