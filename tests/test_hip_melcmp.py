"""Reconstruction check on the device (csrc/wn_melcmp.hip): every element of wn_melcmp_run against the float64 reference of tests/melcmp_util.py inside the
derived bound, and against the host hook bit for bit, over ragged batches, four channel counts, three cepstral orders, the four layout pairs, tight and
padded pitches and a batch that crosses a launch group; NaN beyond every row's frames and in the pitch padding; ReconstructionCheck.score on a synthetic
signal; and the Synthesizer with the switch on through its three routes.  WN_MELCMP_PARITY_OUT=<file> makes the session write the worst err / bound and
err / yardstick per result kind there (profiles/melcmp_parity.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch

import melcmp_util as MU

pytestmark = pytest.mark.gpu

UNIT, ALARM = 12.5, 30.0
CASES = [(M, nc) for M in (1, 13, 80, 128) for nc in sorted({0, min(13, M - 1), M - 1})]
BATCHES = ((0, 1, 63, 65, 300), (64, 128, 129))
PARITY = {}


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    yield
    path = os.environ.get('WN_MELCMP_PARITY_OUT')
    if path and PARITY:
        with open(path, 'w') as f:
            json.dump({'what': 'wn_melcmp_run on an MI355X against the float64 reference of tests/melcmp_util.py: worst error / derived bound per result kind over every element, and the worst per-case ratio of the '
                               'worst error to the floored error of the numpy float32 yardstick (asserted <= 8), of tests/test_hip_melcmp.py::test_device_against_float64_and_the_hook '
                               '(lsd, mcd, lsdc on their squares)', 'kinds': PARITY}, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _run(cmp, a, b, frames, a_cf=True, b_cf=True, ap=None, bp=None, per_frame=True):
    """a, b [B, M, P] numpy channels first -> the device's results as numpy, inputs laid out as asked with NaN in the pitch padding"""
    r = cmp.run(_dev(MU.layout(a, a_cf, ap)), _dev(MU.layout(b, b_cf, bp)), frames, a_channels_first=a_cf, b_channels_first=b_cf, per_frame=per_frame)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in r.items()}


def _same(x, y, frames):
    for r, F in enumerate(frames):
        assert np.array_equal(MU.bits(x['per_frame'][r][:, :F]), MU.bits(y['per_frame'][r][:, :F])), r
    assert np.array_equal(MU.bits(x['summary']), MU.bits(y['summary'])) and np.array_equal(x['marks'], y['marks'])


@pytest.mark.parametrize('M,n_cep', CASES)
def test_device_against_float64_and_the_hook(M, n_cep):
    """EVERY element: inside the derived bound of the float64 reference, and the hook's bits; the same bits run to run, in all four layout pairs, at tight and
    padded pitches, with and without per_frame, and for each row wherever it stands in a batch of 35 that crosses the 32-row launch group.  The inputs carry
    NaN beyond every row's frames and in the pitch padding."""
    from wavenet_vocoder import _ext
    cmp = _ext.MelCompare(M, 40, 300, n_cep=n_cep, unit_db=UNIT, alarm_db=ALARM)
    for bi, frames in enumerate(BATCHES):
        P = max(frames)
        a, b = MU.mels(len(frames), M, P, 10 + bi), MU.mels(len(frames), M, P, 20 + bi)
        ref = MU.reference(a, b, frames, n_cep, UNIT, ALARM)
        bnd = MU.bounds(a, b, frames, n_cep, UNIT)
        yard = MU.reference(a, b, frames, n_cep, UNIT, ALARM, dtype=np.float32)
        ap, bp = MU.poison(a, frames), MU.poison(b, frames)
        hook = _ext.melcmp_host(ap, bp, frames, n_cep=n_cep, unit_db=UNIT, alarm_db=ALARM)
        base = _run(cmp, ap, bp, frames)
        for r, F in enumerate(frames):
            ratios = MU.check_row(base['per_frame'][r], base['summary'][r], base['marks'][r], ref[r], bnd[r], ALARM, (M, n_cep, bi, r))
            MU.check_row(yard[r]['per_frame'], yard[r]['summary'], yard[r]['marks'], ref[r], bnd[r], ALARM, ('yardstick', M, n_cep, bi, r))      # the bound holds for plain float32 on THESE inputs
            for k, q in ratios.items():
                rec = PARITY.setdefault(k, {'err_over_bound': 0.0, 'err_over_floored_yardstick': 0.0})
                rec['err_over_bound'] = max(rec['err_over_bound'], q)
            print('M %d n_cep %d batch %d row %d (%d frames): worst err / bound %.3f' % (M, n_cep, bi, r, F, max(ratios.values())))
            assert np.all(base['per_frame'][r][:, F:] == 0.0)                       # beyond a row's frames the caller's (zeroed) buffer is untouched
        vs = MU.check_against_yardstick([(base['per_frame'][r], base['summary'][r]) for r in range(len(frames))],
                                        [(yard[r]['per_frame'], yard[r]['summary']) for r in range(len(frames))], ref, bnd, (M, n_cep, bi))
        for k, (g, y, floor) in vs.items():
            q = g / max(y, floor) if max(y, floor) > 0 else 0.0
            PARITY[k]['err_over_floored_yardstick'] = max(PARITY[k]['err_over_floored_yardstick'], q)
            print('M %d n_cep %d batch %d %-10s: device err %.3e yardstick %.3e floor %.3e ratio %.2f (<= %g)' % (M, n_cep, bi, k, g, y, floor, q, MU.FACTOR))
        _same(base, hook, frames)                                                     # the hook's bits
        _same(base, _run(cmp, ap, bp, frames), frames)                                # run to run
        for a_cf in (True, False):
            for b_cf in (True, False):
                for pa, pb in ((P, P), (P + 1, P + 37)):
                    _same(base, _run(cmp, ap, bp, frames, a_cf, b_cf, pa, pb), frames)
        _run(cmp, b, a + np.float32(1.0), [P] * len(frames), per_frame=False)        # leaves the handle's scratch full of another call's values up to P
        bare = _run(cmp, ap, bp, frames, False, True, P + 3, P, per_frame=False)
        assert np.array_equal(MU.bits(bare['summary']), MU.bits(base['summary'])) and np.array_equal(bare['marks'], base['marks']) and 'per_frame' not in bare
        if bi == 0:      # 35 rows: each of the five, seven times, in another order: rows 32 ... 34 fall into the second launch group
            order = [(3 * i + 1) % 5 for i in range(35)]
            big = _run(cmp, ap[order], bp[order], [frames[i] for i in order], True, False)
            for j, i in enumerate(order):
                F = frames[i]
                assert np.array_equal(MU.bits(big['per_frame'][j][:, :F]), MU.bits(base['per_frame'][i][:, :F])), (j, i)
                assert np.array_equal(MU.bits(big['summary'][j]), MU.bits(base['summary'][i])) and np.array_equal(big['marks'][j], base['marks'][i]), (j, i)
            alone = _run(cmp, ap[4:5], bp[4:5], [frames[4]])
            assert np.array_equal(MU.bits(alone['summary'][0]), MU.bits(base['summary'][4])) and np.array_equal(MU.bits(alone['per_frame'][0]), MU.bits(base['per_frame'][4]))
    cmp.close()


def test_identical_inputs_and_the_call_validation_on_a_real_handle():
    from wavenet_vocoder import _ext
    cmp = _ext.MelCompare(80, 3, 100, n_cep=13, unit_db=UNIT, alarm_db=0.0)
    a = MU.mels(3, 80, 100, 4)
    r = _run(cmp, a, a.copy(), [100, 0, 37], True, False)
    assert np.all(r['per_frame'] == 0.0) and np.all(r['summary'] == 0.0) and r['marks'].tolist() == [[0, 0], [-1, 0], [0, 0]]
    x = _dev(a)
    for frames, code in (([100, 0, 101], -2), ([1, -1, 1], -1)):
        with pytest.raises(_ext.WnError) as ei:
            cmp.run(x, x, frames)
        assert ei.value.code == code
    with pytest.raises(_ext.WnError) as ei:
        cmp.run(_dev(MU.mels(4, 80, 100, 4)), _dev(MU.mels(4, 80, 100, 4)), [1, 1, 1, 1])
    assert ei.value.code == -2
    cmp.close()


# ---- ReconstructionCheck.score on a synthetic signal
def _signal(n=22000, seed=11, amp=0.06):
    """seeded noise shaped like speech (white noise through the de-emphasis filter, so that the analysis' pre-emphasis whitens it) under a slow envelope, 1 s.
    At this level datasets.audio.melspectrogram of x and of 0.5 x keeps every channel of every compared frame inside the normalised range: min -2.84 and
    max 2.21 of [-4, 4] (verified on the CPU when this test was written; the floor is -4)."""
    from scipy import signal
    rng = np.random.RandomState(seed)
    t = np.arange(n) / 22050.0
    return ((0.8 + 0.2 * np.sin(2 * np.pi * 2.0 * t)) * amp * signal.lfilter([1], [1, -0.97], rng.randn(n))).astype(np.float32)


def test_the_synthetic_signal_stays_off_the_floor():
    import hparams as H
    from datasets import audio
    hp = H._build()
    for s in (1.0, 0.5):
        m = audio.melspectrogram(audio.preemphasis((np.float32(s) * _signal()).astype(np.float64), hp.preemphasis, hp.preemphasize), hp)[:, :80]
        assert m.min() > -3.5 and m.max() < 3.5


def test_score_on_a_synthetic_signal():
    """c from the same analyzer configuration: the score of x itself is exactly 0.  0.5 x: a power of two scales every linear step of the analysis exactly, so
    the mel moves by magnitude_power * 20 log10(0.5) dB up to the rounding of the logarithm and of the normalisation around it -- at most 8 roundings of values
    up to 100 dB per element, 2 x 8 x 2^-24 x 100 dB = 9.5e-5 dB for the difference of two (TOL) -- which is what bias shows, and l1c / lsdc stay within TOL,
    mcd within sqrt(0.5 n_cep M) TOL (|c_k| <= sum_m |D[k][m]| TOL <= sqrt(M) TOL), each on top of the comparison's own bound.  White noise at three rising
    levels gives strictly rising l1c and mcd.  Ten frames' worth of samples replaced by loud noise put the worst frame inside that span and alarm at least ten
    frames, with alarm_db = twice the worst frame of the lightly disturbed signal."""
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    hp = H._build()
    model = WaveNet(hp)
    x = _signal()
    n, hop, Tc, M = x.size, 275, 80, 80
    chk = model.reconstruction_check(4, n)
    assert chk.unit_db == 12.5 and chk.compare.n_cep == 13
    xd = _dev(x[None])
    c = chk.analyzer.run(xd, [n], channels_first=True)[:, :, :Tc].contiguous()
    table, pf = chk.score(xd, [n], c, per_frame=True)
    assert table.shape == (1, 9) and np.all(table[0, :7] == 0.0) and table[0, 7] == 0 and table[0, 8] == 0 and pf.shape == (1, 6, Tc) and float(pf.abs().max()) == 0.0
    assert np.array_equal(chk.score(xd, [n], c.transpose(1, 2).contiguous(), c_channels_first=False), table)
    # half the amplitude
    half = _dev((np.float32(0.5) * x)[None])
    t = chk.score(half, [n], c)[0]
    a = chk.analyzer.run(half, [n], channels_first=True).cpu().numpy()
    cn = c.cpu().numpy()
    ref = MU.reference(a, cn, [Tc], 13, chk.unit_db, chk.alarm_db)[0]
    bnd = MU.bounds(a, cn, [Tc], 13, chk.unit_db)[0]
    for j in range(7):
        assert abs(float(t[j]) - ref['summary'][j]) <= bnd['summary'][j], j
    TOL = 2 * 8 * MU.U * 100.0
    want = float(hp.magnitude_power) * 20.0 * np.log10(0.5)
    print('0.5 x: bias %.6f dB (want %.6f), l1c %.2e, lsdc %.2e, mcd %.2e dB' % (t[0], want, t[4], t[5], t[3]))
    assert abs(float(t[0]) - want) <= TOL + bnd['summary'][0]
    assert float(t[4]) <= TOL + bnd['summary'][4] and float(t[5]) <= TOL + bnd['summary'][5]
    assert float(t[3]) <= np.sqrt(0.5 * 13 * M) * TOL + bnd['summary'][3]
    # rising noise
    rng = np.random.RandomState(5)
    w = rng.randn(n).astype(np.float32)
    rows = np.stack([x + np.float32(lv) * w for lv in (0.001, 0.01, 0.05)])
    t3 = chk.score(_dev(rows), [n] * 3, c.expand(3, -1, -1).contiguous())
    print('noise levels: l1c %s mcd %s' % (t3[:, 4], t3[:, 3]))
    assert t3[0, 4] < t3[1, 4] < t3[2, 4] and t3[0, 3] < t3[1, 3] < t3[2, 3] and t3[0, 4] > 0
    # a burst
    y = rows[0].copy()
    y[30 * hop:40 * hop] = (0.1 * rng.randn(10 * hop)).astype(np.float32)
    alarm = 2.0 * float(t3[0, 6])
    chk2 = model.reconstruction_check(1, n, alarm_db=alarm)
    tb = chk2.score(_dev(y[None]), [n], c)[0]
    print('burst: worst frame %d at %.2f dB, %d frames over %.3f dB' % (tb[7], tb[6], tb[8], alarm))
    assert 30 <= int(tb[7]) <= 40 and int(tb[8]) >= 10 and float(tb[6]) > alarm
    assert int(chk2.score(_dev(rows[:1]), [n], c)[0, 8]) == 0                      # the lightly disturbed signal alarms nothing at that threshold
    chk.close(); chk2.close()


def _analysis_slack(wav, hp, n_cep):
    """(the float64 numpy analysis [M, frames] of the pre-emphasised signal, slack [7]): how far the seven summary values may move when every element of the
    analysed mel moves by the analysis' own tolerance tol (tests/mel_util.py: 8 x the floored float32 yardstick of this signal), T = unit_db tol: bias, l1 and
    lsd by T (means and an RMS are 1-Lipschitz in the sup norm), l1c, lsdc and worst by 2 T (the bias moves too), mcd by sqrt(0.5 n_cep M) T
    (|c_k| <= sqrt(M) T for a unit-norm DCT row)."""
    import mel_util as MelU
    from datasets import audio
    from wavenet_vocoder import _ext
    x = audio.preemphasis(np.asarray(wav, dtype=np.float64), hp.preemphasis, hp.preemphasize)
    a64 = MelU.reference(x, hp)
    tol, _ = MelU.tolerance(x, hp, ref=a64)
    T = _ext.melcmp_unit_db(hp) * tol
    return a64, np.array([T, T, T, np.sqrt(0.5 * n_cep * int(hp.num_mels)) * T, 2 * T, 2 * T, 2 * T])


# ---- the driver
ROUTES = {'oneshot': '', 'slots': ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,input_type=mulaw-quantize,quantize_channels=256,out_channels=256',
          'fold': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4'}
FRAMES_DRV = (40, 45, 50)


@pytest.mark.parametrize('route', ['oneshot', 'slots', 'fold'])
def test_driver_scores_every_utterance_and_writes_the_same_wavs(tmp_path, route, monkeypatch):
    """Synthesizer.synthesize with mi355_reconstruction_check on, host and device output stage: one TSV row per utterance whose numbers are tests/melcmp_util
    applied to the scored signal's analysis and that utterance's mel, inside the bound; the wav files are byte-identical to the run with the switch off."""
    import hparams as H
    from wavenet_vocoder import _ext, reconstruction as R
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesizer import Synthesizer
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],wavenet_synthesis_batch_size=4' + ROUTES[route])
    rng = np.random.RandomState(5)
    mels = [rng.uniform(-4, 4, size=(FRAMES_DRV[i], 16)).astype(np.float32) for i in range(3)]
    names = ['u%d' % i for i in range(3)]
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(4, max(FRAMES_DRV) * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()
    seen = []
    inner = Synthesizer._reconstruction

    def spy(self, decoded, generated_wavs, cond, lengths, basenames, out_dir):
        table = inner(self, decoded, generated_wavs, cond, lengths, basenames, out_dir)
        if table is not None:
            sig = [decoded[b, :n * 16].float().cpu().numpy() for b, n in enumerate(lengths)] if decoded is not None else [np.asarray(w, np.float32) for w in generated_wavs]
            seen.append((sig, np.array(cond), list(lengths), table))
        return table

    monkeypatch.setattr(Synthesizer, '_reconstruction', spy)

    def run(tag, extra=''):
        hp = H._build(); hp.parse(base + extra)
        out = str(tmp_path / tag); os.makedirs(out)
        s = Synthesizer(); s.load(ckpt, hp)
        files = s.synthesize(mels, None, names, out, None)
        s.model.engine.close()
        for st in s._post_stages.values():
            st.close()
        if s._recon is not None:
            s._recon.close()
        return [open(f, 'rb').read() for f in files], out, hp

    plain, out0, _ = run('plain')
    assert not os.path.exists(os.path.join(out0, 'reconstruction.tsv')) and not seen
    for tag, extra in (('host', ',mi355_reconstruction_check=True'), ('device', ',mi355_reconstruction_check=True,mi355_output_stage=device')):
        got, out, hp = run(tag, extra)
        assert got == plain, tag
        assert sorted(os.listdir(out)) == sorted(os.listdir(out0) + ['reconstruction.tsv'])
        rows = R.read_tsv(os.path.join(out, 'reconstruction.tsv'))
        assert [r['name'] for r in rows] == names and [int(r['frames']) for r in rows] == list(FRAMES_DRV)
        sig, cond, lengths, table = seen.pop()
        assert not seen and lengths == list(FRAMES_DRV) and table.shape == (3, 9)
        an = _ext.MelAnalyzer(hp, 1, max(lengths) * 16, preemphasis=float(hp.preemphasis))
        for u in range(3):
            assert sig[u].shape == (lengths[u] * 16,)
            a = an.run(_dev(sig[u][None]), [sig[u].size], channels_first=True).cpu().numpy()
            cu = np.ascontiguousarray(cond[u:u + 1, :lengths[u]].transpose(0, 2, 1))
            assert np.array_equal(cu[0].T, np.clip(mels[u], -4, 4))
            ref = MU.reference(a, cu, [lengths[u]], 13, 12.5, hp.mi355_reconstruction_alarm_db)[0]
            bnd = MU.bounds(a, cu, [lengths[u]], 13, 12.5)[0]
            for j in range(7):
                assert abs(float(table[u, j]) - ref['summary'][j]) <= bnd['summary'][j], (tag, u, j)
            l1c, bl = ref['per_frame'][4], bnd['per_frame'][4]
            assert l1c[int(table[u, 7])] >= l1c.max() - 2 * bl.max()
            alarm = np.float64(np.float32(hp.mi355_reconstruction_alarm_db))
            assert int(np.sum(l1c > alarm + bl)) <= int(table[u, 8]) <= int(np.sum(l1c >= alarm - bl)), (tag, u)
            assert rows[u]['alarm_frames'] == str(int(table[u, 8])) and rows[u]['worst_frame'] == str(int(table[u, 7]))
            # the same numbers from the numpy float64 analysis of the signal, pre-emphasised as preprocessing does it: what the driver configured is what is meant
            a64, slack = _analysis_slack(sig[u], hp, 13)
            ref64 = MU.reference(a64[None], cu, [lengths[u]], 13, 12.5, hp.mi355_reconstruction_alarm_db)[0]
            for j in range(7):
                assert abs(float(table[u, j]) - ref64['summary'][j]) <= slack[j] + bnd['summary'][j], (tag, u, j, float(table[u, j]), ref64['summary'][j], slack[j])
            assert rows[u] == dict(zip(R.TSV_HEADER, R.tsv_row(names[u], lengths[u], table[u]).split('\t')))
            print('%s %s %s: %s' % (route, tag, names[u], R.tsv_row(names[u], lengths[u], table[u])))
        an.close()


def test_eval_step_writes_the_two_scalars_beside_the_eval_loss(tmp_path):
    """eval_step with the switch on: the generated item is scored against its conditioning (the [0, 1] scaling of normalize_for_wavenet undone) and the two
    scalars equal an independent score of the same tensors; with the switch off the scalars line is what it was"""
    import io
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.train import eval_step
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4]')
    rng = np.random.RandomState(3)
    Tc, hop = 30, 16
    y = torch.from_numpy((0.3 * rng.randn(1, Tc * hop)).astype(np.float32).clip(-0.99, 0.99)).cuda()
    c01 = torch.from_numpy(rng.uniform(0, 1, size=(1, 16, Tc)).astype(np.float32)).cuda()
    plots, wavs = str(tmp_path / 'plots'), str(tmp_path / 'wavs')
    os.makedirs(plots); os.makedirs(wavs)
    lines = {}
    for on in (False, True):
        hp = H._build(); hp.parse(base + (',mi355_reconstruction_check=True' if on else ''))
        model = WaveNet(hp)
        model.build(1, Tc * hop)
        out = io.StringIO()
        eval_step(model, (None, y, [Tc * hop], c01, None), 7, plots, wavs, out, hp, 'WaveNet')
        lines[on] = json.loads(out.getvalue())
        if on:
            chk = model.reconstruction_check(1, Tc * hop)
            t = chk.score(model.tower_y_hat[0].float().reshape(1, -1).contiguous(), [Tc * hop], (c01 * 8.0 - 4.0).contiguous())[0]
            chk.close()
        model.engine.close()
    pre = 'Wavenet_eval_model/eval_stats/wavenet_eval_'
    assert set(lines[False]) == {'step', pre + 'loss'}
    assert set(lines[True]) == {'step', pre + 'loss', pre + 'reconstruction_l1c_db', pre + 'reconstruction_mcd_db'}
    assert lines[True][pre + 'reconstruction_l1c_db'] == float(t[4]) > 0 and lines[True][pre + 'reconstruction_mcd_db'] == float(t[3]) > 0


def test_command_line_on_the_device_equals_its_host_evaluation(tmp_path, capsys):
    """python -m wavenet_vocoder.reconstruction without --host (score_device: two pairs of different length in one padded batch) against the same call with
    --host (numpy float64 analysis, the host hook): every summary value within the analysis' own tolerance (_analysis_slack) plus the comparison's bound"""
    from datasets import audio
    from scipy.io import wavfile
    from hip_util import make_hp
    from wavenet_vocoder import reconstruction as R
    over = 'num_mels=20,cin_channels=20,n_fft=256,hop_size=64,win_size=256,sample_rate=8000,fmin=50,fmax=3800'
    hp = make_hp(num_mels=20, cin_channels=20, n_fft=256, hop_size=64, win_size=256, sample_rate=8000, fmin=50, fmax=3800)
    rng = np.random.RandomState(1)
    wav_dir, mel_dir = str(tmp_path / 'wavs'), str(tmp_path / 'mels')
    os.makedirs(wav_dir); os.makedirs(mel_dir)
    for i, (frames, noise) in enumerate(((30, 0.0), (22, 0.2))):
        x = 0.3 * np.sin(2 * np.pi * 440 * np.arange(64 * frames) / 8000.0) + 0.05 * rng.randn(64 * frames)
        pcm = (x * 32767 / np.abs(x).max()).astype(np.int16)
        mel = audio.melspectrogram(audio.preemphasis(pcm.astype(np.float64) / 32768.0, hp.preemphasis, hp.preemphasize), hp).T[:frames]
        if noise:
            pcm = np.clip(pcm + noise * 32767 * rng.randn(pcm.size), -32767, 32767).astype(np.int16)
        wavfile.write(os.path.join(wav_dir, 'wavenet-audio-mel-u%d.wav' % i), 8000, pcm)
        np.save(os.path.join(mel_dir, 'mel-u%d.npy' % i), mel.astype(np.float32))
    args = ['--wavs', wav_dir, '--mels', mel_dir, '--hparams', over]
    names, frames, dev = R.main(args)
    names_h, frames_h, host = R.main(args + ['--host'])
    capsys.readouterr()
    assert names == names_h == ['mel-u0', 'mel-u1'] and frames == frames_h == [30, 22]
    for i in range(2):
        wav = audio.load_wav(os.path.join(wav_dir, 'wavenet-audio-mel-u%d.wav' % i), sr=8000)
        mel = np.load(os.path.join(mel_dir, 'mel-u%d.npy' % i))
        a64, slack = _analysis_slack(wav, hp, 13)
        bnd = MU.bounds(a64[None], np.ascontiguousarray(mel.T)[None], [frames[i]], 13, 12.5)[0]['summary']
        for j in range(7):
            print('pair %d %-8s device %.6f host %.6f (allowed %.2e)' % (i, R.COLUMNS[j], dev[i, j], host[i, j], slack[j] + 2 * bnd[j]))
            assert abs(float(dev[i, j]) - float(host[i, j])) <= slack[j] + 2 * bnd[j], (i, j)
    assert dev[0, 8] == host[0, 8] == 0 and dev[1, 4] > 1.0
