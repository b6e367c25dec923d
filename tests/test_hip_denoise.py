"""Spectral denoiser on the device (csrc/wn_denoise.hip): every output sample of wn_denoise_run against the float64 reference of tests/denoise_ref.py applied
to the device's own inputs and profile, under the one rule of that file -- per row 8 x max(yardstick of the row, 2^-23 max|x| of the row), no element left
out -- over (64, 16) (33 bins: one bin group), (96, 20) (no power of two, hop does not divide n_fft) and one case of (1024, 256); row lengths 0, 1, 15, 16,
17, n_fft / 2 - 1, n_fft, 32 hop - 1, 32 hop, 32 hop + 1, 64 hop + 1 and 2000 in ragged batches of 3 with a pitch beyond the longest row and NaN beyond every
row's length; six kinds of signal at strengths 0, 0.5, 1 and 4; every bin of a fitted profile under the same rule; the bit-for-bit identities; and the
drivers on a tiny model.  WN_DENOISE_PARITY_OUT=<file> makes the session write the worst error / bound per geometry and kind there
(profiles/denoise_parity.json is such a file)."""
import json
import os

import numpy as np
import pytest
import torch

import denoise_ref as R

pytestmark = pytest.mark.gpu
PARITY = {}
SENTINEL = -7.25


@pytest.fixture(scope='module', autouse=True)
def parity_record():
    yield
    path = os.environ.get('WN_DENOISE_PARITY_OUT')
    if path and PARITY:
        with open(path, 'w') as f:
            json.dump({'what': 'wn_denoise_run / wn_denoise_fit on an MI355X against the float64 reference of tests/denoise_ref.py: worst |out - ref| / bound over every sample '
                               'of every row, bound = 8 x max(float32 yardstick of the row, 2^-23 max|x| of the row); yardstick_scale = the worst yardstick / (2^-23 max|x|)',
                       'cases': PARITY}, f, indent=1, sort_keys=True)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _denoiser(name, rows, max_samples):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    d = _ext.SpectralDenoiser(n_fft, hop, rows, max_samples)
    d.profile = R.noise_profile(n_fft, hop)
    return d


def _apply(d, wav, lengths, strength, pitch_out=None):
    """one run into a sentinel-filled output of its own pitch -> numpy"""
    out = torch.full((len(lengths), pitch_out or wav.shape[1]), SENTINEL, device='cuda')
    d.apply(_dev(wav), lengths, strength, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _batches(n_fft, hop):
    ls = R.lengths_of(n_fft, hop)
    order = [0, 11, 5, 1, 8, 6, 2, 10, 3, 4, 7, 9]          # every batch mixes short and long rows
    ls = [ls[i] for i in order]
    return [ls[i:i + 3] for i in range(0, 12, 3)]


@pytest.mark.parametrize('kind', R.KINDS)
@pytest.mark.parametrize('name', ['A', 'B'])
def test_every_sample_against_float64(name, kind):
    n_fft, hop = R.GEOMETRIES[name]
    d = _denoiser(name, 3, 2000)
    prof = d.profile
    worst = scale = 0.0
    for s in R.STRENGTHS:
        for i, lens in enumerate(_batches(n_fft, hop)):
            wav = R.batch(kind, lens, 100 + i, n_fft)
            got = _apply(d, wav, lens, s, pitch_out=wav.shape[1] + 3)
            for b, n in enumerate(lens):
                assert np.all(got[b, n:] == SENTINEL), (s, lens, b)          # nothing beyond a row's length is written
                if kind == 'zeros':
                    assert np.all(got[b, :n] == 0.0)
            w, sc = R.check_rows(got, wav, lens, prof, s, n_fft, hop)
            print('%s %-8s strength %.1f lengths %r: worst error / bound %.3f' % (name, kind, s, lens, w))
            worst, scale = max(worst, w), max(scale, sc)
    PARITY['%s/%s' % (name, kind)] = {'n_fft': n_fft, 'hop': hop, 'worst_error_over_bound': worst, 'yardstick_scale': scale}
    d.close()
    assert worst <= 1.0


def test_production_geometry_three_rows():
    n_fft, hop = R.GEOMETRIES['P']
    lens = [6000, 16 * hop + 1, 777]
    d = _denoiser('P', 3, 6000)
    prof = d.profile
    worst = scale = 0.0
    wav = R.batch('tone', lens, 7, n_fft)
    for s in (0.0, 1.0):
        got = _apply(d, wav, lens, s)
        w, sc = R.check_rows(got, wav, lens, prof, s, n_fft, hop)
        print('P tone strength %.1f: worst error / bound %.3f, yardstick %.2f x 2^-23 max|x|' % (s, w, sc))
        worst, scale = max(worst, w), max(scale, sc)
    PARITY['P/tone'] = {'n_fft': n_fft, 'hop': hop, 'worst_error_over_bound': worst, 'yardstick_scale': scale}
    d.close()
    assert worst <= 1.0


@pytest.mark.parametrize('name', ['A', 'B', 'P'])
def test_fit_every_bin_against_float64(name):
    n_fft, hop = R.GEOMETRIES[name]
    lens = [3 * n_fft + 5, n_fft - 1, 40 * hop + 3] if name != 'P' else [5000, 0, 33 * hop]
    rows = [R.signal('tone' if i == 0 else 'straddle', n, 9 + i, n_fft) for i, n in enumerate(lens)]
    wav = np.full((3, max(lens) + 5), np.nan, np.float32)
    for i, r in enumerate(rows):
        wav[i, :len(r)] = r
    from wavenet_vocoder import _ext
    d = _ext.SpectralDenoiser(n_fft, hop, 3, max(lens))
    d.fit(_dev(wav), lens)
    p1 = d.profile
    d.fit(_dev(wav), lens)
    assert np.array_equal(p1, d.profile)                                  # run to run
    w = R.check_profile(p1, rows, n_fft, hop)
    PARITY['%s/fit' % name] = {'n_fft': n_fft, 'hop': hop, 'worst_error_over_bound': w}
    assert w <= 1.0
    with pytest.raises(_ext.WnError) as e:
        d.fit(_dev(wav), [n_fft - 1, 0, 5])
    assert e.value.code == -2
    assert np.array_equal(p1, d.profile)                                  # a refused fit leaves the profile alone
    d.close()


@pytest.mark.parametrize('name', ['A', 'B'])
def test_a_rows_bits_do_not_depend_on_the_call(name):
    """run to run, a row alone against the same row at another index of a batch, other pitches, in == out"""
    n_fft, hop = R.GEOMETRIES[name]
    lens = [32 * hop + 1, 17, 64 * hop + 1]
    d = _denoiser(name, 3, 2000)
    wav = R.batch('tone', lens, 31, n_fft, fill=0.25)
    a = _apply(d, wav, lens, 1.0)
    assert np.array_equal(a, _apply(d, wav, lens, 1.0))
    for b, n in enumerate(lens):
        alone = np.full((1, n + 1), 0.5, np.float32); alone[0, :n] = wav[b, :n]
        assert np.array_equal(_apply(d, alone, [n], 1.0, pitch_out=n + 9)[0, :n], a[b, :n]), b
    rev = np.ascontiguousarray(wav[::-1])
    r = _apply(d, rev, lens[::-1], 1.0)
    for b, n in enumerate(lens):
        assert np.array_equal(r[2 - b, :n], a[b, :n])
    t = _dev(wav)
    d.apply(t, lens, 1.0, out=t)
    torch.cuda.synchronize()
    t = t.cpu().numpy()
    for b, n in enumerate(lens):
        assert np.array_equal(t[b, :n], a[b, :n]) and np.all(t[b, n:] == 0.25)
    d.close()


def test_a_batch_beyond_one_launch_group():
    n_fft, hop = R.GEOMETRIES['A']
    B = 70
    lens = [(37 * b) % 300 for b in range(B)]
    d = _denoiser('A', B, 300)
    wav = R.batch('straddle', lens, 3, n_fft)
    got = _apply(d, wav, lens, 0.5)
    w, _ = R.check_rows(got, wav, lens, d.profile, 0.5, n_fft, hop)
    assert w <= 1.0
    one = _denoiser('A', 1, 300)
    assert np.array_equal(_apply(one, wav[69:70], lens[69:], 0.5)[0, :lens[69]], got[69, :lens[69]])
    d.close(); one.close()


# ---- drivers: a tiny model through Synthesizer
TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,wavenet_synthesis_batch_size=2,mi355_output_denoise_fft=64,mi355_output_denoise_hop=16,'
        'mi355_output_denoise_profile_frames=12,mi355_reconstruction_check=True,mi355_pitch_check=True,mi355_pitch_window=64,mi355_pitch_fmin=552,'
        'mi355_pitch_fmax=4410')
ROUTES = {'oneshot': '', 'oneshot-device': ',mi355_output_stage=device', 'wide': ',mi355_synthesis_wide_rows=40',
          'slots-device': ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,mi355_output_stage=device',
          'slots': ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,input_type=mulaw-quantize,quantize_channels=256,out_channels=256',
          'fold': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4',
          'fold-device': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4,mi355_output_stage=device'}


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_synthesizer_writes_the_denoised_wave(tmp_path, route):
    """mi355_output_denoise=0.5: the wav written is the chain applied by hand -- the denoiser's own apply at the fitted profile, then the output stage -- to the
    decoded samples the route produced, and the reconstruction.tsv and pitch.tsv rows are those of the denoised wave (the waveform handed to both checks IS
    the denoised one); 0.0: byte-identical files to a run without the key, and
    no handle exists"""
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder import pitch as PT
    from wavenet_vocoder import reconstruction as RC
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesizer import Synthesizer
    base = TINY + ROUTES[route]
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(2, 800)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()
    rs = np.random.RandomState(5)
    mels = [rs.uniform(-3.5, 3.5, size=(F, 16)).astype(np.float32) for F in (20, 31)]
    seen = []
    inner = Synthesizer._denoise

    def spy(self, rows, lengths):
        if self._denoiser is None:          # off: the rows come back as they are, the very object
            assert inner(self, rows, lengths) is rows
            return rows
        before = rows.clone()
        out = inner(self, rows, lengths)
        seen.append((before.cpu().numpy(), out.cpu().numpy(), list(lengths)))
        return out

    refs = [0.5 * np.sin(2 * np.pi * np.arange(F * 16) / 23.0).astype(np.float32) for F in (20, 31)]          # the recordings of the pitch check
    scored = {}
    inner_p, inner_r = Synthesizer._pitch, Synthesizer._reconstruction

    def grab(what, inner_fn):
        def f(self, decoded, generated_wavs, *a):
            if self._denoiser is not None:
                scored[what] = [decoded[b].float().cpu().numpy() for b in range(2)] if decoded is not None else [np.asarray(w, np.float32) for w in generated_wavs]
            return inner_fn(self, decoded, generated_wavs, *a)
        return f

    files = {}
    for tag, extra in (('none', ''), ('zero', ',mi355_output_denoise=0.0'), ('half', ',mi355_output_denoise=0.5')):
        hp = H._build(); hp.parse(base + extra)
        out = str(tmp_path / tag); os.makedirs(out)
        syn = Synthesizer()
        syn.load(ckpt, hp)
        syn.pitch_references = [r.copy() for r in refs]
        Synthesizer._denoise, Synthesizer._pitch, Synthesizer._reconstruction = spy, grab('pitch', inner_p), grab('reconstruction', inner_r)
        try:
            syn.synthesize(mels, None, ['a', 'b'], out, None)
        finally:
            Synthesizer._denoise, Synthesizer._pitch, Synthesizer._reconstruction = inner, inner_p, inner_r
        files[tag] = {n: open(os.path.join(out, n), 'rb').read() for n in sorted(os.listdir(out))}
        if tag != 'half':
            assert syn._denoiser is None and not seen
        else:
            prof, dn = syn._denoiser.profile, syn._denoiser
    assert files['none'] == files['zero'] and sorted(files['none']) == ['pitch.tsv', 'reconstruction.tsv', 'wavenet-audio-a.wav', 'wavenet-audio-b.wav']
    assert seen and np.all(prof >= 0) and prof.max() > 0
    utts = [(before[b, :n], after[b, :n]) for before, after, lens in seen for b, n in enumerate(lens)]          # per utterance, in order (a route may denoise row by row)
    lens = [20 * 16, 31 * 16]
    assert [len(x) for x, _ in utts] == lens
    device, k = Synthesizer._output_mode(syn)
    for (x, y), n, name in zip(utts, lens, ('a', 'b')):
        assert np.array_equal(dn.apply(_dev(x[None]), [n], 0.5).cpu().numpy()[0], y)          # the Python chain by hand: the same bits
        w, _ = R.check_rows(y[None], x[None], [n], prof, 0.5, 64, 16)
        assert w <= 1.0
        if device:          # the written file: the existing output stage on the denoised row
            want = syn._stage(1, 'raw', k).finish(_dev(y[None]), [n])[1].cpu().numpy()[0]
        else:
            want = (y * (32767 / max(0.01, float(np.max(np.abs(y)))))).astype(np.int16)
        sr, data = wavfile.read(str(tmp_path / 'half' / ('wavenet-audio-%s.wav' % name)))
        assert np.array_equal(data, want), name
    assert files['half']['wavenet-audio-b.wav'] != files['none']['wavenet-audio-b.wav']
    # the check scored the denoised wave
    rows = RC.read_tsv(str(tmp_path / 'half' / 'reconstruction.tsv'))
    chk = syn.model.reconstruction_check(2, max(lens))
    after = np.zeros((2, max(lens)), np.float32)
    for b, (_, y) in enumerate(utts):
        after[b, :lens[b]] = y
    cond = np.stack([np.pad(m, [(0, 31 - len(m)), (0, 0)], constant_values=-4.0) for m in mels]).astype(np.float32)
    table = chk.score(_dev(after), lens, _dev(cond), frames=[20, 31], c_channels_first=False)
    for b, name in enumerate(('a', 'b')):
        assert rows[b] == dict(zip(RC.TSV_HEADER, RC.tsv_row(name, [20, 31][b], table[b]).split('\t')))
    assert files['half']['reconstruction.tsv'] != files['none']['reconstruction.tsv']
    # ... and so did the pitch check: both were handed the denoised rows, and pitch.tsv holds PitchCheck.score of them against the recordings
    for what in ('pitch', 'reconstruction'):
        for b, (_, y) in enumerate(utts):
            assert np.array_equal(scored[what][b][:lens[b]], y), (what, b)
    prow = PT.read_tsv(str(tmp_path / 'half' / 'pitch.tsv'))
    pchk = syn.model.pitch_check(2, max(lens))
    ref = np.zeros((2, max(lens)), np.float32)
    for b, r in enumerate(refs):
        ref[b, :lens[b]] = r
    ptable = pchk.score(_dev(after), _dev(ref), lens)
    assert len(prow) == 2
    for b, name in enumerate(('a', 'b')):
        assert prow[b] == dict(zip(PT.TSV_HEADER, PT.tsv_row(name, ptable[b]).split('\t')))


def test_eval_step_writes_and_scores_the_denoised_item(tmp_path):
    """eval_step with mi355_output_denoise=0.5 on a real model: the item is denoised by the model's own handle, fitted once; the pred wav is the denoised
    item and the scalars of both checks equal an independent score of it; with the key at 0 the row and the wav are those of a run without the key"""
    import io
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder.models.wavenet import OutputDenoiser, WaveNet
    from wavenet_vocoder.train import eval_step
    Tc, hop = 30, 16
    y = torch.from_numpy((0.5 * np.sin(2 * np.pi * np.arange(Tc * hop) / 23.0)).astype(np.float32)[None]).cuda()
    c01 = torch.from_numpy(np.random.RandomState(3).uniform(0, 1, size=(1, 16, Tc)).astype(np.float32)).cuda()
    seen, fits = [], []
    inner, inner_fit = OutputDenoiser.apply, OutputDenoiser.fit_from_model

    def spy(self, wav, lengths, strength, out=None):
        before = wav.clone()
        res = inner(self, wav, lengths, strength, out=out)
        seen.append((before.cpu().numpy(), res.cpu().numpy(), strength))
        return res

    def spy_fit(self, *a, **k):
        fits.append(1)
        return inner_fit(self, *a, **k)

    lines, pcm = {}, {}
    OutputDenoiser.apply, OutputDenoiser.fit_from_model = spy, spy_fit
    try:
        for tag, extra in (('none', ''), ('zero', ',mi355_output_denoise=0.0'), ('half', ',mi355_output_denoise=0.5')):
            d = str(tmp_path / tag); os.makedirs(d)
            hp = H._build(); hp.parse(TINY + extra)
            model = WaveNet(hp)
            model.build(1, Tc * hop)
            for step in (7, 8):
                out = io.StringIO()
                eval_step(model, (None, y, [Tc * hop], c01, None), step, d, d, out, hp, 'WaveNet')
            lines[tag] = json.loads(out.getvalue())
            pcm[tag] = wavfile.read(os.path.join(d, 'step-8-pred.wav'))[1]
            if tag == 'half':
                item = model.tower_y_hat[0].float().reshape(1, -1).contiguous()
                rt = model.reconstruction_check(1, Tc * hop).score(item, [Tc * hop], model.tower_eval_c[0].float().unsqueeze(0) * 8 - 4, frames=[Tc])[0]
                pt = model.pitch_check(1, Tc * hop).score(item, model.tower_y_target[0].float().reshape(1, -1).contiguous(), [Tc * hop])[0]
                prof = model._eval_denoiser.profile
            else:
                assert getattr(model, '_eval_denoiser', None) is None
            model.engine.close()
    finally:
        OutputDenoiser.apply, OutputDenoiser.fit_from_model = inner, inner_fit
    assert lines['none'] == lines['zero'] and np.array_equal(pcm['none'], pcm['zero'])
    assert len(fits) == 1 and len(seen) == 2 and seen[1][2] == 0.5                     # fitted once per model, applied at every eval
    before, after, _ = seen[1]
    w, _ = R.check_rows(after, before, [Tc * hop], prof, 0.5, 64, 16)
    assert w <= 1.0 and np.array_equal(after, item.cpu().numpy())
    a = after[0]
    assert np.array_equal(pcm['half'], (a * (32767 / max(0.01, float(np.max(np.abs(a)))))).astype(np.int16))
    pre = 'Wavenet_eval_model/eval_stats/wavenet_eval_'
    assert lines['half'][pre + 'reconstruction_l1c_db'] == float(rt[4]) and lines['half'][pre + 'reconstruction_mcd_db'] == float(rt[3])
    assert lines['half'][pre + 'f0_rmse_cents'] == float(pt[6]) and lines['half'][pre + 'vuv_error'] == float(pt[4]) and lines['half'][pre + 'gpe'] == float(pt[5])
    assert lines['half'][pre + 'loss'] == lines['none'][pre + 'loss']
