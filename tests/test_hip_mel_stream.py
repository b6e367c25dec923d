"""Streaming mel analysis on the GPU (csrc/wn_mel_stream.hip): rows pushed under three schedules equal MelAnalyzer.run of the whole row BIT FOR BIT in both
layouts, with pre-emphasis and per-row gains; n_out follows the rule and nothing is written beyond it; restart, 65 rows, rows left alone, one parity case
against the float64 reference, two runs; and LiveVocoder on a tiny untrained model against a SlotSession fed the whole analyse_wavs mels."""
import os

import numpy as np
import pytest
import torch

import mel_stream_ref as M
import mel_util

pytestmark = pytest.mark.gpu

PRE = 0.97
SENTINEL = 12345.0


def _hp(name):
    if name == 'odd_win':      # Hl != Hr: not one of mel_util.CONFIGS
        n_fft, win, hop = M.GEOMETRIES[name]
        return mel_util.mel_hparams(n_fft=n_fft, win_size=win, hop_size=hop)
    return mel_util.mel_hparams(**({} if name == 'default' else dict(mel_util.CONFIGS)[name]))


def _geom(hp):
    from datasets import audio
    return int(hp.n_fft), int(hp.win_size), int(audio.get_hop_size(hp))


def _rows(hp):
    """the rows of the issue: lengths around the tile edges, the signal kinds cycling, gains != 1"""
    hop = _geom(hp)[2]
    lens = [1, hop - 1, 3 * hop, 31 * hop, 32 * hop + 5, 33 * hop, 70 * hop + hop // 2]
    wavs = [mel_util.make_signal(mel_util.KINDS[i % len(mel_util.KINDS)], n, 300 + i, hp.sample_rate) for i, n in enumerate(lens)]
    gains = [float(np.float32(0.5 + 0.17 * i)) for i in range(len(lens))]
    return wavs, gains


_whole = {}


def _reference(name, cf):
    """MelAnalyzer.run of the whole rows, once per geometry and layout: a list of [num_mels, F_b] / [F_b, num_mels] arrays"""
    from wavenet_vocoder import _ext
    if (name, cf) not in _whole:
        hp = _hp(name)
        wavs, gains = _rows(hp)
        an = _ext.MelAnalyzer(hp, len(wavs), max(len(w) for w in wavs), preemphasis=PRE)
        full = mel_util.run_analyzer(an, wavs, channels_first=cf, gain=torch.tensor(gains, dtype=torch.float32).cuda())
        an.close()
        hop = _geom(hp)[2]
        _whole[(name, cf)] = [np.ascontiguousarray(full[b, :, :1 + len(w) // hop] if cf else full[b, :1 + len(w) // hop]) for b, w in enumerate(wavs)]
    return _whole[(name, cf)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _push_all(ms, geom, wavs, gains, pushes, cf, max_push):
    """the rows through the schedule: checks n_out against the rule and the sentinel beyond it at every push; -> the frames of every row since its last restart"""
    B, nm = len(wavs), ms.num_mels
    S, F = [0] * B, [0] * B
    got = [[] for _ in range(B)]
    pos = [0] * B
    pitch = max_push // geom[2] + 6
    for n, r, f in pushes:
        blk = np.full((B, max_push), np.nan, np.float32)      # what lies beyond n[b] must never be read
        for b in range(B):
            if r[b]:
                pos[b], S[b], F[b], got[b] = 0, 0, 0, []
            blk[b, :n[b]] = wavs[b][pos[b]:pos[b] + n[b]]
            pos[b] += n[b]
        out = torch.full((B, nm, pitch) if cf else (B, pitch, nm), SENTINEL, dtype=torch.float32, device='cuda')
        _, n_out = ms.push(torch.from_numpy(blk).cuda(), n=n, restart=r, final=f, gain=gains, channels_first=cf, out=out)
        o = out.cpu().numpy()
        for b in range(B):
            if n[b] > 0 or f[b]:
                S[b] += n[b]
                F1 = M.ready(*geom, S[b], bool(f[b]))
            else:
                F1 = F[b]
            assert n_out[b] == F1 - F[b], (b, n_out[b], F1, F[b])
            F[b] = F1
            fr = o[b, :, :n_out[b]] if cf else o[b, :n_out[b]]
            rest = o[b, :, n_out[b]:] if cf else o[b, n_out[b]:]
            assert np.all(rest == SENTINEL), b
            got[b].append(fr)
    return [np.concatenate(g, axis=1 if cf else 0) for g in got]


def _schedule(kind, geom, lens, max_push, seed=0):
    if kind == 'whole':
        return M.whole_schedule(lens, max_push)
    if kind == 'cycled':
        return M.cycled_schedule(lens, max_push, M.fixed_cuts(*geom, max_push))
    return M.random_schedule(np.random.RandomState(seed), lens, max_push, M.fixed_cuts(*geom, max_push))


@pytest.mark.parametrize('cf', [True, False])
@pytest.mark.parametrize('kind', ['whole', 'cycled', 'random'])
@pytest.mark.parametrize('name', ['default', 'fft1024', 'fft800', 'odd_win'])
def test_streamed_equals_run_bit_for_bit(name, kind, cf):
    """max_push = 40 hop as the issue sets it; the row of 70.5 hop does not fit one push, so under 'whole' it goes in pushes of max_push, the last one final"""
    from wavenet_vocoder import _ext
    hp = _hp(name)
    geom = _geom(hp)
    wavs, gains = _rows(hp)
    max_push = 40 * geom[2]
    ref = _reference(name, cf)
    ms = _ext.MelStream(hp, len(wavs), max_push, preemphasis=PRE)
    got = _push_all(ms, geom, wavs, gains, _schedule(kind, geom, [len(w) for w in wavs], max_push, seed=11), cf, max_push)
    ms.close()
    for b, (g, w) in enumerate(zip(got, ref)):
        assert g.shape == w.shape, (b, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), (name, kind, cf, b, int(np.sum(_bits(g) != _bits(w))))


def test_a_row_restarted_mid_session_inherits_nothing():
    """row 1 is cut off after 5 hop + 3 samples of one signal (no final) and restarted with its own signal and gain; row 0 ends and is restarted with another
    signal: both equal a fresh handle's output"""
    from wavenet_vocoder import _ext
    hp = _hp('default')
    geom = _geom(hp)
    hop = geom[2]
    max_push = 40 * hop
    a = mel_util.make_signal('harmonic', 9 * hop + 7, 1)
    b = mel_util.make_signal('noise', 12 * hop + 1, 2)
    c = mel_util.make_signal('sine', 6 * hop, 3)
    ms = _ext.MelStream(hp, 2, max_push, preemphasis=PRE)
    fresh = _ext.MelStream(hp, 2, max_push, preemphasis=PRE)
    want = _push_all(fresh, geom, [c, b], [0.7, 1.9], M.whole_schedule([len(c), len(b)], max_push), True, max_push)
    # first lives of the two rows: row 0 = a whole and final (gain 3), row 1 = the head of a, not final (gain 0.25)
    first = M.cycled_schedule([len(a), 5 * hop + 3], max_push, [2 * hop + 1])
    first = [(n, r, [f[0], 0]) for n, r, f in first]
    _push_all(ms, geom, [a, a], [3.0, 0.25], first, True, max_push)
    sched = M.random_schedule(np.random.RandomState(5), [len(c), len(b)], max_push, M.fixed_cuts(*geom, max_push))
    got = _push_all(ms, geom, [c, b], [0.7, 1.9], sched, True, max_push)
    for r in range(2):
        assert np.array_equal(_bits(got[r]), _bits(want[r])), r
    ms.close(); fresh.close()


def test_65_rows_cross_the_launch_group_edge():
    from wavenet_vocoder import _ext
    hp = _hp('fft800')
    geom = _geom(hp)
    hop = geom[2]
    max_push = 3 * hop
    lens = [1 + (37 * i) % (5 * hop) for i in range(65)]
    wavs = [mel_util.make_signal(mel_util.KINDS[i % 3], n, 500 + i, hp.sample_rate) for i, n in enumerate(lens)]
    gains = [float(np.float32(0.4 + 0.03 * i)) for i in range(65)]
    an = _ext.MelAnalyzer(hp, 65, max(lens), preemphasis=PRE)
    full = mel_util.run_analyzer(an, wavs, channels_first=True, gain=torch.tensor(gains, dtype=torch.float32).cuda())
    an.close()
    ms = _ext.MelStream(hp, 65, max_push, preemphasis=PRE)
    got = _push_all(ms, geom, wavs, gains, M.random_schedule(np.random.RandomState(3), lens, max_push, [1, hop, max_push]), True, max_push)
    ms.close()
    for b in range(65):
        assert np.array_equal(_bits(got[b]), _bits(full[b, :, :1 + lens[b] // hop])), b


def test_a_row_left_alone_is_unchanged():
    """row 0 waits (n = 0, neither restarted nor final) through pushes that move row 1, then goes on: its frames are those of an undisturbed run"""
    from wavenet_vocoder import _ext
    hp = _hp('fft1024')
    geom = _geom(hp)
    hop = geom[2]
    max_push = 40 * hop
    x = [mel_util.make_signal('harmonic', 7 * hop + 9, 7), mel_util.make_signal('noise', 20 * hop, 8)]
    pushes = [([3 * hop + 1, hop], [1, 1], [0, 0]), ([0, 5 * hop], [0, 0], [0, 0]), ([0, 3], [0, 0], [0, 0]), ([0, 14 * hop - 3], [0, 0], [0, 1]),
              ([4 * hop + 8, 0], [0, 0], [1, 0])]
    ms = _ext.MelStream(hp, 2, max_push, preemphasis=PRE)
    got = _push_all(ms, geom, x, [1.5, 0.5], pushes, True, max_push)
    alone = _ext.MelStream(hp, 1, max_push, preemphasis=PRE)
    want = _push_all(alone, geom, x[:1], [1.5], [([len(x[0])], [1], [1])], True, max_push)
    assert np.array_equal(_bits(got[0]), _bits(want[0]))
    ms.close(); alone.close()


def test_parity_against_the_float64_reference():
    """the streamed frames of one row against mel_util.reference inside mel_util.tolerance (its own bound and factor), default geometry, no pre-emphasis, gain 1"""
    from wavenet_vocoder import _ext
    hp = _hp('default')
    geom = _geom(hp)
    hop = geom[2]
    w = mel_util.make_signal('harmonic', 40 * hop + 19, 21, hp.sample_rate)
    ref = mel_util.reference(w, hp)
    tol, yard = mel_util.tolerance(w, hp, ref)
    ms = _ext.MelStream(hp, 1, 8 * hop)
    got = _push_all(ms, geom, [w], None, M.cycled_schedule([len(w)], 8 * hop, [8 * hop, 3, 2 * hop + 1]), True, 8 * hop)[0]
    ms.close()
    err = float(np.max(np.abs(got.astype(np.float64) - ref)))
    print('streamed mel parity: yardstick=%.3e device=%.3e tolerance=%.3e' % (yard, err, tol))
    assert got.shape == ref.shape and err <= tol


def test_two_runs_are_bit_identical():
    from wavenet_vocoder import _ext
    hp = _hp('default')
    geom = _geom(hp)
    wavs, gains = _rows(hp)
    max_push = 40 * geom[2]
    runs = []
    for _ in range(2):
        ms = _ext.MelStream(hp, len(wavs), max_push, preemphasis=PRE)
        runs.append(_push_all(ms, geom, wavs, gains, _schedule('random', geom, [len(w) for w in wavs], max_push, seed=4), False, max_push))
        ms.close()
    for a, b in zip(*runs):
        assert np.array_equal(_bits(a), _bits(b))


# ---- LiveVocoder on a tiny untrained model (the smallest configuration of the slot tests: hop 16)
TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_output_denoise_fft=64,mi355_output_denoise_hop=16')
LIVE_FRAMES = (9, 14, 20)


def _recordings(path, hp, lens):
    """seeded recordings as int16 wav files -> (paths, the float32 signals load_wav returns)"""
    from scipy.io import wavfile
    os.makedirs(path, exist_ok=True)
    paths, sigs = [], []
    for i, n in enumerate(lens):
        x = mel_util.make_signal(('harmonic', 'noise', 'sine')[i % 3], n, 40 + i, hp.sample_rate)
        q = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
        paths.append(os.path.join(path, 'rec%d.wav' % i))
        wavfile.write(paths[-1], hp.sample_rate, q)
        sigs.append(q.astype(np.float32) / 32768.0)
    return paths, sigs


@pytest.mark.parametrize('chunk', [700, 50])
def test_live_vocoder_equals_a_slot_session_fed_the_whole_mels(tmp_path, chunk):
    """three recordings of 9, 14 and 20 frames in chunks of 700 samples (at hop 16 a recording fits one chunk; chunks of 50 samples cut every recording into
    several pushes): samples and playable chunks (output stage and denoiser on) bit-equal to a SlotSession fed the whole analyse_wavs mels, same slots and seeds"""
    import hparams as H
    import denoise_ref as D
    from wavenet_vocoder import live
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesize import analyse_wavs
    hp = H._build(); hp.parse(TINY)
    hop = 16
    lens = [(f - 1) * hop + 5 + 3 * i for i, f in enumerate(LIVE_FRAMES)]
    paths, sigs = _recordings(str(tmp_path / 'wavs'), hp, lens)
    mels = analyse_wavs(paths, hp)
    assert [m.shape for m in mels] == [(f, 16) for f in LIVE_FRAMES]
    model = WaveNet(hp)
    model.build(3, 32 * hop)
    k = float(hp.preemphasis) if hp.preemphasize else 0.0

    def handles():
        ds = model.stream_denoiser(3, 32 * hop)
        ds.set_profile(0.05 * D.noise_profile(64, 16))
        return dict(post=model.output_stage(3, in_type='raw'), post_output='float', denoise=ds, denoise_strength=0.25)
    # the reference: one session, the whole mels in one push
    kw = handles()
    sess = model.slots(3)
    for b in range(3):
        sess.open(b, seed=70 + b)
    c = {b: (live.condition(hp, torch.from_numpy(np.ascontiguousarray(mels[b].T)).cuda()), True) for b in range(3)}
    want = sess.push(c, post=kw['post'], post_output='float', denoise=kw['denoise'], denoise_strength=0.25)
    torch.cuda.synchronize(); sess.check(); sess.close()
    kw['post'].close(); kw['denoise'].close()
    # live
    voc = live.LiveVocoder(model, 3, chunk, **handles())
    for b in range(3):
        voc.open(b, seed=70 + b, gain=live.peak_gain(hp, live.chunked_peak([sigs[b]], k), 'cuda') if hp.rescale else 1.0)
    got, frames, pos = {b: [] for b in range(3)}, {b: [] for b in range(3)}, [0] * 3
    while any(voc._open):
        blk = np.zeros((3, chunk), np.float32)
        n, fin = [0] * 3, [False] * 3
        for b in range(3):
            if voc._open[b]:
                n[b] = min(chunk, lens[b] - pos[b])
                blk[b, :n[b]] = sigs[b][pos[b]:pos[b] + n[b]]
                pos[b] += n[b]; fin[b] = pos[b] == lens[b]
        for b, ch in voc.push(blk, n, fin).items():
            got[b].append(ch.result); frames[b].append(ch.frames)
    torch.cuda.synchronize(); voc.check(); voc.close()
    for b in range(3):
        assert np.array_equal(_bits(torch.cat(frames[b], 1).cpu().numpy().T), _bits(mels[b])), b            # the frames are analyse_wavs'
        smp = torch.cat([r[0] for r in got[b]])
        assert smp.shape[0] == LIVE_FRAMES[b] * hop and torch.equal(smp, want[b][0]), b                        # the generated samples
        y = torch.cat([r[1] for r in got[b]])
        assert y.shape == want[b][1].shape and torch.equal(y.view(torch.int32), want[b][1].view(torch.int32)), b      # the playable chunks
        assert float(y.abs().max()) > 0
    model.engine.close()


def test_wavs_dir_through_the_live_route_writes_the_same_mels(tmp_path):
    """synthesize.py --wavs_dir (its driver, run_wav_synthesis) with mi355_synthesis_live_chunk_ms = 50: the wavs are written, mel-*.npy are byte-identical to
    the whole-recording route's"""
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesize import run_wav_synthesis
    base = TINY + ',wavenet_synthesis_batch_size=4'
    hp0 = H._build(); hp0.parse(base)
    lens = [700, 1102 * 2, 1500]
    paths, _ = _recordings(str(tmp_path / 'wavs'), hp0, lens)
    model = WaveNet(hp0)
    model.build(3, 16 * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()

    class Args:
        wavs_dir = str(tmp_path / 'wavs')
    outs = {}
    for tag, extra in (('whole', ''), ('live', ',mi355_synthesis_live_chunk_ms=50')):
        hp = H._build(); hp.parse(base + extra)
        out = str(tmp_path / tag)
        run_wav_synthesis(Args, ckpt, out, hp)
        outs[tag] = os.path.join(out, 'wavs')
    for i, n in enumerate(lens):
        a, b = (open(os.path.join(outs[t], 'mel-rec%d.npy' % i), 'rb').read() for t in ('whole', 'live'))
        assert a == b and len(a) > 128, i
        rate, pcm = wavfile.read(os.path.join(outs['live'], 'wavenet-audio-rec%d.wav' % i))
        assert rate == hp0.sample_rate and pcm.dtype == np.int16 and pcm.shape == ((1 + n // 16) * 16,), (i, pcm.shape)
    rows = open(os.path.join(outs['live'], 'map.txt')).read().strip().split('\n')
    assert len(rows) == 3 and all(len(r.split('|')) == 3 for r in rows)
