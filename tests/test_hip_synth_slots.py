"""Synthesis slots (wn_synth_slots_*): utterances join and leave a running batch.  A slot's out_samples / out_raw are compared with torch.equal
against ONE Engine.synthesize of the same B and steps_per_graph with the utterance's frames in batch row = slot index (device noise: column b of
the reference's noise = fill_noise(B = 1, seed_b)) -- whatever the cutting into pushes, the time the slot was opened, its neighbours or its
previous occupant."""
import random

import numpy as np
import pytest
import torch

from hip_util import SMALL, make_hp, oracle_cfg, synth_batch, upload_params
from oracle import mulaw as M
from oracle import wavenet_oracle as O
from test_hip_synth import _noise, _setup
from test_hip_synth_pipe import PAPER_FULL
from test_hip_synth_stream import WN_E_SHAPE, WN_E_STATE, _alloc

pytestmark = pytest.mark.gpu

WN_E_UNSUPPORTED = -4


class Utt(object):
    """One utterance of a test session: c [cin, Tc] mel frames, the slot it goes to, the push index from which it may be opened."""

    def __init__(self, name, slot, c, open_at=0, seed=0, g=None, ti=None, noise=None, abandon_after=None):
        self.name, self.slot, self.c, self.open_at, self.seed = name, slot, c.contiguous(), open_at, seed
        self.g, self.ti, self.noise, self.abandon_after = g, ti, noise, abandon_after
        self.Tc = int(c.shape[-1])


def _mels(cfg, Tc, seed):
    return synth_batch(cfg, 1, Tc * cfg.hop, seed=seed)[1][0]


def _neutral_noise(cfg, n, B, nps):
    if cfg.input_type != 'mulaw-quantize' and cfg.out_channels == 2:
        return torch.zeros(n, B, nps)
    return torch.full((n, B, nps), 0.5)


def _set_g(eng, cfg, B, rows):
    """global condition of a reference batch: rows {slot: g}; the other rows get a neutral one"""
    if cfg.gin_channels <= 0:
        return
    if cfg.use_speaker_embedding:
        g = torch.zeros(B, dtype=torch.int32)
        for s, v in rows.items():
            g[s] = int(v)
    else:
        g = torch.zeros(B, cfg.gin_channels)
        for s, v in rows.items():
            g[s] = v
    eng.set_global_condition(g.cuda())


def _reference(eng, cfg, B, utts, spg=0, exact_len=False, device_noise=True):
    """{name: (samples [T_u], raw [O, T_u], features [cin, T_u])} from one-shot runs: utterances in distinct slots share a call (zero frames behind
    a shorter one: only with a zero lookahead, where the frames after an utterance's end do not reach its conditioning); exact_len: one call per
    distinct length.  Returns the configuration of the runs too."""
    hop, nps, C = eng.hop, eng.noise_per_step, cfg.cin_channels
    todo, res, conf = [u for u in utts], {}, None
    scalar = cfg.input_type != 'mulaw-quantize'
    while todo:
        grp, rest = [], []
        for u in todo:
            if all(u.slot != v.slot for v in grp) and (not exact_len or not grp or grp[0].Tc == u.Tc):
                grp.append(u)
            else:
                rest.append(u)
        todo = rest
        Tc = max(u.Tc for u in grp)
        T = Tc * hop
        c = torch.zeros(B, C, Tc)
        nz = _neutral_noise(cfg, T, B, nps)
        ti = None
        if any(u.ti is not None for u in grp):
            ti = torch.zeros(B, T, dtype=torch.float32 if scalar else torch.int32)
        for u in grp:
            c[u.slot, :, :u.Tc] = u.c
            n = u.Tc * hop
            if u.noise is not None:
                nz[:n, u.slot] = u.noise
            elif device_noise:
                one = torch.empty(n, 1, nps, device='cuda')
                eng.fill_noise(one, 1, n, u.seed)
                nz[:n, u.slot] = one[:, 0].cpu()
            if u.ti is not None:
                ti[u.slot, :n] = u.ti
        _set_g(eng, cfg, B, {u.slot: u.g for u in grp})
        out, raw = _alloc(eng, cfg, B, T)
        eng.synthesize(c.cuda(), nz.cuda(), out, raw, None if ti is None else ti.cuda(), steps_per_graph=spg)
        feats = torch.empty(B, C, T, device='cuda')
        eng.upsampled_features(feats)
        torch.cuda.synchronize(); eng.synth_check()
        conf = eng.synth_config()
        for u in grp:
            n = u.Tc * hop
            res[u.name] = (out[u.slot, :n].cpu(), raw[u.slot, :, :n].cpu(), feats[u.slot, :, :n].cpu())
    return res, conf


def _session(eng, cfg, B, utts, spg=0, seed=0, tick=None, between=None, sizes=(0, 1, 1, 2, 3, 5, 8, 13), check_feats=False):
    """Run the utterances through one slot session: every push gives each live slot a random number of frames (or `tick`), opens what is due and
    whose slot is free, abandons what asks for it.  Returns {name: (samples, raw, features of the last push)}, the configuration, the pushes."""
    from wavenet_vocoder.models.wavenet import stream_schedule
    hop, nps, C, O_ = eng.hop, eng.noise_per_step, cfg.cin_channels, cfg.out_channels
    right = eng.stream_lookahead()[1]
    scalar = cfg.input_type != 'mulaw-quantize'
    rnd = random.Random(seed)
    eng.slots_begin(B, steps_per_graph=spg)
    pending = sorted(utts, key=lambda u: u.open_at)
    live, keep, k = {}, [], 0
    acc = {u.name: [[], [], None] for u in utts}
    for s in range(B):
        assert eng.slot_frames_done(s) == -1
    while pending or live:
        for s in [s for s, st in live.items() if st['u'].abandon_after is not None and st['sent'] >= st['u'].abandon_after]:
            eng.slot_abandon(s)
            assert eng.slot_frames_done(s) == -1
            del live[s]
        for u in list(pending):
            if u.open_at > k or u.slot in live:
                continue
            gd = None
            if cfg.gin_channels > 0:
                gd = (torch.tensor([int(u.g)], dtype=torch.int32) if cfg.use_speaker_embedding else u.g.float()).cuda()
            eng.slot_open(u.slot, seed=u.seed, g=gd)
            live[u.slot] = dict(u=u, sent=0, done=0)
            pending.remove(u)
        frames, final, n = [0] * B, [False] * B, [0] * B
        for s, st in live.items():
            u = st['u']
            rem = u.Tc - st['sent']
            frames[s] = min(rem, tick if tick else rnd.choice(sizes))
            final[s] = frames[s] == rem
            first, end = stream_schedule(st['done'], st['sent'] + frames[s], right, final[s])
            n[s] = (end - first) * hop
        Tn, n_max = max(frames), max(n)
        cc = None
        if Tn > 0:
            cc = torch.zeros(B, C, Tn)
            for s, st in live.items():
                cc[s, :, :frames[s]] = st['u'].c[:, st['sent']:st['sent'] + frames[s]]
            cc = cc.cuda()
        pitch = n_max + 3                                   # (a pitch wider than the longest span: the tail keeps the caller's bytes)
        out, raw = _alloc(eng, cfg, B, pitch)
        nz = ti = None
        if any(st['u'].noise is not None for st in live.values()):
            nz = _neutral_noise(cfg, max(n_max, 1), B, nps)
            for s, st in live.items():
                t0 = st['done'] * hop
                nz[:n[s], s] = st['u'].noise[t0:t0 + n[s]]
            nz = nz.cuda()
        if any(st['u'].ti is not None for st in live.values()):
            ti = torch.zeros(B, pitch, dtype=torch.float32 if scalar else torch.int32)
            for s, st in live.items():
                t0 = st['done'] * hop
                if st['u'].ti is not None:
                    ti[s, :n[s]] = st['u'].ti[t0:t0 + n[s]]
            ti = ti.cuda()
        got = eng.slots_push(cc, frames, final, out, raw, nz, ti)
        assert got == n, (k, got, n)
        fe = None
        if check_feats and n_max > 0:
            fe = torch.empty(B, C, n_max, device='cuda')
            eng.upsampled_features(fe)
        keep.append((out, raw, list(n)))
        for s in list(live):
            st = live[s]
            name = st['u'].name
            acc[name][0].append(out[s, :n[s]]); acc[name][1].append(raw[s, :, :n[s]])
            if fe is not None and n[s] > 0:
                acc[name][2] = fe[s, :, :n[s]]
            st['sent'] += frames[s]; st['done'] += n[s] // hop
            if final[s]:
                assert st['done'] == st['u'].Tc
                del live[s]
                assert eng.slot_frames_done(s) == -1
            else:
                assert eng.slot_frames_done(s) == st['done']
        if between is not None:
            between(k)
        k += 1
    torch.cuda.synchronize(); eng.synth_check()
    conf = eng.synth_config()
    for out, raw, n in keep:                                # nothing beyond n_out[b] was written (idle slots: nothing at all)
        for s in range(B):
            assert bool((out[s, n[s]:] == -7).all()) and bool(torch.isnan(raw[s, :, n[s]:]).all()), 'slot %d wrote past its %d samples' % (s, n[s])
    eng.slots_end()
    res = {}
    for u in utts:
        a = acc[u.name]
        res[u.name] = (torch.cat(a[0]).cpu() if a[0] else None, torch.cat(a[1], 1).cpu() if a[1] else None, None if a[2] is None else a[2].cpu())
    return res, conf, k


def _same(got, ref, names, feats=False):
    for name in names:
        g, r = got[name], ref[name]
        assert g[0].shape == r[0].shape, (name, g[0].shape, r[0].shape)
        assert torch.equal(g[0], r[0]), '%s: out_samples differ at %d of %d positions (first %d)' % (
            name, int((g[0] != r[0]).sum()), g[0].numel(), int((g[0] != r[0]).nonzero()[0]))
        assert torch.equal(g[1], r[1]), '%s: out_raw differs at %d positions (max %.3e)' % (name, int((g[1] != r[1]).sum()), float((g[1] - r[1]).abs().max()))
        if feats:
            n = g[2].shape[-1]
            assert torch.equal(g[2], r[2][:, r[2].shape[-1] - n:]), '%s: upsampled features of the last push differ' % name


# --------------------------------------------------------------------------------------------------------------------------------
def _rows_independent(eng, cfg, B, Tc, seed):
    T = Tc * cfg.hop
    _, c = synth_batch(cfg, B, T, seed=seed)
    nz, _ = _noise(cfg, T, B, seed=seed + 1)
    _, c2 = synth_batch(cfg, B, T, seed=seed + 7)
    nz2, _ = _noise(cfg, T, B, seed=seed + 8)
    out, raw = _alloc(eng, cfg, B, T)
    eng.synthesize(c.cuda(), nz.cuda(), out, raw)
    torch.cuda.synchronize(); eng.synth_check()
    out, raw = out.cpu(), raw.cpu()
    for b in (0, B // 2, B - 1):
        cm, nm = c2.clone(), nz2.clone()
        cm[b] = c[b]; nm[:, b] = nz[:, b]
        o2, r2 = _alloc(eng, cfg, B, T)
        eng.synthesize(cm.cuda(), nm.cuda(), o2, r2)
        torch.cuda.synchronize(); eng.synth_check()
        assert torch.equal(o2[b].cpu(), out[b]) and torch.equal(r2[b].cpu(), raw[b]), 'row %d of %d depends on the other rows' % (b, B)
    return eng.synth_config()


def test_reference_rows_are_independent():
    """The reference of every equality below is sound: row b of a one-shot run does not change, bit for bit, when the other rows' mels and noise
    columns are replaced (paper model B = 8; hparams.py's model B = 20 on three instances).  Passes without the slot sessions too."""
    hp, cfg, eng, params, wav, c, T = _setup(8, 6, **PAPER_FULL)
    conf = _rows_independent(eng, cfg, 8, 6, seed=20)
    assert conf['path'] == 'pipeline'
    eng.close()
    from wavenet_vocoder import _ext
    hp = make_hp(); cfg = oracle_cfg(hp)
    eng = _ext.Engine(hp, 20, 5 * cfg.hop)
    eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=11, bias_scale=0.05)))
    conf = _rows_independent(eng, cfg, 20, 5, seed=30)
    assert conf['path'] == 'pipeline' and conf['instances'] == 3
    eng.close()


def _paper_utts(cfg, reuse):
    L = dict(a=80, b=37, c=64, d=11, e=52)
    u = [Utt('a', 0, _mels(cfg, L['a'], 1), 0, seed=101), Utt('b', 5, _mels(cfg, L['b'], 2), 0, seed=102), Utt('c', 2, _mels(cfg, L['c'], 3), 3, seed=103),
         Utt('d', 7, _mels(cfg, L['d'], 4), 7, seed=104), Utt('e', 1, _mels(cfg, L['e'], 5), 7, seed=105)]
    if reuse:
        # slot 5 again after its 37-frame utterance, while slots 0 and 2 are mid-utterance; slot 3: an utterance abandoned after >= 9 frames, then a new one
        u += [Utt('f', 5, _mels(cfg, 29, 6), 1, seed=106), Utt('x', 3, _mels(cfg, 30, 7), 1, seed=107, abandon_after=9), Utt('y', 3, _mels(cfg, 15, 8), 2, seed=108)]
    return u


@pytest.mark.parametrize('reuse', [False, True])
def test_slots_staggered_joins_paper_pipeline(reuse):
    """Paper model on the pipeline, B = 8: utterances of 80, 37, 64, 11, 52 frames (22 000 steps for the longest: every d = 2048 queue wraps) opened at
    pushes 0, 0, 3, 7, 7 into slots 0, 5, 2, 7, 1; irregular pushes (0 and 1 frames, different counts per slot); device noise, then explicit noise.
    reuse: slot 5 is reopened after its utterance next to mid-utterance neighbours, and a slot abandoned mid-utterance is reopened: nothing of the
    old queue rows, carry or noise counter leaks.  Slots 4 and 6 (and 3 without reuse) are never opened."""
    B = 8
    hp, cfg, eng, params, wav, c, T = _setup(B, 80, **PAPER_FULL)
    assert eng.stream_lookahead() == (0, 0)
    utts = _paper_utts(cfg, reuse)
    names = [u.name for u in utts if u.abandon_after is None]
    ref, rconf = _reference(eng, cfg, B, [u for u in utts if u.abandon_after is None])
    got, conf, pushes = _session(eng, cfg, B, utts, seed=5 + reuse)
    assert rconf['path'] == 'pipeline' and conf == rconf
    _same(got, ref, names)
    if not reuse:
        for u in utts:
            u.noise = _noise(cfg, u.Tc * cfg.hop, 1, seed=40 + u.slot)[0][:, 0]
        ref, _ = _reference(eng, cfg, B, utts)
        got, conf, pushes = _session(eng, cfg, B, utts, seed=9)
        _same(got, ref, names)
    print('\npaper model, %d slots, %d utterances in %d pushes: every slot == its one-shot reference (%s)' % (B, len(utts), pushes, conf))
    eng.close()


def test_slots_neighbours_undisturbed():
    """The same utterance in slot 0 gives equal bits whether the other seven slots are idle, live, or opening / finishing on every push."""
    B = 8
    hp, cfg, eng, params, wav, c, T = _setup(B, 16, **PAPER_FULL)
    main = Utt('m', 0, _mels(cfg, 14, 1), 0, seed=77)
    ref, _ = _reference(eng, cfg, B, [main])
    alone, _, _ = _session(eng, cfg, B, [main], seed=1, tick=2)
    live = [Utt('n%d' % s, s, _mels(cfg, 14, 10 + s), 0, seed=200 + s) for s in range(1, B)]
    busy, _, _ = _session(eng, cfg, B, [main] + live, seed=1, tick=2)
    churn = [Utt('k%d_%d' % (s, i), s, _mels(cfg, 1 + (s + i) % 2, 30 + 8 * i + s), i, seed=300 + 8 * i + s) for s in range(1, B) for i in range(0, 7, 1 + s % 2)]
    moving, _, _ = _session(eng, cfg, B, [main] + churn, seed=1, tick=2)
    for got in (alone, busy, moving):
        _same(got, ref, ['m'])
    eng.close()


def test_slots_default_model_subpixel_three_instances():
    """hparams.py's own model ('SubPixel' [11, 25], two frames of lookahead on both sides) with 20 slots on three pipeline instances: 26 utterances
    of 3 ... 14 frames, so slots open and finish next to mid-utterance neighbours and the upsample windows differ per slot in one push; samples, raw
    outputs and the upsampled features of each slot's last push vs the one-shot run of exactly that utterance's frames."""
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import slot_plan
    hp = make_hp(); cfg = oracle_cfg(hp)
    assert cfg.upsample_type == 'SubPixel'
    B = 20
    eng = _ext.Engine(hp, B, 16 * cfg.hop)
    eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=11, bias_scale=0.05)))
    assert eng.stream_lookahead() == (2, 2)
    rnd = random.Random(3)
    lengths = [3, 14] + [rnd.randint(3, 14) for _ in range(24)]
    utts, k = [], 0
    for opens, frames, final in slot_plan(lengths, B, 3):          # the plan decides which slot an utterance takes and from which push on
        utts += [Utt('u%d' % u, b, _mels(cfg, lengths[u], 50 + u), k, seed=500 + u) for b, u in opens]
        k += 1
    assert len(utts) == 26
    ref, rconf = _reference(eng, cfg, B, utts, exact_len=True)
    assert rconf['path'] == 'pipeline' and rconf['instances'] == 3
    got, conf, pushes = _session(eng, cfg, B, utts, seed=2, sizes=(0, 1, 2, 3, 4), check_feats=True)
    assert conf == rconf
    _same(got, ref, [u.name for u in utts], feats=True)
    eng.close()


def test_slots_launch_per_layer_mulaw_speaker_teacher_forced():
    """The launch-per-layer hipGraph path (steps_per_graph = 8): mu-law-quantize head, a different speaker id per slot given at slot_open, teacher
    forcing in one slot next to a free-running one (one test_inputs buffer serves a push: the free-running slot's row carries its own one-shot
    samples, which is free running), 'Resize' lookahead, push lengths that are not multiples of 8 steps."""
    B = 3
    hp, cfg, eng, params, wav, c, T = _setup(B, 19, input_type='mulaw-quantize', out_channels=256, quantize_channels=256, gin_channels=16,
                                             use_speaker_embedding=True, n_speakers=4, upsample_type='Resize', upsample_scales=[3, 5], hop_size=15)
    assert eng.stream_lookahead() == (1, 1)
    ids = torch.from_numpy(M.mulaw_quantize(wav.numpy())).int()
    tf = Utt('tf', 2, _mels(cfg, 19, 1), 0, seed=5, g=3, ti=ids[0].flip(0).contiguous())
    fr = Utt('fr', 0, _mels(cfg, 13, 2), 2, seed=6, g=1)
    late = Utt('late', 2, _mels(cfg, 7, 3), 3, seed=7, g=0)            # reuses the teacher-forced slot, free running
    free_ref, rconf = _reference(eng, cfg, B, [fr, late], spg=8, exact_len=True)
    assert rconf['path'] == 'graph'
    fr.ti, late.ti = free_ref['fr'][0], free_ref['late'][0]
    ref, _ = _reference(eng, cfg, B, [tf, fr, late], spg=8, exact_len=True)
    assert torch.equal(ref['fr'][0], free_ref['fr'][0]) and torch.equal(ref['late'][1], free_ref['late'][1])
    got, conf, _ = _session(eng, cfg, B, [tf, fr, late], spg=8, seed=4, sizes=(0, 1, 2, 3, 5), check_feats=True)
    assert conf['path'] == 'graph'
    _same(got, ref, ['tf', 'fr', 'late'], feats=True)
    fr.ti = late.ti = None                                           # ... and a session without test_inputs: the fed-back ids cross the push edges
    got, _, _ = _session(eng, cfg, B, [fr, late], spg=8, seed=8, sizes=(1, 2, 4))
    _same(got, free_ref, ['fr', 'late'])
    eng.close()


def test_slots_global_condition_per_slot_pipeline():
    """gin_channels = 8, float conditions, pipeline: two utterances with different g in neighbouring slots, one opened later."""
    B = 4
    hp, cfg, eng, params, wav, c, T = _setup(B, 24, gin_channels=8, use_speaker_embedding=False)
    gg = torch.Generator().manual_seed(2)
    u = [Utt('p', 1, _mels(cfg, 24, 1), 0, seed=11, g=torch.randn(8, generator=gg)), Utt('q', 2, _mels(cfg, 17, 2), 4, seed=12, g=torch.randn(8, generator=gg))]
    ref, rconf = _reference(eng, cfg, B, u)
    assert rconf['path'] == 'pipeline'
    got, conf, _ = _session(eng, cfg, B, u, seed=3)
    assert conf == rconf
    _same(got, ref, ['p', 'q'])
    eng.close()


def test_slots_isolated_from_training_steps():
    """wn_train_fwd + wn_train_bwd between pushes rewrite the context's conditioning, bias table and activations; the session keeps its own."""
    B = 4
    hp, cfg, eng, params, wav, c, T = _setup(B, 24, gin_channels=8, use_speaker_embedding=False)
    gg = torch.Generator().manual_seed(5)
    u = [Utt('p', 0, _mels(cfg, 24, 1), 0, seed=21, g=torch.randn(8, generator=gg)), Utt('q', 3, _mels(cfg, 12, 2), 2, seed=22, g=torch.randn(8, generator=gg))]
    ref, _ = _reference(eng, cfg, B, u)
    wav2, c2 = synth_batch(cfg, B, T, seed=8)
    x = wav2.view(B, 1, T).contiguous().cuda(); y = wav2.view(B, T, 1).contiguous().cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda'); loss = torch.zeros(1, device='cuda')
    grads = torch.empty(eng.n_params, device='cuda')
    eng.set_global_condition(torch.randn(B, 8, generator=gg).cuda())          # (the training step's own condition; a session does not use it)

    def train(i):
        eng.train_fwd(x, c2.cuda(), y, ln, 77 + i, loss)
        eng.train_bwd(grads)

    got, _, _ = _session(eng, cfg, B, u, seed=6, between=train)
    _same(got, ref, ['p', 'q'])
    assert torch.isfinite(loss).all()
    eng.close()


def test_slots_inference_only_never_allocates():
    """A session of 2 slots on an inference-only context of max_time = 16 frames runs utterances of 128, 40 and 90 frames in 8-frame pushes; the
    references come from a second, large context; wn_workspace_bytes does not change and neither (printed) does the free device memory."""
    from wavenet_vocoder import _ext
    B = 2
    hp = make_hp(**dict(SMALL, **PAPER_FULL))
    cfg = oracle_cfg(hp)
    params = O.init_params(cfg, seed=11, bias_scale=0.05)
    utts = [Utt('a', 0, _mels(cfg, 128, 1), 0, seed=31), Utt('b', 1, _mels(cfg, 40, 2), 0, seed=32), Utt('c', 1, _mels(cfg, 90, 3), 0, seed=33)]
    big = _ext.Engine(hp, B, 128 * cfg.hop, inference_only=True)
    big.pack_weights(upload_params(big, params))
    ref, rconf = _reference(big, cfg, B, utts)
    big.close()
    small = _ext.Engine(hp, B, 16 * cfg.hop, inference_only=True)
    small.pack_weights(upload_params(small, params))
    ws = small.lib.wn_workspace_bytes(small.h)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    got, conf, pushes = _session(small, cfg, B, utts, seed=1, tick=8)
    assert small.lib.wn_workspace_bytes(small.h) == ws
    assert conf == rconf
    _same(got, ref, ['a', 'b', 'c'])
    print('\n3 utterances (%d samples) through 2 slots of a context of max_time %d in %d pushes; free device memory %d -> %d (torch buffers of the test included)'
          % (sum(u.Tc for u in utts) * cfg.hop, 16 * cfg.hop, pushes, free0, torch.cuda.mem_get_info()[0]))
    small.close()


def test_slots_state_errors(monkeypatch):
    from wavenet_vocoder import _ext
    B, Tc = 2, 8
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc)
    cd = c.cuda()
    out, raw = _alloc(eng, cfg, B, T)

    def code(fn):
        with pytest.raises(_ext.WnError) as ei:
            fn()
        return ei.value.code

    push = lambda fr=(2, 0), fin=(False, False), k=2: eng.slots_push(cd[:, :, :k].contiguous(), list(fr), list(fin), out, raw)
    assert code(push) == WN_E_STATE                                           # no session
    assert code(lambda: eng.slot_open(0)) == WN_E_STATE
    eng.slots_begin(B)
    assert code(push) == WN_E_STATE                                           # frames for an idle slot
    eng.slot_open(0, seed=1)
    assert code(lambda: eng.slot_open(0, seed=2)) == WN_E_STATE               # open of a live slot
    assert push() == [2 * cfg.hop, 0]
    assert code(lambda: push((2, 1))) == WN_E_STATE                           # slot 1 is idle
    assert eng.slot_frames_done(0) == 2                                       # (a rejected push leaves every slot as it was)
    big = torch.cat([cd, cd], 2).contiguous()                                 # 16 frames > max_time / hop = 8 in one push
    assert code(lambda: eng.slots_push(big, [16, 0], [False, False], out, raw)) == WN_E_SHAPE
    assert eng.slot_frames_done(0) == 2
    assert push((6, 0), (True, False), 6) == [6 * cfg.hop, 0]
    assert eng.slot_frames_done(0) == -1
    for ender in (lambda: eng.synthesize(cd, None, out, raw, seed=1), lambda: eng.pack_weights(upload_params(eng, params)), lambda: eng.pipeline_dtype(True),
                  lambda: eng.stream_begin(B, seed=1)):
        eng.slots_begin(B)
        eng.slot_open(0, seed=1)
        push()
        ender()
        assert code(push) == WN_E_STATE
        assert code(lambda: eng.slot_open(1)) == WN_E_STATE
    eng.stream_begin(B, seed=1)                                               # ... and beginning a session ends a stream
    eng.slots_begin(B)
    assert code(lambda: eng.stream_push(cd[:, :, :2].contiguous(), out, raw)) == WN_E_STATE
    # poisoned by a flagged pipeline run (the hook sets the flag as a timed-out hand-off would; no fault is involved)
    eng.slot_open(0, seed=3)
    monkeypatch.setenv('WN_PIPE_TEST_ABORT', '1')
    push()
    monkeypatch.delenv('WN_PIPE_TEST_ABORT')
    torch.cuda.synchronize()
    assert code(eng.synth_check) == -3
    assert code(push) == WN_E_STATE
    assert code(lambda: eng.slot_open(1)) == WN_E_STATE
    eng.slots_begin(B)                                                        # a new session is clean
    eng.slot_open(1, seed=3)
    assert push((0, 8), (False, True), 8) == [0, T]
    torch.cuda.synchronize(); eng.synth_check()
    eng.close()
    hp32, cfg32, eng32, *_ = _setup(B, Tc, mi355_compute_dtype='fp32')
    assert code(lambda: eng32.slots_begin(B)) == WN_E_UNSUPPORTED
    eng32.close()


def test_facade_slots_equal_engine_level():
    """WaveNet.slots(): open / push per slot give the samples of the engine-level session (and so of the one-shot references)."""
    from wavenet_vocoder.models.wavenet import WaveNet
    B = 3
    hp, cfg, eng, params, wav, c, T = _setup(B, 20)
    utts = [Utt('a', 0, _mels(cfg, 20, 1), 0, seed=41), Utt('b', 2, _mels(cfg, 9, 2), 0, seed=42)]
    ref, _ = _reference(eng, cfg, B, utts)
    flat = upload_params(eng, params)
    eng.close()
    model = WaveNet(hp)
    model.build(B, T, params=flat.cpu())
    sess = model.slots(B)
    sess.open(0, seed=41)
    got = {'a': [], 'b': []}
    a, b = utts
    r = sess.push({0: a.c[:, :3].cuda()}); got['a'].append(r[0])
    sess.open(2, seed=42)
    r = sess.push({0: a.c[:, 3:4].cuda(), 2: (b.c[:, :9].cuda(), True)}, return_raw=True); got['a'].append(r[0][0]); got['b'].append(r[2][0])
    assert torch.equal(r[2][1].cpu(), ref['b'][1])
    r = sess.push({0: (a.c[:, 4:].cuda(), True)}); got['a'].append(r[0])
    torch.cuda.synchronize(); sess.check(); sess.close()
    for k in got:
        assert torch.equal(torch.cat(got[k]).cpu(), ref[k][0]), k


def test_synthesize_driver_slots(tmp_path):
    """wavenet_synthesize with mi355_synthesis_slots=4 on the 3-mel set of the chunked driver test: the same file names, each wav of its utterance's
    length, byte-identical between a tick of 3 and a tick of 8 frames (the cutting does not matter)."""
    import os
    import types
    import hparams as H
    from scipy.io import wavfile
    from test_hip_drivers import _dataset
    from wavenet_vocoder.train import wavenet_train
    from wavenet_vocoder.synthesize import wavenet_synthesize
    root = str(tmp_path)
    meta = _dataset(root)
    hp = H._build()
    hp.parse('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,'
             'hop_size=16,upsample_scales=[4,4],max_time_steps=512,wavenet_batch_size=4,wavenet_test_batches=1,wavenet_synthesis_batch_size=4,'
             'wavenet_learning_rate=1e-3,wavenet_dropout=0.0')
    log_dir = os.path.join(root, 'logs-WaveNet'); os.makedirs(log_dir, exist_ok=True)
    args = types.SimpleNamespace(base_dir=root, model='WaveNet', restore=False, wavenet_train_steps=2, checkpoint_interval=2,
                                 summary_interval=100, eval_interval=100, embedding_interval=100, eval_max_time=0)
    save_dir = wavenet_train(args, log_dir, hp, meta)
    mels_dir = os.path.join(root, 'mels_in'); os.makedirs(mels_dir)
    for i in range(3):
        np.save(os.path.join(mels_dir, 'mel-%d.npy' % i), np.load(os.path.join(root, 'mels', 'mel-%03d.npy' % i))[:10 + i])
    cwd = os.getcwd(); os.chdir(root)
    try:
        for slots, chunk, od in ((0, 0, 'one/'), (4, 3, 'slots3/'), (4, 8, 'slots8/')):
            hp.set_hparam('mi355_synthesis_slots', slots)
            hp.set_hparam('mi355_synthesis_chunk_frames', chunk)
            wavenet_synthesize(types.SimpleNamespace(model='WaveNet', mels_dir=mels_dir, output_dir=od, speaker_id=None), hp, save_dir)
    finally:
        os.chdir(cwd)
    ls = {od: sorted(os.listdir(os.path.join(root, 'wavenet_' + od, 'wavs'))) for od in ('one', 'slots3', 'slots8')}
    wavs = [f for f in ls['one'] if f.endswith('.wav')]
    assert ls['one'] == ls['slots3'] == ls['slots8'] and len(wavs) == 3
    for f in wavs:
        a = open(os.path.join(root, 'wavenet_slots3', 'wavs', f), 'rb').read()
        assert a == open(os.path.join(root, 'wavenet_slots8', 'wavs', f), 'rb').read(), f
        i = int(f.replace('.wav', '').split('-')[-1])
        sr, data = wavfile.read(os.path.join(root, 'wavenet_slots3', 'wavs', f))
        assert len(data) == (10 + i) * 16, (f, len(data))
