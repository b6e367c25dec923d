"""Folded synthesis on the device (wn_synthesize_folded): the rows of a folded run are one-shot rows, the unfold is the numpy mirror of
tests/fold_util.py, the conditioning is the whole utterance's, and the call leaves the context as wn_synthesize does.  Comparisons are torch.equal /
np.array_equal unless a test says otherwise."""
import ctypes

import numpy as np
import pytest
import torch

import fold_util as FU
from hip_util import SMALL, make_hp, oracle_cfg, synth_batch, upload_params
from oracle import wavenet_oracle as O
from test_hip_synth import _noise, _setup
from test_hip_synth_pipe import PAPER_FULL
from test_hip_synth_stream import WN_E_SHAPE, WN_E_STATE, _alloc

pytestmark = pytest.mark.gpu

WN_E_UNSUPPORTED = -4
HEADS = {'mol-raw': dict(), 'gauss-mulaw': dict(out_channels=2, input_type='mulaw'),
         'softmax-mulaw-quantize': dict(input_type='mulaw-quantize', quantize_channels=256, out_channels=256)}
FRAMES = (37, 9)                                 # test 1: U = 2, rows_max 5, warm 1, fade 1 (min_keep 4: the 37-frame utterance takes four rows)


def _mels(cfg, frames, seed=1):
    return [synth_batch(cfg, 1, F * cfg.hop, seed=seed + u)[1][0].contiguous() for u, F in enumerate(frames)]


def _engine(n_rows, max_frames, **kw):
    hp, cfg, eng, params, _, _, _ = _setup(n_rows, max_frames, **kw)
    return hp, cfg, eng, params


def _fold(eng, cfg, cs, plan, noise=None, seed=0, ti=None, g=None, spg=0, kind='equal_power', pad=4):
    """one folded run with sentinels everywhere: (wav [U, pitch], rows, raw, features, configuration), all on the host"""
    hop, C = cfg.hop, cfg.cin_channels
    frames = [int(c.shape[-1]) for c in cs]
    U, F_max, n_max = len(cs), max(frames), max(r[2] for r in plan) * hop
    cc = torch.zeros(U, C, F_max)
    for u, c in enumerate(cs):
        cc[u, :, :frames[u]] = c
    wav = torch.full((U, F_max * hop + pad), float('nan'), device='cuda')
    rows, raw = _alloc(eng, cfg, len(plan), n_max + pad)
    tid = None
    if ti is not None:
        tid = torch.zeros(U, F_max * hop + pad, dtype=rows.dtype)
        for u, t in enumerate(ti):
            tid[u, :frames[u] * hop] = t
        tid = tid.cuda()
    eng.synthesize_folded(cc.cuda(), frames, plan, wav, fade_kind=kind, g=g, noise=None if noise is None else noise.cuda(), seed=seed, test_inputs=tid,
                          out_rows=rows, out_raw=raw, steps_per_graph=spg)
    feats = torch.empty(len(plan), C, n_max, device='cuda')
    eng.upsampled_features(feats)
    torch.cuda.synchronize(); eng.synth_check()
    return wav.cpu(), rows.cpu(), raw.cpu(), feats.cpu(), eng.synth_config()


def _rows_oneshot(eng, cfg, cs, plan, noise, spg=0, g_rows=None):
    """ONE wn_synthesize(B = n_rows): row r holds the frames of plan row r, zero frames behind"""
    hop = cfg.hop
    Tc = max(r[2] for r in plan)
    c = torch.zeros(len(plan), cfg.cin_channels, Tc)
    for i, (u, first, n, _, _) in enumerate(plan):
        c[i, :, :n] = cs[u][:, first:first + n]
    if g_rows is not None:
        eng.set_global_condition(g_rows.cuda())
    out, raw = _alloc(eng, cfg, len(plan), Tc * hop)
    eng.synthesize(c.cuda(), noise.cuda(), out, raw, None, steps_per_graph=spg)
    torch.cuda.synchronize(); eng.synth_check()
    return out.cpu(), raw.cpu(), eng.synth_config()


def _rows_equal(plan, hop, rows, raw, ref_out, ref_raw):
    for i, (_, _, n, _, _) in enumerate(plan):
        n *= hop
        assert torch.equal(rows[i, :n], ref_out[i, :n]), 'row %d: samples differ at %d of %d positions' % (i, int((rows[i, :n] != ref_out[i, :n]).sum()), n)
        assert torch.equal(raw[i, :, :n], ref_raw[i, :, :n]), 'row %d: raw outputs differ (max %.3e)' % (i, float((raw[i, :, :n] - ref_raw[i, :, :n]).abs().max()))
        assert bool((rows[i, n:] == -7).all()) and bool(torch.isnan(raw[i, :, n:]).all()), 'row %d wrote past its %d samples' % (i, n)


def _device_noise_columns(eng, cfg, plan, seed):
    hop, nps = cfg.hop, eng.noise_per_step
    n_max = max(r[2] for r in plan) * hop
    nz = torch.zeros(n_max, len(plan), nps) if cfg.input_type != 'mulaw-quantize' and cfg.out_channels == 2 else torch.full((n_max, len(plan), nps), 0.5)
    for i, r in enumerate(plan):
        one = torch.empty(r[2] * hop, 1, nps, device='cuda')
        eng.fill_noise(one, 1, r[2] * hop, seed + i)
        nz[:r[2] * hop, i] = one[:, 0].cpu()
    return nz


def _eq(a, b):
    """torch.equal that lets the NaN sentinels of untouched elements compare equal"""
    return torch.equal(torch.nan_to_num(a, nan=-9.0), torch.nan_to_num(b, nan=-9.0))


def _decode(cfg, t):
    from wavenet_vocoder import _ext
    if cfg.input_type == 'mulaw-quantize':
        return _ext.inv_mulaw_quantize(t.cuda().contiguous()).cpu().numpy()
    if cfg.input_type == 'mulaw':
        return _ext.inv_mulaw(t.cuda().contiguous()).cpu().numpy()
    return t.numpy().copy()


# ---- 1
@pytest.mark.parametrize('spg', [0, 4])
@pytest.mark.parametrize('head', sorted(HEADS))
def test_rows_are_oneshot_rows(head, spg):
    """SMALL ('2D' upsampling: zero lookahead), two utterances of 37 and 9 frames in 4 + 1 rows: samples and raw outputs of every row == row r of ONE
    wn_synthesize(B = 5) holding that row's frames; explicit noise, then device noise (column r = fill_noise(B = 1, seed + r))."""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    assert [r[0] for r in plan] == [0, 0, 0, 0, 1] and max(r[4] for r in plan) == 1
    hp, cfg, eng, params = _engine(len(plan), max(r[2] for r in plan) + 1, **HEADS[head])
    assert eng.stream_lookahead() == (0, 0)
    cs = _mels(cfg, FRAMES)
    n_max = max(r[2] for r in plan) * cfg.hop
    nz = _noise(cfg, n_max, len(plan), seed=4)[0]
    ref_out, ref_raw, rconf = _rows_oneshot(eng, cfg, cs, plan, nz, spg)
    wav, rows, raw, _, conf = _fold(eng, cfg, cs, plan, noise=nz, spg=spg)
    assert conf == rconf and conf['path'] == ('graph' if spg else 'pipeline')
    _rows_equal(plan, cfg.hop, rows, raw, ref_out, ref_raw)
    nzd = _device_noise_columns(eng, cfg, plan, seed=900)
    ref_out, ref_raw, _ = _rows_oneshot(eng, cfg, cs, plan, nzd, spg)
    wav, rows, raw, _, _ = _fold(eng, cfg, cs, plan, noise=None, seed=900, spg=spg)
    _rows_equal(plan, cfg.hop, rows, raw, ref_out, ref_raw)
    eng.close()


# ---- 2
@pytest.mark.parametrize('kind', ['equal_power', 'linear'])
@pytest.mark.parametrize('head', sorted(HEADS))
def test_unfold_arithmetic(head, kind):
    """out_wav == the numpy float32 mirror (tests/fold_util.py) fed Engine.inv_mulaw* of the run's own rows, both fade kinds, the three input types; pitches
    that allow the 16-byte accesses (equal_power: + 4) and pitches that do not (linear: + 3); elements beyond an utterance's length keep the caller's bytes."""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    hp, cfg, eng, params = _engine(len(plan), max(r[2] for r in plan) + 1, **HEADS[head])
    cs = _mels(cfg, FRAMES)
    n_max = max(r[2] for r in plan) * cfg.hop
    nz = _noise(cfg, n_max, len(plan), seed=4)[0]
    pad = 4 if kind == 'equal_power' else 3
    wav, rows, raw, _, _ = _fold(eng, cfg, cs, plan, noise=nz, kind=kind, pad=pad)
    want = FU.unfold(list(FRAMES), plan, cfg.hop, _decode(cfg, rows), kind)
    fades = 0
    for u, F in enumerate(FRAMES):
        n = F * cfg.hop
        got = wav[u, :n].numpy()
        assert np.array_equal(got.view(np.uint32), want[u].view(np.uint32)), 'utterance %d: %d of %d samples differ (max %.3e)' % (
            u, int((got != want[u]).sum()), n, float(np.abs(got - want[u]).max()))
        assert bool(torch.isnan(wav[u, n:]).all()), 'utterance %d: written past its %d samples' % (u, n)
        assert np.abs(got).max() <= 1.5 and np.isfinite(got).all()
        fades += sum(r[4] for r in plan if r[0] == u)
    assert fades == 3
    eng.close()


# ---- 3
@pytest.mark.parametrize('utype,scales,look', [('SubPixel', [4, 4], (2, 2)), ('Resize', [3, 5], (1, 1))])
def test_conditioning_is_the_whole_utterances(utype, scales, look):
    """Upsample kernels with every tap alive (NN_init off) and a lookahead: the features a folded run used == the gathered columns of the features of
    the one-shot run of each WHOLE utterance; upsampling a row's own frames gives other features (so the test tells the two apart).  Utterances of
    37, 9 and 37 frames: the two equal ones are upsampled as one batch."""
    from wavenet_vocoder import _ext
    frames = (37, 9, 37)
    hop = scales[0] * scales[1]
    plan = _ext.fold_plan(list(frames), 7, 1, 1, 4)
    hp, cfg, eng, params = _engine(len(plan), 40, upsample_type=utype, upsample_scales=scales, hop_size=hop, NN_init=False)
    assert eng.stream_lookahead() == look
    cs = _mels(cfg, frames)
    n_max = max(r[2] for r in plan) * hop
    nz = _noise(cfg, n_max, len(plan), seed=4)[0]
    whole = []
    for u, F in enumerate(frames):
        out, raw = _alloc(eng, cfg, 1, F * hop)
        eng.synthesize(cs[u][None].contiguous().cuda(), None, out, raw, seed=1)
        fe = torch.empty(1, cfg.cin_channels, F * hop, device='cuda')
        eng.upsampled_features(fe)
        torch.cuda.synchronize(); eng.synth_check()
        whole.append(fe[0].cpu())
    _, _, _, feats, _ = _fold(eng, cfg, cs, plan, noise=nz)
    for i, (u, first, n, _, _) in enumerate(plan):
        assert torch.equal(feats[i, :, :n * hop], whole[u][:, first * hop:(first + n) * hop]), 'row %d reads other conditioning than the one-shot run' % i
    # a row cut out of the middle, upsampled alone, differs at its edges
    u, first, n, _, _ = plan[1]
    out, raw = _alloc(eng, cfg, 1, n * hop)
    eng.synthesize(cs[u][None, :, first:first + n].contiguous().cuda(), nz[:n * hop, :1].contiguous().cuda(), out, raw)
    fe = torch.empty(1, cfg.cin_channels, n * hop, device='cuda')
    eng.upsampled_features(fe)
    torch.cuda.synchronize()
    assert not torch.equal(fe[0].cpu(), whole[u][:, first * hop:(first + n) * hop])
    eng.close()


# ---- 4
@pytest.mark.parametrize('spg', [0, 4])
def test_teacher_forcing_past_the_receptive_field_is_the_oneshot_run(spg):
    """SMALL with 'SubPixel', teacher forced, warm 1: for every row r > 0 the raw outputs at row-local times >= 13 == those of a teacher-forced one-shot run
    of B = n_rows whose every row is the whole utterance, at the matching absolute times; both paths.
    The bound is the receptive field, 13 samples: the output at time t reads the INPUTS of the steps t - 12 ... t, and the input of a step is the previous
    sample -- the row's step 0 reads silence (the cold start) where the one-shot run reads the teacher's sample, so step 12 still differs (asserted: the
    bound is tight) and step 13 is the first whose 13 inputs are all teacher samples.  (One step later than "12 past samples" suggests: a row's warm-up of
    16 samples still covers it.)"""
    from wavenet_vocoder import _ext
    F = 37
    plan = _ext.fold_plan([F], 4, 1, 1, 4)
    assert len(plan) == 4
    hp, cfg, eng, params = _engine(len(plan), F, upsample_type='SubPixel', NN_init=False)
    assert eng.receptive_field == 13
    hop, T = cfg.hop, F * cfg.hop
    wav, c = synth_batch(cfg, 1, T, seed=3)
    n_max = max(r[2] for r in plan) * hop
    nz = _noise(cfg, T, len(plan), seed=4)[0]
    out, raw = _alloc(eng, cfg, len(plan), T)
    eng.synthesize(c.repeat(len(plan), 1, 1).contiguous().cuda(), nz.cuda(), out, raw, wav.repeat(len(plan), 1).contiguous().cuda(), steps_per_graph=spg)
    torch.cuda.synchronize(); eng.synth_check()
    ref_raw, rconf = raw.cpu(), eng.synth_config()
    _, rows, fraw, _, conf = _fold(eng, cfg, [c[0]], plan, noise=nz[:n_max].contiguous(), ti=[wav[0]], spg=spg)
    assert conf == rconf and conf['path'] == ('graph' if spg else 'pipeline')
    rf = eng.receptive_field
    assert rf <= plan[1][3] * hop - plan[1][1] * hop                       # the warm-up covers it: nothing that differs is kept
    for i, (_, first, n, _, _) in enumerate(plan):
        t0 = 0 if i == 0 else rf
        got, want = fraw[i, :, t0:n * hop], ref_raw[i, :, first * hop + t0:(first + n) * hop]
        assert torch.equal(got, want), 'row %d: %d raw outputs differ past the receptive field (max %.3e)' % (i, int((got != want).sum()), float((got - want).abs().max()))
        if i > 0:
            assert not torch.equal(fraw[i, :, rf - 1], ref_raw[i, :, first * hop + rf - 1])              # (the cold start does show up to the step before)
    eng.close()


# ---- 5
@pytest.mark.parametrize('head', sorted(HEADS))
def test_one_row_per_utterance_is_wn_synthesize(head):
    """min_keep larger than half of every utterance: the plan is one row per utterance and out_wav == the decoded samples of the one-shot run"""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 12, 4, 2, 40)
    assert plan == [(0, 0, 37, 0, 0), (1, 0, 9, 0, 0)]
    hp, cfg, eng, params = _engine(2, 37, **HEADS[head])
    cs = _mels(cfg, FRAMES)
    nz = _noise(cfg, 37 * cfg.hop, 2, seed=4)[0]
    ref_out, _, _ = _rows_oneshot(eng, cfg, cs, plan, nz)
    wav, rows, _, _, _ = _fold(eng, cfg, cs, plan, noise=nz)
    dec = _decode(cfg, ref_out)
    for u, F in enumerate(FRAMES):
        n = F * cfg.hop
        assert np.array_equal(wav[u, :n].numpy().view(np.uint32), dec[u, :n].view(np.uint32)), u
    eng.close()


# ---- 6
def _check_against_oneshot(eng, cfg, cs, plan, seed):
    n_max = max(r[2] for r in plan) * cfg.hop
    nz = _noise(cfg, n_max, len(plan), seed=seed)[0]
    ref_out, ref_raw, rconf = _rows_oneshot(eng, cfg, cs, plan, nz)
    wav, rows, raw, _, conf = _fold(eng, cfg, cs, plan, noise=nz)
    assert conf == rconf and conf['path'] == 'pipeline'
    _rows_equal(plan, cfg.hop, rows, raw, ref_out, ref_raw)
    assert torch.isfinite(wav[0, :cs[0].shape[-1] * cfg.hop]).all()
    return conf


def test_specialised_pipeline_paper_model():
    """PAPER_FULL (R = S = 256: the width-specialised kernel with the batched pre-multiplication), 1 utterance x 24 frames in 3 rows, warm 2, fade 1"""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan([24], 3, 2, 1, 4)
    assert len(plan) == 3
    hp, cfg, eng, params = _engine(3, max(r[2] for r in plan) + 1, **PAPER_FULL)
    conf = _check_against_oneshot(eng, cfg, _mels(cfg, [24]), plan, seed=6)
    assert conf['kernel_spec'] == 1
    eng.close()


def test_specialised_pipeline_default_model_several_instances():
    """hparams.py's own model ('SubPixel' [11, 25], R = S = 128), 1 utterance x 48 frames in 12 rows (min_keep 4): more than one pipeline instance.  The
    upsample kernels are the NN-initialised ones, whose side taps are zero: a row's own frames upsample to the whole utterance's rows bit for bit, so the
    one-shot run of the row's frames is an exact reference here (test_conditioning_is_the_whole_utterances covers kernels whose side taps are alive)."""
    from wavenet_vocoder import _ext
    hp = make_hp(); cfg = oracle_cfg(hp)
    assert cfg.upsample_type == 'SubPixel' and hp.NN_init
    plan = _ext.fold_plan([48], 12, 4, 2, 4)
    assert len(plan) == 12
    eng = _ext.Engine(hp, 12, (max(r[2] for r in plan) + 1) * cfg.hop)
    eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=11, bias_scale=0.05)))
    conf = _check_against_oneshot(eng, cfg, _mels(cfg, [48]), plan, seed=7)
    assert conf['instances'] > 1 and conf['kernel_spec'] == 2
    eng.close()


# ---- 7
def test_global_conditioning_per_utterance():
    """speaker ids: two utterances with different speakers; every row == the one-shot row under its utterance's speaker"""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    hp, cfg, eng, params = _engine(len(plan), max(r[2] for r in plan) + 1, gin_channels=16, use_speaker_embedding=True, n_speakers=4)
    cs = _mels(cfg, FRAMES)
    n_max = max(r[2] for r in plan) * cfg.hop
    nz = _noise(cfg, n_max, len(plan), seed=4)[0]
    spk = torch.tensor([3, 1], dtype=torch.int32)
    g_rows = torch.tensor([int(spk[r[0]]) for r in plan], dtype=torch.int32)
    ref_out, ref_raw, rconf = _rows_oneshot(eng, cfg, cs, plan, nz, g_rows=g_rows)
    swapped, _, _ = _rows_oneshot(eng, cfg, cs, plan, nz, g_rows=torch.tensor([int(spk[1 - r[0]]) for r in plan], dtype=torch.int32))
    assert not torch.equal(swapped, ref_out)                                   # (the speaker does change the samples)
    wav, rows, raw, _, conf = _fold(eng, cfg, cs, plan, noise=nz, g=spk.cuda())
    assert conf == rconf
    _rows_equal(plan, cfg.hop, rows, raw, ref_out, ref_raw)
    eng.close()


# ---- 8
def _code(fn):
    from wavenet_vocoder import _ext
    with pytest.raises(_ext.WnError) as ei:
        fn()
    return ei.value.code


def test_folded_run_ends_streams_and_sessions_and_ignores_training_steps():
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    B = len(plan)
    hp, cfg, eng, params = _engine(B, max(r[2] for r in plan) + 1)
    cs = _mels(cfg, FRAMES)
    T = 8 * cfg.hop
    _, c = synth_batch(cfg, B, T, seed=3)
    out, raw = _alloc(eng, cfg, B, T)
    first = _fold(eng, cfg, cs, plan, seed=5)
    eng.stream_begin(B, seed=1)
    eng.stream_push(c[:, :, :2].contiguous().cuda(), out, raw)
    assert _eq(_fold(eng, cfg, cs, plan, seed=5)[0], first[0])
    assert _code(lambda: eng.stream_push(c[:, :, 2:4].contiguous().cuda(), out, raw)) == WN_E_STATE
    eng.slots_begin(B)
    eng.slot_open(0, seed=1)
    eng.slots_push(c[:, :, :2].contiguous().cuda(), [2] + [0] * (B - 1), [False] * B, out, raw)
    again = _fold(eng, cfg, cs, plan, seed=5)
    assert _code(lambda: eng.slots_push(c[:, :, 2:4].contiguous().cuda(), [2] + [0] * (B - 1), [False] * B, out, raw)) == WN_E_STATE
    # a training step between two folded runs changes nothing
    wav2, c2 = synth_batch(cfg, B, T, seed=8)
    x = wav2.view(B, 1, T).contiguous().cuda(); y = wav2.view(B, T, 1).contiguous().cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda'); loss = torch.zeros(1, device='cuda')
    grads = torch.empty(eng.n_params, device='cuda')
    eng.train_fwd(x, c2.cuda(), y, ln, 77, loss)
    eng.train_bwd(grads)
    after = _fold(eng, cfg, cs, plan, seed=5)
    for a, b, c_ in zip(first[:3], again[:3], after[:3]):          # waveforms, rows, raw outputs (sentinels included)
        assert _eq(a, b) and _eq(a, c_)
    for i, r in enumerate(plan):                                   # features: the columns a row read (beyond them the table is stale, as after a slot push)
        n = r[2] * cfg.hop
        assert torch.equal(first[3][i, :, :n], again[3][i, :, :n]) and torch.equal(first[3][i, :, :n], after[3][i, :, :n])
    assert torch.isfinite(loss).all()
    eng.close()


def test_inference_only_context_never_allocates():
    """the library's allocation counter (wn_test_device_resources [4]) does not move over folded runs on an inference-only context, with and without the
    caller taking the rows (the row scratch is reserved with the slot tables), teacher forcing included"""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    hp = make_hp(**SMALL); cfg = oracle_cfg(hp)
    eng = _ext.Engine(hp, len(plan), (max(r[2] for r in plan) + 1) * cfg.hop, inference_only=True)
    eng.pack_weights(upload_params(eng, O.init_params(cfg, seed=11, bias_scale=0.05)))
    cs = _mels(cfg, FRAMES)
    res = (ctypes.c_int64 * 5)()
    assert eng.lib.wn_test_device_resources(res) == 0
    before = list(res)
    a = _fold(eng, cfg, cs, plan, seed=5)
    _fold(eng, cfg, cs, plan, seed=5, ti=[a[1][0].new_zeros(F * cfg.hop) for F in FRAMES])
    cc = torch.zeros(2, cfg.cin_channels, 37)
    for u, c in enumerate(cs):
        cc[u, :, :FRAMES[u]] = c
    wav = torch.full((2, 37 * cfg.hop), float('nan'), device='cuda')
    eng.synthesize_folded(cc.cuda(), list(FRAMES), plan, wav, seed=5)               # no out_rows / out_raw: the rows live in the context's scratch
    torch.cuda.synchronize(); eng.synth_check()
    assert eng.lib.wn_test_device_resources(res) == 0
    assert (res[0], res[4]) == (before[0], before[4]), 'a folded run allocated: live buffers / allocations ever %s -> %s' % (before, list(res))
    for u, F in enumerate(FRAMES):
        assert torch.equal(wav[u, :F * cfg.hop].cpu(), a[0][u, :F * cfg.hop])
    eng.close()


def test_shape_errors():
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    n_fr = max(r[2] for r in plan)
    hp = make_hp(**SMALL); cfg = oracle_cfg(hp)
    cs = _mels(cfg, FRAMES)
    params = O.init_params(cfg, seed=11, bias_scale=0.05)

    def engine(B, frames, **kw):
        e = _ext.Engine(make_hp(**dict(SMALL, **kw)), B, frames * cfg.hop)
        e.pack_weights(upload_params(e, params))
        return e

    eng = engine(len(plan) - 1, 40)
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=1)) == WN_E_SHAPE             # more rows than max_batch
    eng.close()
    eng = engine(len(plan), n_fr - 1)
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=1)) == WN_E_SHAPE             # the longest row exceeds max_time
    eng.close()
    eng = engine(len(plan), n_fr)
    _fold(eng, cfg, cs, plan, seed=1, pad=0)                                          # exactly max_time: fits
    ti = [torch.zeros(F * cfg.hop) for F in FRAMES]
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=1, ti=ti, pad=4)) == WN_E_SHAPE      # gathered test_inputs at a pitch of n_max + 4 exceed the row scratch
    _fold(eng, cfg, cs, plan, seed=1, ti=ti, pad=0)
    eng.close()
    eng = engine(len(plan), 40, mi355_compute_dtype='fp32')
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=1)) == WN_E_UNSUPPORTED
    eng.close()
    eng = _ext.Engine(hp, len(plan), 40 * cfg.hop)
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=1)) == WN_E_STATE             # before wn_pack_weights
    eng.pack_weights(upload_params(eng, params))
    bad = list(plan); bad[2] = (bad[2][0], bad[2][1], bad[2][2], bad[2][3] - 1, bad[2][4])
    with pytest.raises(_ext.WnError) as ei:
        _fold(eng, cfg, cs, bad, seed=1)
    assert ei.value.code == -1 and 'row 2' in str(ei.value)
    eng.close()


def test_failed_pipeline_run_is_reported_and_poisons_nothing(monkeypatch):
    """the flag a timed-out hand-off would raise (set by the library's test hook; no fault is involved) is reported by synth_check; a stream opened
    afterwards works"""
    from wavenet_vocoder import _ext
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    B = len(plan)
    hp, cfg, eng, params = _engine(B, max(r[2] for r in plan) + 1)
    cs = _mels(cfg, FRAMES)
    good = _fold(eng, cfg, cs, plan, seed=5)
    assert good[4]['path'] == 'pipeline'
    monkeypatch.setenv('WN_PIPE_TEST_ABORT', '1')
    assert _code(lambda: _fold(eng, cfg, cs, plan, seed=5)) == -3
    monkeypatch.delenv('WN_PIPE_TEST_ABORT')
    _, c = synth_batch(cfg, B, 4 * cfg.hop, seed=3)
    out, raw = _alloc(eng, cfg, B, 4 * cfg.hop)
    eng.stream_begin(B, seed=1)
    assert eng.stream_push(c.cuda(), out, raw, final=True) == 4 * cfg.hop
    torch.cuda.synchronize(); eng.synth_check()
    assert torch.equal(_fold(eng, cfg, cs, plan, seed=5)[1], good[1])
    eng.close()


# ---- façade
def test_facade_folded_equals_engine_level():
    """WaveNet.folded: the waveforms of the engine-level call with the plan, seed and noise the façade derives; one row per utterance: incremental()'s samples"""
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet, fold_capacity
    hp, cfg, eng, params = _engine(5, 16)
    flat = upload_params(eng, params).cpu()
    cs = _mels(cfg, FRAMES)
    plan = _ext.fold_plan(list(FRAMES), 5, 1, 1, 4)
    model = WaveNet(hp)
    model.build(*fold_capacity(list(FRAMES), plan, cfg.hop), params=flat)
    wavs, info = model.folded(cs, rows=5, warm=1, fade=1, min_keep=4, return_rows=True, check=True)
    assert info['plan'] == plan and [int(w.shape[0]) for w in wavs] == [F * cfg.hop for F in FRAMES]
    eng.pack_weights(flat.cuda())
    ref = _fold(eng, cfg, cs, plan, seed=info['seed'])
    for u, F in enumerate(FRAMES):
        assert torch.equal(wavs[u].cpu(), ref[0][u, :F * cfg.hop])
    for i, r in enumerate(plan):
        n = r[2] * cfg.hop
        assert torch.equal(info['rows'][i, :n].cpu(), ref[1][i, :n]) and torch.equal(info['raw'][i, :, :n].cpu(), ref[2][i, :, :n])
    eng.close()


# ---- 9
def test_synthesize_driver_folded(tmp_path):
    """wavenet_synthesize with mi355_synthesis_fold_rows=4 on the 3-mel set of the chunked driver test (10, 11 and 12 frames; min_frames 4, so the rows are
    1 + 1 + 2): the same file names as the one-call path, each wav of its utterance's length, and two fresh runs agree byte for byte."""
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
             'wavenet_learning_rate=1e-3,wavenet_dropout=0.0,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4')
    log_dir = os.path.join(root, 'logs-WaveNet'); os.makedirs(log_dir, exist_ok=True)
    args = types.SimpleNamespace(base_dir=root, model='WaveNet', restore=False, wavenet_train_steps=2, checkpoint_interval=2,
                                 summary_interval=100, eval_interval=100, embedding_interval=100, eval_max_time=0)
    save_dir = wavenet_train(args, log_dir, hp, meta)
    mels_dir = os.path.join(root, 'mels_in'); os.makedirs(mels_dir)
    for i in range(3):
        np.save(os.path.join(mels_dir, 'mel-%d.npy' % i), np.load(os.path.join(root, 'mels', 'mel-%03d.npy' % i))[:10 + i])
    cwd = os.getcwd(); os.chdir(root)
    try:
        for rows, od in ((0, 'one/'), (4, 'fold_a/'), (4, 'fold_b/')):
            hp.set_hparam('mi355_synthesis_fold_rows', rows)
            wavenet_synthesize(types.SimpleNamespace(model='WaveNet', mels_dir=mels_dir, output_dir=od, speaker_id=None), hp, save_dir)
    finally:
        os.chdir(cwd)
    ls = {od: sorted(os.listdir(os.path.join(root, 'wavenet_' + od, 'wavs'))) for od in ('one', 'fold_a', 'fold_b')}
    wavs = [f for f in ls['one'] if f.endswith('.wav')]
    assert ls['one'] == ls['fold_a'] == ls['fold_b'] and len(wavs) == 3
    for f in wavs:
        a = open(os.path.join(root, 'wavenet_fold_a', 'wavs', f), 'rb').read()
        assert a == open(os.path.join(root, 'wavenet_fold_b', 'wavs', f), 'rb').read(), f
        i = int(f.replace('.wav', '').split('-')[-1])
        sr, data = wavfile.read(os.path.join(root, 'wavenet_fold_a', 'wavs', f))
        assert len(data) == (10 + i) * 16, (f, len(data))
