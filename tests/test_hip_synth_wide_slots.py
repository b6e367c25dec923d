"""Wide slot sessions (wn_synth_wide_slots_begin): a slot session of any B <= max_batch on the wide owner of the launch-per-layer path.

The session table of csrc/wn_synth.hip has one block per tile of 32 slots and every tile advances its own push-local step, so a slot's samples and
raw outputs are torch.equal to
  * Engine.synthesize(steps_per_graph = 24) of <= 32 streams with the utterance in row slot & 31 (the reference of every test below), and
  * Engine.synthesize_wide with the utterance in row slot,
whatever B, the slot's tile, the cutting into pushes, the time the slot was opened, the other slots and tiles, or the slot's previous occupant.
Models: synth_ref.MODELS on hip_util.SMALL (hop 16, R = 64); utterances of 3 ... 20 frames (48 ... 320 samples: from 9 frames on an utterance passes
128 steps and the d = 32 ring of s6 wraps).  The drivers of a session and of the one-shot references are those of test_hip_synth_slots.py."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import synth_ref as SR
from hip_util import oracle_cfg, synth_batch, upload_params
from test_hip_synth import _noise
from test_hip_synth_slots import Utt, _mels, _reference, _same, _session
from test_hip_synth_stream import _alloc

pytestmark = pytest.mark.gpu

SPG = 24
MAXF = 20                                   # frames of the longest utterance = max_time of the engines
LENS = (3, 20, 7, 12, 5, 9)
WN_E_ARG, WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -1, -2, -4, -5


class Wide(object):
    """An engine whose slots_begin opens the WIDE session, so that test_hip_synth_slots._session drives it; pairs {slot: (tau_scale, tau_select)} are
    set right after the slot is opened."""

    def __init__(self, eng, pairs=None):
        self._e, self._pairs = eng, pairs or {}

    def __getattr__(self, k):
        return getattr(self._e, k)

    def slots_begin(self, B, steps_per_graph=0):
        self._e.wide_slots_begin(B, steps_per_graph=steps_per_graph)

    def slot_open(self, slot, seed=0, g=None):
        self._e.slot_open(slot, seed=seed, g=g)
        if slot in self._pairs:
            self._e.slot_temperature(slot, *self._pairs[slot])


def _model(model, B, extra=None, **kw):
    from wavenet_vocoder import _ext
    hp, cfg, params = SR.make_case(model, 1, 16, extra)[:3]
    eng = _ext.Engine(hp, B, MAXF * cfg.hop, **kw)
    eng.pack_weights(upload_params(eng, params))
    return hp, cfg, params, eng


def _g(cfg, i):
    if cfg.gin_channels <= 0:
        return None
    return i % cfg.n_speakers if cfg.use_speaker_embedding else torch.randn(cfg.gin_channels, generator=torch.Generator().manual_seed(900 + i))


def _utt(cfg, name, slot, frames, i, open_at=0, **kw):
    return Utt(name, slot, _mels(cfg, frames, 100 + i), open_at, seed=5000 + i, g=_g(cfg, i), **kw)


def _one_per_slot(cfg, slots):
    return [_utt(cfg, 'u%d' % s, s, LENS[(5 * s + s // 32) % len(LENS)], s) for s in slots]


def _tile_reference(eng, cfg, utts):
    """{name: (samples, raw, features)} of the runs of <= 32 streams: the utterances of tile k in the rows slot & 31 of synthesize(steps_per_graph = 24)
    (one call per distinct length when the upsampling looks ahead: test_hip_synth_slots._reference)."""
    res = {}
    for k in sorted({u.slot >> 5 for u in utts}):
        rows = [Utt(u.name, u.slot & 31, u.c, u.open_at, u.seed, u.g, u.ti, u.noise) for u in utts if u.slot >> 5 == k]
        r, conf = _reference(eng, cfg, 32, rows, spg=SPG, exact_len=eng.stream_lookahead() != (0, 0))
        assert conf['path'] == 'graph'
        res.update(r)
    return res


def _wide_session(eng, cfg, B, utts, pairs=None, **kw):
    got, conf, pushes = _session(Wide(eng, pairs), cfg, B, utts, spg=SPG, **kw)
    assert conf['path'] == 'graph'
    return got, pushes


# ---- 1. slot == one-shot ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model,B', [('s6', 33), ('s6', 64), ('s6', 70), ('s6_gauss', 70), ('s6_softmax', 70), ('s6_gin', 70), ('s6_gin_raw_1d', 70)])
def test_every_slot_equals_the_run_of_its_tile(model, B):
    """Every slot open with its own length; pushes of (0, 1, 1, 2, 3, 5, 8, 13) frames.  33: one stream in the second tile; 64: two full tiles; 70: six
    streams in the third.  70 slots on s6: also ONE synthesize_wide of the 70 utterances padded to the longest."""
    hp, cfg, params, eng = _model(model, B)
    utts = _one_per_slot(cfg, range(B))
    ref = _tile_reference(eng, cfg, utts)
    got, pushes = _wide_session(eng, cfg, B, utts, seed=B)
    _same(got, ref, [u.name for u in utts])
    if (model, B) == ('s6', 70):
        T, nps = MAXF * cfg.hop, eng.noise_per_step
        c = torch.zeros(B, cfg.cin_channels, MAXF)
        nz = torch.full((T, B, nps), 0.5)
        for u in utts:
            n = u.Tc * cfg.hop
            c[u.slot, :, :u.Tc] = u.c
            nz[:n, u.slot] = eng.fill_noise(torch.empty(n, 1, nps, device='cuda'), 1, n, u.seed)[:, 0].cpu()
        out, raw = _alloc(eng, cfg, B, T)
        eng.synthesize_wide(c.cuda(), nz.cuda(), out, raw, None, steps_per_graph=SPG)
        torch.cuda.synchronize(); eng.synth_check()
        for u in utts:
            n = u.Tc * cfg.hop
            assert torch.equal(out[u.slot, :n].cpu(), got[u.name][0]) and torch.equal(raw[u.slot, :, :n].cpu(), got[u.name][1]), 'slot %d differs from row %d of the wide run' % (u.slot, u.slot)
    print('\n%s: %d slots in %d pushes, every slot == row slot & 31 of the run of its tile' % (model, B, pushes))
    eng.close()


# ---- 2. joins, leaves, reuse across tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('teacher', [False, True])
def test_hundred_utterances_through_forty_slots(teacher):
    from wavenet_vocoder.models.wavenet import slot_plan
    B = 40
    hp, cfg, params, eng = _model('s6', B)
    rnd = random.Random(7)
    lengths = [3, 20] + [rnd.randint(3, 20) for _ in range(98)]
    utts, k, per_slot = [], 0, [0] * B
    for opens, frames, final in slot_plan(lengths, B, 3):
        for b, u in opens:
            ti = synth_batch(cfg, 1, lengths[u] * cfg.hop, seed=700 + u)[0][0] if teacher else None
            utts.append(_utt(cfg, 'u%d' % u, b, lengths[u], u, open_at=k, ti=ti))
            per_slot[b] += 1
        k += 1
    assert len(utts) == 100 and min(per_slot[:32]) >= 2 and min(per_slot[32:]) >= 2      # slots of both tiles are reopened
    ref = _tile_reference(eng, cfg, utts)
    got, pushes = _wide_session(eng, cfg, B, utts, seed=11, sizes=(0, 1, 2, 3, 4))
    _same(got, ref, [u.name for u in utts])
    eng.close()


# ---- 3. tile edges and idle tiles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['edges', 'idle_middle_tile', 'tile_finishes_first'])
def test_tile_edges_idle_tiles_and_finished_tiles(case):
    """edges: only the lanes 31 | 32, 63 | 64 and 69 ever carry utterances (the rest of all three tiles are dummies), two of them twice.
    idle_middle_tile: tiles 0 and 2 run, tile 1 never has a live slot.  tile_finishes_first: every utterance in ONE push -- tile 0's counts (48 steps) are
    used up while tile 1 still generates (320 steps) -- and then pushes in which tile 0 has nothing at all.  _session checks that rows and elements beyond
    n_out[b] keep the caller's bytes."""
    B = 70
    hp, cfg, params, eng = _model('s6', B)
    kw = dict(seed=3)
    if case == 'edges':
        utts = [_utt(cfg, 'a', 31, 20, 1), _utt(cfg, 'b', 32, 9, 2), _utt(cfg, 'c', 63, 3, 3, open_at=1), _utt(cfg, 'd', 64, 12, 4), _utt(cfg, 'e', 69, 20, 5, open_at=2),
                _utt(cfg, 'f', 63, 10, 6, open_at=3), _utt(cfg, 'g', 32, 5, 7, open_at=2)]
    elif case == 'idle_middle_tile':
        utts = [_utt(cfg, 'a', 3, 20, 1), _utt(cfg, 'b', 31, 7, 2), _utt(cfg, 'c', 64, 13, 3), _utt(cfg, 'd', 69, 20, 4, open_at=1), _utt(cfg, 'e', 0, 9, 5, open_at=4)]
    else:
        utts = [_utt(cfg, 'a', 0, 3, 1), _utt(cfg, 'b', 31, 3, 2), _utt(cfg, 'c', 40, 20, 3), _utt(cfg, 'd', 33, 20, 4, open_at=1), _utt(cfg, 'e', 69, 4, 5)]
        kw = dict(tick=100)
    ref = _tile_reference(eng, cfg, utts)
    got, pushes = _wide_session(eng, cfg, B, utts, **kw)
    _same(got, ref, [u.name for u in utts])
    if case == 'tile_finishes_first':       # ... and with 16 frames a push: 'd' runs on over two pushes in which tile 0 has finished
        got, pushes = _wide_session(eng, cfg, B, utts, tick=16)
        _same(got, ref, [u.name for u in utts])
    eng.close()


# ---- 4. cut invariance ----------------------------------------------------------------------------------------------------------------------
def test_the_cutting_into_pushes_does_not_matter():
    B = 70
    hp, cfg, params, eng = _model('s6', B)
    utts = _one_per_slot(cfg, range(B))
    names = [u.name for u in utts]
    one, _ = _wide_session(eng, cfg, B, utts, tick=1)
    cyc, _ = _wide_session(eng, cfg, B, utts, seed=5)
    all_, pushes = _wide_session(eng, cfg, B, utts, tick=100)
    assert pushes == 1
    _same(cyc, one, names)
    _same(all_, one, names)
    eng.close()


# ---- 5. noise and temperature ---------------------------------------------------------------------------------------------------------------
PAIRS = ((1.0, 1.0), (0.7, 0.85), (0.0, 0.0))


@pytest.mark.parametrize('model', ['s6', 's6_gauss'])
def test_device_noise_and_pairs_per_slot(model):
    """Device noise of slot b = fill_noise(B = 1, T, seed_b), tempered by ITS pair: the reference reads temper_noise of that column at (1, 1)."""
    B = 40
    hp, cfg, params, eng = _model(model, B)
    nps = eng.noise_per_step
    slots = [0, 5, 30, 31, 32, 33, 38, 39]
    utts = _one_per_slot(cfg, slots)
    pairs = {s: PAIRS[i % 3] for i, s in enumerate(slots)}
    plain = _tile_reference(eng, cfg, utts)                       # (device noise, untempered)
    got, _ = _wide_session(eng, cfg, B, utts, seed=1)
    _same(got, plain, [u.name for u in utts])
    for u in utts:
        n = u.Tc * cfg.hop
        col = eng.fill_noise(torch.empty(n, 1, nps, device='cuda'), 1, n, u.seed)
        u.noise = eng.temper_noise(col, *pairs[u.slot])[:, 0].cpu()
    ref = _tile_reference(eng, cfg, utts)
    for u in utts:
        u.noise = None
    got, _ = _wide_session(eng, cfg, B, utts, pairs=pairs, seed=2)
    _same(got, ref, [u.name for u in utts])
    assert not torch.equal(ref['u5'][0], plain['u5'][0])
    eng.close()


def test_caller_noise_is_tempered_column_by_column():
    B = 40
    hp, cfg, params, eng = _model('s6', B)
    nps, hop = eng.noise_per_step, cfg.hop
    slots = [1, 31, 32, 39]
    utts = [_utt(cfg, 'u%d' % s, s, 9, s) for s in slots]
    pairs = {s: PAIRS[(i + 1) % 3] for i, s in enumerate(slots)}
    T = 9 * hop
    nz = _noise(cfg, T, B, seed=6)[0].cuda()
    for u in utts:
        u.noise = eng.temper_noise(nz[:, u.slot:u.slot + 1].contiguous(), *pairs[u.slot])[:, 0].cpu()
    ref = _tile_reference(eng, cfg, utts)
    eng.wide_slots_begin(B, steps_per_graph=SPG)
    cc = torch.zeros(B, cfg.cin_channels, 9)
    for u in utts:
        eng.slot_open(u.slot, seed=u.seed)
        eng.slot_temperature(u.slot, *pairs[u.slot])
        cc[u.slot] = u.c
    keep = nz.clone()
    out, raw = _alloc(eng, cfg, B, T)
    n = eng.slots_push(cc.cuda(), [9 if s in slots else 0 for s in range(B)], [s in slots for s in range(B)], out, raw, nz)
    torch.cuda.synchronize(); eng.synth_check()
    assert n == [T if s in slots else 0 for s in range(B)]
    assert torch.equal(nz, keep), 'the caller\'s noise buffer was written'
    for u in utts:
        assert torch.equal(out[u.slot].cpu(), ref[u.name][0]) and torch.equal(raw[u.slot].cpu(), ref[u.name][1]), u.name
    eng.close()


# ---- 6. isolation ---------------------------------------------------------------------------------------------------------------------------
def test_training_steps_between_pushes_and_the_features_of_a_push():
    B = 40
    hp, cfg, params, eng = _model('s6', B)
    utts = [_utt(cfg, 'a', 0, 20, 1), _utt(cfg, 'b', 31, 12, 2), _utt(cfg, 'c', 32, 20, 3, open_at=1), _utt(cfg, 'd', 39, 7, 4), _utt(cfg, 'e', 31, 6, 5, open_at=2)]
    ref = _tile_reference(eng, cfg, utts)
    Bt, T = 2, MAXF * cfg.hop
    wav2, c2 = synth_batch(cfg, Bt, T, seed=8)
    x = wav2.view(Bt, 1, T).contiguous().cuda(); y = wav2.view(Bt, T, 1).contiguous().cuda(); c2 = c2.cuda()
    ln = torch.full((Bt,), T, dtype=torch.int32, device='cuda'); loss = torch.zeros(1, device='cuda')
    grads = torch.empty(eng.n_params, device='cuda')

    def train(i):
        eng.train_fwd(x, c2, y, ln, 77 + i, loss)
        eng.train_bwd(grads)

    got, _ = _wide_session(eng, cfg, B, utts, seed=6, between=train, check_feats=True)
    _same(got, ref, [u.name for u in utts], feats=True)
    assert torch.isfinite(loss).all()
    eng.close()


# ---- 7. an inference-only context -----------------------------------------------------------------------------------------------------------
def test_inference_only_context_of_70_slots_never_allocates():
    """References from a training context, closed before the inference-only one of max_batch = 70 is created.  The test's own tensors come out of torch's
    cache (warmed before wn_create), so the free device memory after the last push is the one after wn_create."""
    B = 70
    hp, cfg, params, big = _model('s6', B)
    utts = _one_per_slot(cfg, range(B))
    ref = _tile_reference(big, cfg, utts)
    big.close()
    warm = [torch.empty(256 << 20, dtype=torch.uint8, device='cuda')] + [torch.empty(512 << 10, dtype=torch.uint8, device='cuda') for _ in range(64)]
    del warm
    hp, cfg, params, eng = _model('s6', B, inference_only=True)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    res0, res1 = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    assert eng.lib.wn_test_device_resources(res0) == 0
    got, pushes = _wide_session(eng, cfg, B, utts, seed=4)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert eng.lib.wn_test_device_resources(res1) == 0
    print('\n70 slots on an inference-only context, %d pushes: free device memory %d -> %d; buffers %d -> %d, allocations ever %d -> %d' % (
        pushes, free0, free1, res0[0], res1[0], res0[4], res1[4]))
    _same(got, ref, [u.name for u in utts])
    assert res0[0] == res1[0] and res0[4] == res1[4], 'a wide slot session on an inference-only context allocated a device buffer'
    assert free1 == free0
    eng.close()


# ---- 8. state and errors --------------------------------------------------------------------------------------------------------------------
def test_state_and_errors():
    from wavenet_vocoder import _ext
    B = 40
    hp, cfg, params, eng = _model('s6', B)
    hop, C = cfg.hop, cfg.cin_channels
    T = MAXF * hop
    out, raw = _alloc(eng, cfg, B, T)
    cd = torch.zeros(B, C, MAXF + 4, device='cuda')

    def code(fn):
        with pytest.raises(_ext.WnError) as ei:
            fn()
        return ei.value.code

    def push(frames, final=(), k=2):
        fr = [frames.get(s, 0) for s in range(B)]
        return eng.slots_push(cd[:, :, :k].contiguous(), fr, [s in final for s in range(B)], out, raw)

    assert code(lambda: eng.wide_slots_begin(0)) == WN_E_SHAPE
    assert code(lambda: eng.wide_slots_begin(B + 1)) == WN_E_SHAPE
    with pytest.raises(_ext.WnError, match=r'slot count 33 outside \(0, min\(32, max_batch = 40\)\]') as ei:      # the narrow session keeps its limit and its text
        eng.slots_begin(33)
    assert ei.value.code == WN_E_SHAPE
    eng.wide_slots_begin(B, steps_per_graph=SPG)
    assert code(lambda: push({35: 2})) == WN_E_STATE                            # frames for an idle slot
    assert code(lambda: eng.slot_open(B, seed=1)) == WN_E_ARG                   # slot index >= B
    eng.slot_open(35, seed=1); eng.slot_open(2, seed=2)
    assert code(lambda: eng.slot_open(35, seed=3)) == WN_E_STATE                # open of a live slot
    got = push({35: 2, 2: 1})
    assert got[35] == 2 * hop and got[2] == hop and sum(got) == 3 * hop
    assert eng.synth_path == 'graph'
    assert code(lambda: push({35: 1, 7: 1})) == WN_E_STATE                      # slot 7 is idle: the push is rejected as a whole
    assert (eng.slot_frames_done(35), eng.slot_frames_done(2), eng.slot_frames_done(7)) == (2, 1, -1)
    assert code(lambda: push({35: MAXF + 4, 2: 1}, k=MAXF + 4)) == WN_E_SHAPE   # slot 35's window of 24 frames exceeds what the workspace holds (max_time = 20 frames)
    assert (eng.slot_frames_done(35), eng.slot_frames_done(2)) == (2, 1)       # ... and every slot is as it was
    assert code(lambda: eng.slot_temperature(B, 1.0, 1.0)) == WN_E_ARG and code(lambda: eng.slot_abandon(B)) == WN_E_ARG
    assert push({35: 2}, final=(35,))[35] == 2 * hop
    assert eng.slot_frames_done(35) == -1
    co, cr = _alloc(eng, cfg, 2, 2 * hop)
    enders = (lambda: eng.synthesize_wide(cd[:, :, :2].contiguous(), None, out[:, :2 * hop].contiguous(), None, None, steps_per_graph=SPG),
              lambda: eng.stream_begin(2, seed=1, steps_per_graph=SPG), lambda: eng.slots_begin(2, steps_per_graph=SPG),
              lambda: eng.synthesize(cd[:2, :, :2].contiguous(), None, co, cr, seed=1, steps_per_graph=SPG), lambda: eng.pack_weights(upload_params(eng, params)))
    for ender in enders:
        eng.wide_slots_begin(B, steps_per_graph=SPG)
        eng.slot_open(35, seed=1)
        push({35: 1})
        ender()
        if ender is enders[2]:                                                  # (a narrow session is open now: 40 entries do not fit it, nor is slot 35 its)
            assert code(lambda: eng.slot_open(35, seed=1)) == WN_E_ARG
            eng.slots_end()
        assert code(lambda: push({35: 1})) == WN_E_STATE
        assert code(lambda: eng.slot_open(36, seed=1)) == WN_E_STATE
    torch.cuda.synchronize(); eng.synth_check()
    eng.close()
    from wavenet_vocoder import _ext as E
    hp0 = SR.make_case('s6', 1, 16)[0]
    raw_eng = E.Engine(hp0, B, T)
    assert code(lambda: raw_eng.wide_slots_begin(B)) == WN_E_STATE              # before wn_pack_weights
    raw_eng.close()
    hp32, cfg32, p32, eng32 = _model('s6', B, extra=dict(mi355_compute_dtype='fp32'))
    assert code(lambda: eng32.wide_slots_begin(B)) == WN_E_UNSUPPORTED
    eng32.close()


# ---- 9. facade and driver -------------------------------------------------------------------------------------------------------------------
def test_facade_wide_slots_equal_engine_level():
    from wavenet_vocoder.models.wavenet import WaveNet
    B = 40
    hp, cfg, params, eng = _model('s6', B)
    utts = [_utt(cfg, 'a', 0, 20, 1), _utt(cfg, 'b', 33, 9, 2), _utt(cfg, 'c', 39, 5, 3)]
    ref = _tile_reference(eng, cfg, utts)
    got_eng, _ = _wide_session(eng, cfg, B, utts, seed=2)
    flat = upload_params(eng, params)
    eng.close()
    model = WaveNet(hp)
    model.build(B, MAXF * cfg.hop, params=flat.cpu())
    sess = model.wide_slots(B, steps_per_graph=SPG)
    assert sess.wide
    a, b, c = utts
    got = {'a': [], 'b': [], 'c': []}
    sess.open(0, seed=a.seed); sess.open(39, seed=c.seed)
    r = sess.push({0: a.c[:, :3].cuda(), 39: (c.c.cuda(), True)}); got['a'].append(r[0]); got['c'].append(r[39])
    sess.open(33, seed=b.seed)
    r = sess.push({0: a.c[:, 3:4].cuda(), 33: (b.c.cuda(), True)}, return_raw=True); got['a'].append(r[0][0]); got['b'].append(r[33][0])
    assert torch.equal(r[33][1].cpu(), ref['b'][1])
    r = sess.push({0: (a.c[:, 4:].cuda(), True)}); got['a'].append(r[0])
    torch.cuda.synchronize(); sess.check(); sess.close()
    assert model.engine.synth_path == 'graph'
    for k in got:
        assert torch.equal(torch.cat(got[k]).cpu(), ref[k][0]) and torch.equal(got_eng[k][0], ref[k][0]), k
    model.engine.close()


def test_driver_wide_slots_route(tmp_path):
    """Synthesizer.synthesize with mi355_synthesis_wide_slots = 40 on 45 utterances of 3 ... 16 frames: 45 wavs in input order, each the bytes of its
    one-shot reference -- synthesize(steps_per_graph = 24) with the utterance in the row (slot & 31) slot_plan gave it and the noise of the driver's seed rule;
    two route keys together raise the existing ValueError."""
    import hparams as H
    from datasets.audio import save_wavenet_wav
    from wavenet_vocoder.models.wavenet import WaveNet, slot_plan
    from wavenet_vocoder.synthesizer import Synthesizer, _interp
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],wavenet_synthesis_batch_size=64')
    rng = np.random.RandomState(5)
    U = 45
    frames = [3 + (5 * i) % 14 for i in range(U)]                            # 3 ... 16; slot b + 32 does not repeat slot b's length
    mels = [rng.uniform(-4, 4, size=(frames[i], 16)).astype(np.float32) for i in range(U)]
    names = ['mel-%02d' % i for i in range(U)]
    hp0 = H._build(); hp0.parse(base + ',mi355_synthesis_wide_slots=40')
    model = WaveNet(hp0)
    model.build(32, 16 * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    # the references: the same weights, the rows and seeds the driver's plan gives
    cfg = oracle_cfg(hp0)
    rng_ = (-hp0.max_abs_value, hp0.max_abs_value) if hp0.symmetric_mels else (0, hp0.max_abs_value)
    seed0 = ((int(hp0.wavenet_random_seed) << 20) + 1) << 20
    utts, k = [], 0
    for opens, fr, fin in slot_plan(frames, 40, 8):
        for b, u in opens:
            m = np.clip(mels[u], rng_[0], rng_[1]) if hp0.clip_for_wavenet else mels[u]
            m = _interp(m, rng_).astype(np.float32) if hp0.normalize_for_wavenet else m
            utts.append(Utt('u%d' % u, b, torch.from_numpy(np.ascontiguousarray(m.T)), k, seed=seed0 + u))
        k += 1
    assert len(utts) == U and any(u.slot >= 32 for u in utts)
    model._ensure_packed()
    ref = _tile_reference(model.engine, cfg, utts)
    model.engine.close()
    od = str(tmp_path / 'out'); os.makedirs(od)
    s = Synthesizer(); s.load(ckpt, hp0)
    files = s.synthesize(mels, None, names, od, None)
    assert s.model.engine.synth_path == 'graph'
    s.model.engine.close()
    assert [os.path.basename(f) for f in files] == ['wavenet-audio-%s.wav' % n for n in names]
    for i, f in enumerate(files):
        want = str(tmp_path / 'ref.wav')
        save_wavenet_wav(ref['u%d' % i][0].float().numpy(), want, sr=hp0.sample_rate)
        assert open(f, 'rb').read() == open(want, 'rb').read(), 'utterance %d differs from its one-shot reference' % i
    hp2 = H._build(); hp2.parse(base + ',mi355_synthesis_wide_slots=40,mi355_synthesis_slots=4')
    s2 = Synthesizer(); s2.load(ckpt, hp2)
    with pytest.raises(ValueError, match='mi355_synthesis_slots and mi355_synthesis_wide_slots are both > 0: choose one'):
        s2.synthesize(mels[:2], None, names[:2], od, None)
    if s2.model.engine is not None:
        s2.model.engine.close()
