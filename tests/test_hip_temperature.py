"""Sampling temperature on the device: wn_temper_noise against the float64 mirror, and the contract of the header -- a device-noise run at a
temperature is, bit for bit, the run at (1, 1) on fill_noise + temper_noise; caller noise is tempered into the context's buffer; streams and slots
temper push by push (slots: column by column); temperature 0 is the greedy decode -- on the persistent pipeline, the launch-per-layer path and the
fp32 mode, for all three heads."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import temper_util as TU
from hip_util import SMALL, make_hp, oracle_cfg, synth_batch, upload_params
from test_hip_synth import _noise, _setup
from test_hip_synth_slots import Utt, _mels, _reference, _session
from test_hip_synth_stream import WN_E_SHAPE, WN_E_STATE, _alloc, _oneshot, _same, _stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WN_E_ARG = -1
HEADS = {'mol': dict(out_channels=30), 'gauss': dict(out_channels=2),
         'softmax': dict(input_type='mulaw-quantize', quantize_channels=256, out_channels=256)}
PATHS = {'pipeline': dict(spg=0), 'launch-per-layer': dict(spg=32)}
B, TC = 3, 8
TAU = (0.7, 0.85)


def _engine(head, inference_only=False, **kw):
    if not inference_only:
        return _setup(B, TC, **dict(HEADS[head], **kw))
    from oracle import wavenet_oracle as O
    from wavenet_vocoder import _ext
    hp = make_hp(**dict(SMALL, **dict(HEADS[head], **kw)))
    cfg = oracle_cfg(hp)
    T = TC * cfg.hop
    eng = _ext.Engine(hp, B, T, inference_only=True)
    params = O.init_params(cfg, seed=11, bias_scale=0.05)
    eng.pack_weights(upload_params(eng, params))
    wav, c = synth_batch(cfg, B, T, seed=3)
    return hp, cfg, eng, params, wav, c, T


def _filled(eng, T, nb, seed):
    nz = torch.empty(T, nb, eng.noise_per_step, device='cuda')
    eng.fill_noise(nz, nb, T, seed)
    return nz


def _expect_path(conf, path):
    if path == 'pipeline':
        assert conf['path'] == 'pipeline', conf
    else:
        assert conf['path'] in ('graph', 'graph-fp32'), conf


def _code(fn):
    from wavenet_vocoder import _ext
    with pytest.raises(_ext.WnError) as ei:
        fn()
    return ei.value.code


# ---- 1. the stand-alone kernel
def test_temper_noise_kernel_against_the_float64_mirror():
    """The accuracy test of tests/test_temperature_cpu.py on the device, same bound and temperatures, on fill_noise output of 2^20 elements for the
    MoL and the softmax row length; the Gaussian head is one float32 product; in place == out of place; a buffer off the 16-byte grid takes
    the element-wise kernel and gives the same bits.  Worst normalised errors -> profiles/temperature_parity.json."""
    report = {'note': 'worst normalised error (tests/temper_util.py) of wn_temper_noise on the device and of the numpy float32 yardstick, over tau in %s' % (TU.TAUS,)}
    for head, T in (('mol', 95326), ('softmax', 4096)):
        hp, cfg, eng, params, wav, c, _ = _engine(head)
        nps = eng.noise_per_step
        nz = _filled(eng, T, 1, 77)
        assert nz.numel() >= 1 << 20
        u = nz.cpu().numpy().reshape(T, nps)
        kinds = TU.kinds(TU.MOL if head == 'mol' else TU.SOFTMAX, nps)
        worst = {}
        for tau in TU.TAUS:
            got = eng.temper_noise(nz, tau, tau)
            inplace = eng.temper_noise(nz.clone(), tau, tau)
            ip = nz.clone(); eng.temper_noise(ip, tau, tau, out=ip)
            assert torch.equal(got, inplace) and torch.equal(got, ip)
            g = got.cpu().numpy().reshape(T, nps)
            assert g.min() >= TU.LO and g.max() <= TU.HI
            for kind in sorted(set(kinds.tolist())):
                cols = np.nonzero(kinds == kind)[0]
                uk, gk = u[:, cols].reshape(-1), g[:, cols].reshape(-1)
                w = worst.setdefault(kind, [0.0, 0.0])
                w[0] = max(w[0], TU.worst_error(uk, gk, kind, tau))
                w[1] = max(w[1], TU.worst_error(uk, TU.temper_kind(uk, kind, tau, np.float32), kind, tau))
        # a buffer that starts off the 16-byte grid (and an element count that is no multiple of 4)
        flat = torch.empty(1 + (T - 1) * nps, device='cuda')
        flat[1:] = nz.reshape(-1)[:(T - 1) * nps]
        odd = eng.temper_noise(flat[1:].view(T - 1, 1, nps), 0.8, 0.8)
        assert torch.equal(odd, eng.temper_noise(nz[:T - 1].contiguous(), 0.8, 0.8))
        for kind, (dev, yard) in worst.items():
            name = {TU.SELECT: 'select', TU.LOGISTIC: 'logistic'}[kind]
            report['%s/%s' % (head, name)] = {'device': dev, 'numpy_float32': yard, 'limit': 8.0 * yard}
            print('\n%s %s entries: worst normalised error device %.3f, numpy float32 %.3f' % (head, name, dev, yard))
            assert dev <= 8.0 * yard, '%s %s: device %.3f exceeds 8 x %.3f of the float32 yardstick' % (head, name, dev, yard)
        eng.close()
    hp, cfg, eng, params, wav, c, _ = _engine('gauss')
    e = _filled(eng, 4099, 3, 5)
    for tau in (0.7, 1.5):
        got = eng.temper_noise(e, tau, 0.3)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), (np.float32(tau) * e.cpu().numpy()).view(np.uint32))
    ip = e.clone(); eng.temper_noise(ip, 0.7, 1.0, out=ip)
    assert torch.equal(ip, eng.temper_noise(e, 0.7, 1.0))
    assert torch.equal(eng.temper_noise(e, 1.0, 1.0), e)
    assert _code(lambda: eng.temper_noise(e, 3.0, 1.0)) == WN_E_ARG and _code(lambda: eng.temper_noise(e, 1.0, float('nan'))) == WN_E_ARG
    with open(os.path.join(ROOT, 'profiles', 'temperature_parity.json'), 'w') as f:
        json.dump(report, f, indent=1, sort_keys=True)


@pytest.mark.parametrize('head,T,nb', [('mol', 4099, 5), ('softmax', 259, 3), ('gauss', 4099, 5)])
def test_fused_fill_equals_fill_then_temper(head, T, nb):
    """the fill kernel of a device-noise run at a pair (sizes that are no multiple of the four elements a thread generates, rows that straddle them)"""
    hp, cfg, eng, params, wav, c, _ = _engine(head)
    for pair in (TAU, (1.0, 0.5), (0.5, 1.0), (0.0, 0.0), (2.0, 2.0), (1.0, 1.0)):
        fused = eng.fill_noise_tempered(torch.empty(T, nb, eng.noise_per_step, device='cuda'), nb, T, 9, *pair)
        assert torch.equal(fused, eng.temper_noise(_filled(eng, T, nb, 9), *pair)), pair


# ---- 2. device noise at a temperature == explicit tempered noise at (1, 1)
@pytest.mark.parametrize('head,path,kw', [(h, p, {}) for h in HEADS for p in PATHS] + [('mol', 'launch-per-layer', dict(mi355_compute_dtype='fp32'))],
                         ids=lambda v: v if isinstance(v, str) else ('fp32' if v else 'bf16'))
def test_device_noise_equals_explicit_tempered_noise(head, path, kw):
    hp, cfg, eng, params, wav, c, T = _engine(head, **kw)
    spg = PATHS[path]['spg']
    assert eng.temperature == (1.0, 1.0)
    plain = _oneshot(eng, cfg, c, seed=5, spg=spg)
    eng.set_temperature(*TAU)
    assert eng.temperature == tuple(float(np.float32(t)) for t in TAU)
    a = _oneshot(eng, cfg, c, seed=5, spg=spg)
    _expect_path(a[2], path)
    eng.set_temperature(1.0, 1.0)
    nz = eng.temper_noise(_filled(eng, T, B, 5), *TAU)
    b = _oneshot(eng, cfg, c, noise=nz, spg=spg)
    _same(a, b)
    assert not torch.equal(a[0], plain[0]), 'the temperature changed nothing'


# ---- 3. caller noise at a temperature == pre-tempered caller noise at (1, 1); the caller's buffer is not written
@pytest.mark.parametrize('head,path', [('mol', 'pipeline'), ('softmax', 'launch-per-layer')])
def test_caller_noise_is_tempered_into_the_context(head, path):
    hp, cfg, eng, params, wav, c, T = _engine(head)
    spg = PATHS[path]['spg']
    nz = _noise(cfg, T, B, seed=4)[0].cuda()
    keep = nz.clone()
    eng.set_temperature(*TAU)
    a = _oneshot(eng, cfg, c, noise=nz, spg=spg)
    _expect_path(a[2], path)
    assert torch.equal(nz, keep), 'the caller\'s noise was written'
    eng.set_temperature(1.0, 1.0)
    b = _oneshot(eng, cfg, c, noise=eng.temper_noise(nz, *TAU), spg=spg)
    _same(a, b)


# ---- 4. (1, 1) is the behaviour of a context that never heard of temperature
def test_back_to_one_is_a_fresh_context():
    hp, cfg, eng, params, wav, c, T = _engine('mol')
    nz = _noise(cfg, T, B, seed=4)[0]
    eng.set_temperature(0.5, 0.5)
    _oneshot(eng, cfg, c, seed=8)
    _oneshot(eng, cfg, c, noise=nz)
    eng.set_temperature(1.0, 1.0)
    dev, call = _oneshot(eng, cfg, c, seed=8), _oneshot(eng, cfg, c, noise=nz)
    eng.close()
    hp, cfg, fresh, params, wav, c, T = _engine('mol')
    _same(dev, _oneshot(fresh, cfg, c, seed=8))
    _same(call, _oneshot(fresh, cfg, c, noise=nz))


# ---- 5. streams
@pytest.mark.parametrize('head,path', [('mol', 'pipeline'), ('gauss', 'launch-per-layer')])
def test_stream_at_a_temperature_equals_the_one_shot(head, path):
    hp, cfg, eng, params, wav, c, T = _engine(head)
    spg, hop = PATHS[path]['spg'], cfg.hop
    eng.set_temperature(*TAU)
    ref = _oneshot(eng, cfg, c, seed=13, spg=spg)
    got = _stream(eng, cfg, c, [1, 3, 4], seed=13, spg=spg)
    _expect_path(got[2], path)
    _same(got, ref)
    cn = _noise(cfg, T, B, seed=4)[0]                                                        # caller noise: every push reads a tempered copy of its rows
    _same(_stream(eng, cfg, c, [1, 3, 4], noise=cn, spg=spg), _oneshot(eng, cfg, c, noise=cn, spg=spg))
    # the pair changes between two pushes: the stream stays open and every push is tempered by the pair of ITS time
    later = (0.4, 0.6)
    got = _stream(eng, cfg, c, [1, 3, 4], seed=13, spg=spg, between=lambda i: eng.set_temperature(*later) if i == 0 else None)
    eng.set_temperature(1.0, 1.0)
    nz = _filled(eng, T, B, 13)
    mixed = torch.cat([eng.temper_noise(nz[:hop].contiguous(), *TAU), eng.temper_noise(nz[hop:].contiguous(), *later)])
    ref2 = _oneshot(eng, cfg, c, noise=mixed, spg=spg)
    _same(got, ref2)
    assert torch.equal(got[0][:, :hop], ref[0][:, :hop]) and not torch.equal(got[0][:, hop:], ref[0][:, hop:])


# ---- 6. slots
@pytest.mark.parametrize('path', list(PATHS))
def test_slots_temper_column_by_column(path):
    hp, cfg, eng, params, wav, c, T = _engine('mol')
    spg, hop, tick = PATHS[path]['spg'], cfg.hop, 2
    pairs = {'a': (1.0, 1.0), 'b': (0.6, 0.9), 'c': (0.0, 0.0), 'd': (0.8, 0.8)}
    override = (1.0, 0.25)
    utts = [Utt('a', 0, _mels(cfg, 8, 1), 0, seed=41), Utt('b', 1, _mels(cfg, 7, 2), 0, seed=42), Utt('c', 2, _mels(cfg, 3, 3), 2, seed=43),
            Utt('d', 2, _mels(cfg, 5, 4), 3, seed=44)]                                      # d takes slot 2 once c has finished
    by_seed = {u.seed: u.name for u in utts}
    # references: column b of the noise = fill_noise(B = 1, seed_b) tempered by the slot's pair, push by push
    eng.set_temperature(1.0, 1.0)
    ref_utts = []
    for u in utts:
        n = u.Tc * hop
        one = _filled(eng, n, 1, u.seed)
        if u.name == 'd':                                                                   # its first push (tick frames) at the pair of its open, the rest overridden
            col = torch.cat([eng.temper_noise(one[:tick * hop].contiguous(), *pairs['d']), eng.temper_noise(one[tick * hop:].contiguous(), *override)])
        else:
            col = eng.temper_noise(one, *pairs[u.name])
        ref_utts.append(Utt(u.name, u.slot, u.c, u.open_at, seed=u.seed, noise=col[:, 0].cpu()))
    ref, _ = _reference(eng, cfg, B, ref_utts, spg=spg, device_noise=False)
    # the session: the context's pair at slot_open is the slot's; d is overridden after its first push
    opened, state = [], {}
    raw_open = eng.slot_open

    def slot_open(slot, seed=0, g=None):
        eng.set_temperature(*pairs[by_seed[seed]])
        raw_open(slot, seed=seed, g=g)
        eng.set_temperature(0.3, 0.3)                                                       # (what the context holds afterwards does not reach a live slot)
        opened.append(by_seed[seed])

    def between(k):
        if 'd' in opened and 'done' not in state:
            eng.slot_temperature(2, *override)
            state['done'] = k
    eng.slot_open = slot_open
    try:
        got, conf, pushes = _session(eng, cfg, B, utts, spg=spg, tick=tick, between=between)
    finally:
        del eng.slot_open
    _expect_path(conf, path)
    assert opened == ['a', 'b', 'c', 'd'] and 'done' in state
    for name in ('a', 'b', 'c', 'd'):
        assert torch.equal(got[name][0], ref[name][0]), '%s: samples differ at %d positions' % (name, int((got[name][0] != ref[name][0]).sum()))
        assert torch.equal(got[name][1], ref[name][1]), '%s: raw outputs differ' % name
    # errors
    eng.set_temperature(1.0, 1.0)
    assert _code(lambda: eng.slot_temperature(0, 0.5, 0.5)) == WN_E_STATE                   # no session (the one above has ended)
    eng.slots_begin(B, steps_per_graph=spg)
    assert _code(lambda: eng.slot_temperature(1, 0.5, 0.5)) == WN_E_STATE                   # an idle slot
    eng.slot_open(1, seed=1)
    assert _code(lambda: eng.slot_temperature(1, 3.0, 1.0)) == WN_E_ARG
    assert _code(lambda: eng.slot_temperature(B, 0.5, 0.5)) == WN_E_ARG
    eng.slot_temperature(1, 0.5, 0.5)
    eng.slots_end()


def test_slots_temper_caller_noise_column_by_column():
    """a session fed explicit noise: the push's [n_max, B, nps] buffer is tempered into the context's, every column by its slot's pair; the
    caller's buffers are not written"""
    hp, cfg, eng, params, wav, c, T = _engine('mol')
    hop, nps = cfg.hop, eng.noise_per_step
    pairs = {41: (1.0, 1.0), 42: (0.6, 0.9), 43: (0.0, 0.3)}
    utts, ref_utts = [], []
    for name, slot, Tc, open_at, seed in (('a', 0, 8, 0, 41), ('b', 1, 7, 0, 42), ('c', 2, 5, 1, 43)):
        nz = _noise(cfg, Tc * hop, 1, seed=seed)[0][:, 0].contiguous()                        # [n, nps]
        mel = _mels(cfg, Tc, seed)
        utts.append(Utt(name, slot, mel, open_at, seed=seed, noise=nz))
        ref_utts.append(Utt(name, slot, mel, open_at, seed=seed, noise=eng.temper_noise(nz.view(-1, 1, nps).cuda(), *pairs[seed])[:, 0].cpu()))
    keep = [u.noise.clone() for u in utts]
    ref, _ = _reference(eng, cfg, B, ref_utts, device_noise=False)
    raw_open = eng.slot_open

    def slot_open(slot, seed=0, g=None):
        eng.set_temperature(*pairs[seed])
        raw_open(slot, seed=seed, g=g)
    eng.slot_open = slot_open
    try:
        got, conf, _ = _session(eng, cfg, B, utts, seed=3)
    finally:
        del eng.slot_open
    for u, k in zip(utts, keep):
        assert torch.equal(u.noise, k)
        assert torch.equal(got[u.name][0], ref[u.name][0]) and torch.equal(got[u.name][1], ref[u.name][1]), u.name


# ---- 7. temperature 0 is deterministic and greedy
def _greedy_disagreements(logits, chosen):
    """positions where `chosen` is not the first arg-max of logits [N, K]; each must be a near-tie (the sampler adds one tiny constant to every logit
    before it compares): the two largest logits closer than 2^-20 max(1, |logit|)"""
    best = np.argmax(logits, axis=1)
    bad = np.nonzero(best != chosen)[0]
    for i in bad:
        top = np.sort(logits[i])[-2:]
        assert chosen[i] in np.argsort(logits[i])[-2:] and top[1] - top[0] < 2.0 ** -20 * max(1.0, abs(float(top[1]))), (i, top, best[i], chosen[i])
    return len(bad)


@pytest.mark.parametrize('head', list(HEADS))
def test_temperature_zero_is_the_greedy_decode(head):
    from wavenet_vocoder import _ext
    hp, cfg, eng, params, wav, c, T = _engine(head)
    eng.set_temperature(0.0, 0.0)
    a, b = _oneshot(eng, cfg, c, seed=1), _oneshot(eng, cfg, c, seed=2)
    _expect_path(a[2], 'pipeline')
    _same(a, b)
    out, raw = a[0].numpy(), a[1].numpy()                                                    # [B, T], [B, O, T]
    N = B * T
    if head == 'softmax':
        ids = _ext.argmax_channels(a[1].cuda()).cpu().numpy()
        nbad = _greedy_disagreements(raw.transpose(0, 2, 1).reshape(N, -1), out.reshape(N))
        assert nbad == int((ids != out).sum())
    elif head == 'gauss':
        nbad = 0
        assert np.array_equal(out, np.clip(raw[:, 0], -1.0, 1.0))
    else:
        M = cfg.out_channels // 3
        logits, mu = raw[:, :M].transpose(0, 2, 1).reshape(N, M), raw[:, M:2 * M].transpose(0, 2, 1).reshape(N, M)
        x = out.reshape(N)
        chosen = np.argmax(logits, axis=1)
        miss = np.nonzero(np.clip(mu[np.arange(N), chosen], -1.0, 1.0) != x)[0]
        for i in miss:                                                                      # not the arg-max component's mean: the runner-up's, at a near-tie
            second = np.argsort(logits[i])[-2]
            assert np.clip(mu[i, second], -1.0, 1.0) == x[i]
            chosen[i] = second
        nbad = _greedy_disagreements(logits, chosen)
    assert nbad <= 0.01 * N
    assert nbad == 0, 'this model has no near-tie'


# ---- 8. teacher forced: the logistic draw scales by tau
def test_teacher_forced_draw_scales_with_the_temperature():
    hp, cfg, eng, params, wav, c, T = _engine('mol')
    M = cfg.out_channels // 3
    nz = _noise(cfg, T, B, seed=6)[0]
    ti = wav.cuda().contiguous()
    eng.set_temperature(0.5, 1.0)
    xt, rt, _ = _oneshot(eng, cfg, c, noise=nz, ti=ti)
    eng.set_temperature(1.0, 1.0)
    x1, r1, _ = _oneshot(eng, cfg, c, noise=nz, ti=ti)
    assert torch.equal(rt, r1)                                                               # teacher forcing: the network outputs do not see the samples
    N = B * T
    raw = r1.numpy().astype(np.float64)
    u = nz.numpy().transpose(1, 0, 2).reshape(N, M + 1)                                      # [B, T] order like the outputs
    logits = raw[:, :M].transpose(0, 2, 1).reshape(N, M)
    mu = raw[:, M:2 * M].transpose(0, 2, 1).reshape(N, M)
    ls = np.maximum(raw[:, 2 * M:].transpose(0, 2, 1).reshape(N, M), float(hp.log_scale_min))
    bi = np.argmax(logits + TU.gumbel(u[:, :M]), axis=1)
    r = np.arange(N)
    mu, sc, u2 = mu[r, bi], np.exp(ls[r, bi]), u[:, M]
    xt, x1 = xt.numpy().reshape(N).astype(np.float64), x1.numpy().reshape(N).astype(np.float64)
    free = (np.abs(xt) < 1.0) & (np.abs(x1) < 1.0)
    assert free.sum() >= 64                                                                  # (this model clips about half of its samples: enough are left)
    ref = 0.5 * TU.logit(u2)
    s_l = TU.floor_logistic(TU.temper_kind(u2, TU.LOGISTIC, 0.5), ref)
    # the chosen components are identical: both samples are draws of component bi
    assert np.all(np.abs((x1 - mu) - sc * TU.logit(u2))[free] <= sc[free] * 16 * TU.floor_logistic(u2.astype(np.float64), TU.logit(u2))[free] + 2.0 ** -22)
    d = np.abs((xt - mu) - 0.5 * (x1 - mu))
    print('\nworst |(x_tau - mu) - tau (x_1 - mu)| / (exp(ls) 16 s_l) = %.3f over %d unclipped positions' % (float((d / (sc * 16 * s_l))[free].max()), int(free.sum())))
    assert np.all(d[free] <= (sc * 16 * s_l)[free])


# ---- 9. façade and driver
def test_facade_incremental_temperature_equals_engine_calls():
    from wavenet_vocoder.models.wavenet import WaveNet
    hp, cfg, eng, params, wav, c, T = _engine('mol')
    eng.set_temperature(0.7, 1.0)
    flat = upload_params(eng, params)
    model = WaveNet(hp)
    model.build(B, T, params=flat.cpu())
    out, raw = model.incremental(None, c=c.cuda(), temperature=0.7, return_raw=True, check=True)
    assert model.engine.temperature == (float(np.float32(0.7)), 1.0)
    seed = ((int(hp.wavenet_random_seed) << 20) + model._synth_calls) * 64
    ref = _oneshot(eng, cfg, c, seed=seed)
    assert torch.equal(out.cpu(), ref[0]) and torch.equal(raw.cpu(), ref[1])
    nz = _noise(cfg, T, B, seed=2)[0].cuda()
    out = model.incremental(None, c=c.cuda(), temperature=0.7, mixture_temperature=0.0, noise=nz, check=True)
    eng.set_temperature(0.7, 0.0)
    assert torch.equal(out.cpu(), _oneshot(eng, cfg, c, noise=nz)[0])
    with pytest.raises(_ext_error()):
        model.incremental(None, c=c.cuda(), temperature=2.5)


def _ext_error():
    from wavenet_vocoder import _ext
    return _ext.WnError


def test_synthesize_driver_temperature_zero(tmp_path):
    """wavenet_synthesize on the tiny model of the slot driver test with both temperature keys 0: the wavs do not depend on wavenet_random_seed
    (padded batches and a slot session, each against itself); at temperature 1 they do."""
    import types
    import hparams as H
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
    runs = (('z1/', 0.0, 1234, 0), ('z2/', 0.0, 4321, 0), ('z3/', 0.0, 1234, 4), ('z4/', 0.0, 4321, 4), ('one/', 1.0, 4321, 0))
    cwd = os.getcwd(); os.chdir(root)
    try:
        for od, tau, seed, slots in runs:
            hp.set_hparam('mi355_synthesis_temperature', tau); hp.set_hparam('mi355_synthesis_mixture_temperature', tau)
            hp.set_hparam('wavenet_random_seed', seed); hp.set_hparam('mi355_synthesis_slots', slots)
            wavenet_synthesize(types.SimpleNamespace(model='WaveNet', mels_dir=mels_dir, output_dir=od, speaker_id=None), hp, save_dir)
    finally:
        os.chdir(cwd)

    def wavs(od):
        d = os.path.join(root, 'wavenet_' + od, 'wavs')
        return {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d)) if f.endswith('.wav')}
    z1, z2, z3, z4, one = wavs('z1'), wavs('z2'), wavs('z3'), wavs('z4'), wavs('one')
    assert len(z1) == 3 and z1 == z2
    assert len(z3) == 3 and z3 == z4, 'the slot session\'s greedy decode depends on the seed'
    assert sorted(one) == sorted(z1) and all(one[f] != z1[f] for f in z1)


# ---- 10. an inference-only context never allocates for it
def test_inference_only_context_tempers_into_its_presized_buffer():
    from wavenet_vocoder import _ext
    hp, cfg, eng, params, wav, c, T = _engine('mol', inference_only=True)
    nz = _noise(cfg, T, B, seed=4)[0].cuda()
    res = (ctypes.c_int64 * 5)()
    _oneshot(eng, cfg, c, noise=nz)                                                          # (the first run: everything lazy is behind us)
    assert eng.lib.wn_test_device_resources(res) == 0
    before = list(res)
    eng.set_temperature(*TAU)
    a = _oneshot(eng, cfg, c, noise=nz)
    assert eng.lib.wn_test_device_resources(res) == 0
    assert (res[0], res[4]) == (before[0], before[4]), 'the tempered run allocated: live buffers / allocations ever %s -> %s' % (before, list(res))
    eng.set_temperature(1.0, 1.0)
    _same(a, _oneshot(eng, cfg, c, noise=eng.temper_noise(nz, *TAU)))
    # beyond the pre-sized shape: still WN_E_SHAPE
    eng.set_temperature(*TAU)
    c2 = synth_batch(cfg, B, 2 * T, seed=3)[1]
    nz2 = _noise(cfg, 2 * T, B, seed=4)[0].cuda()
    out, raw = _alloc(eng, cfg, B, 2 * T)
    assert _code(lambda: eng.synthesize(c2.cuda(), nz2, out, raw)) == WN_E_SHAPE
