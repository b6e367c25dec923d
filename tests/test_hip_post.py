"""Output stage on the device (csrc/wn_post.hip): wn_post_push / wn_post_finish against the numpy mirror of tests/post_util.py bit for bit -- float
output, int16 and clip counts; ragged rows across the 4096-sample LDS block, the 4-sample vector width and the 32-row launch group; sentinels beyond
a row's length; independence of how rows are cut into pushes, restart, finish beside a running push sequence, gain and clamp, the decode against
wn_inv_mulaw / wn_inv_mulaw_quantize, determinism, the validation on a real handle, the four synthesis routes with post= and the driver's hparams."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import post_util as PU
from hip_util import upload_params

pytestmark = pytest.mark.gpu

WN_E_ARG, WN_E_SHAPE = -1, -2
K = 0.97
ORDER = [4099, 0, 65, 1024, 1, 1023, 63, 1025, 64]      # n of row b = ORDER[b % 9]: B = 1 takes the longest, B = 3 an empty row, 32 / 33 all of them
TORCH_IN = {0: torch.float32, 1: torch.float32, 2: torch.int32}


def _stage(rows, in_type, k=K, gain=1.0):
    from wavenet_vocoder import _ext
    import hparams as H
    return _ext.OutputStage(H._build(), rows, deemphasis=k, gain=gain, in_type=in_type)


@functools.lru_cache(maxsize=None)
def _row(in_type, b, gain=1.0):
    """input and mirror of row b at K from y[-1] = 0: (a, y, int16, clipped, carry) -- computed once, shared, never modified"""
    a = PU.samples(in_type, ORDER[b % 9], seed=1000 * in_type + b)
    res = (a,) + PU.mirror_push(in_type, a, K, gain=gain)
    for t in res[:3]:
        t.setflags(write=False)
    return res


def _pack(rows, pitch, dtype, fill=0):
    t = torch.full((len(rows), pitch), fill, dtype=dtype)
    for b, a in enumerate(rows):
        t[b, :len(a)] = torch.from_numpy(np.array(a))
    return t.cuda()


def _push(st, samples, n, restart=None, want_y=True, want_q=True):
    """wn_post_push into sentinel-filled outputs of the input's pitch -> (y, q, clipped) on the host"""
    from wavenet_vocoder import _ext
    B, pitch = samples.shape
    y = torch.full((B, pitch), -77.0, device='cuda') if want_y else None
    q = torch.full((B, pitch), -77, dtype=torch.int16, device='cuda') if want_q else None
    cl = torch.full((B,), -77, dtype=torch.int32, device='cuda')
    rs = None if restart is None else (ctypes.c_int32 * B)(*[int(v) for v in restart])
    rc = st.lib.wn_post_push(st.h, _ext._ptr(samples), pitch, (ctypes.c_int32 * B)(*n), rs, B, _ext._ptr(y), _ext._ptr(q), pitch, _ext._ptr(cl), _ext._stream())
    assert rc == 0, st.lib.wn_post_last_error(st.h)
    torch.cuda.synchronize()
    return (None if y is None else y.cpu().numpy()), (None if q is None else q.cpu().numpy()), cl.cpu().numpy()


def _case_mirror(in_type, B):
    n = [ORDER[b % 9] for b in range(B)]
    pitch = max(n) + 5
    st = _stage(B, in_type)
    y, q, cl = _push(st, _pack([_row(in_type, b)[0] for b in range(B)], pitch, TORCH_IN[in_type]), n, restart=[1] * B)
    st.close()
    return n, y, q, cl


@pytest.mark.parametrize('B', [1, 3, 32, 33])
@pytest.mark.parametrize('in_type', [0, 1, 2])
def test_push_equals_the_mirror(in_type, B):
    n, y, q, cl = _case_mirror(in_type, B)
    for b in range(B):
        _, my, mq, mclip, _ = _row(in_type, b)
        assert np.array_equal(PU.bits(y[b, :n[b]]), PU.bits(my)), b
        assert np.array_equal(q[b, :n[b]], mq) and cl[b] == mclip, b
        assert np.all(y[b, n[b]:] == -77.0) and np.all(q[b, n[b]:] == -77), b            # beyond n[b]: the caller's bytes


CUTS = ([7, 1018, 0, 3074], [1024, 1, 4096 - 1025, 3], [4099, 0, 0, 0], [5, 4090, 2, 2])      # per row, 4 pushes each; row 0 has an empty push, row 2 three


def _case_boundaries(in_type):
    rows = [PU.samples(in_type, 4099, seed=50 + b) for b in range(4)]
    st = _stage(4, in_type)
    one = _push(st, _pack(rows, 4099, TORCH_IN[in_type]), [4099] * 4, restart=[1] * 4)
    parts_y, parts_q, t0 = [[] for _ in rows], [[] for _ in rows], [0] * 4
    for i in range(4):
        n = [CUTS[b][i] for b in range(4)]
        y, q, _ = _push(st, _pack([rows[b][t0[b]:t0[b] + n[b]] for b in range(4)], max(max(n), 1) + i, TORCH_IN[in_type]), n, restart=[i == 0] * 4)
        for b in range(4):
            parts_y[b].append(y[b, :n[b]]); parts_q[b].append(q[b, :n[b]]); t0[b] += n[b]
    st.close()
    return rows, one, [np.concatenate(p) for p in parts_y], [np.concatenate(p) for p in parts_q]


@pytest.mark.parametrize('in_type', [0, 1, 2])
def test_rows_cut_into_pushes_equal_one_push(in_type):
    rows, one, ys, qs = _case_boundaries(in_type)
    for b in range(4):
        assert np.array_equal(PU.bits(ys[b]), PU.bits(one[0][b])) and np.array_equal(qs[b], one[1][b]), b
        my, mq, _, _ = PU.mirror_push(in_type, rows[b], K)
        assert np.array_equal(PU.bits(one[0][b]), PU.bits(my)) and np.array_equal(one[1][b], mq), b


def _case_restart():
    a = [PU.samples(0, 700, seed=70 + b) for b in range(3)]
    fresh = PU.samples(0, 300, seed=80)
    st = _stage(3, 0)
    _push(st, _pack([r[:400] for r in a], 400, torch.float32), [400] * 3, restart=None)          # (a new stage starts from zero state)
    y, q, _ = _push(st, _pack([a[0][400:], fresh, a[2][400:]], 300, torch.float32), [300] * 3, restart=[0, 1, 0])
    y2, _, _ = _push(st, _pack([a[0][:1]] * 3, 1, torch.float32), [0, 0, 0], restart=[0, 0, 1])    # an empty push that restarts row 2 ...
    y3, _, _ = _push(st, _pack([fresh[:9]] * 3, 9, torch.float32), [9, 0, 9], restart=None)        # ... which then starts afresh; row 0 runs on; row 1 untouched
    st.close()
    return a, fresh, y, q, y3


def test_restart_of_one_row_leaves_its_neighbours_running():
    a, fresh, y, q, y3 = _case_restart()
    for b in (0, 2):
        assert np.array_equal(PU.bits(y[b]), PU.bits(PU.chain(a[b], K)[0][400:])), b
    assert np.array_equal(PU.bits(y[1]), PU.bits(PU.chain(fresh, K)[0]))
    assert np.array_equal(PU.bits(y3[2]), PU.bits(PU.chain(fresh[:9], K)[0]))
    assert np.array_equal(PU.bits(y3[0]), PU.bits(PU.chain(np.concatenate([a[0], fresh[:9]]), K)[0][700:]))
    assert np.all(y3[1] == -77.0)


def _case_finish(in_type):
    B = 5
    n = [4099, 0, 1025, 64, 2500]
    rows = [PU.samples(in_type, n[b], seed=90 + b) for b in range(B)]
    if in_type == 0:
        rows[2] = (rows[2] * np.float32(0.0005)).astype(np.float32)                    # a peak under the 0.01 floor
    st = _stage(B, in_type)
    run = PU.samples(in_type, 900, seed=99)
    first = _push(st, _pack([run[:500]] * B, 500, TORCH_IN[in_type]), [500] * B, restart=[1] * B)
    fill = {0: 5.0, 1: 0.999, 2: 0}[in_type]                                           # beyond n[b] the input holds the loudest value there is: it must not reach the peak
    y, q, pk = st.finish(_pack(rows, max(n) + 5, TORCH_IN[in_type], fill), n, peak=True)       # in between: neither reads nor writes the carried state
    second = _push(st, _pack([run[500:]] * B, 400, TORCH_IN[in_type]), [400] * B)
    y2 = st.finish(_pack(rows, max(n) + 5, TORCH_IN[in_type], fill), n, pcm=False)
    torch.cuda.synchronize()
    st.close()
    return n, rows, run, y.cpu().numpy(), q.cpu().numpy(), pk.cpu().numpy(), np.concatenate([first[0], second[0]], 1), y2.cpu().numpy()


@pytest.mark.parametrize('in_type', [0, 1, 2])
def test_finish_peak_normalises_as_save_wavenet_wav_and_keeps_the_pushed_state(in_type):
    n, rows, run, y, q, pk, pushed, y2 = _case_finish(in_type)
    for b in range(len(n)):
        my, mq, mpeak = PU.mirror_finish(in_type, rows[b], K)
        assert np.array_equal(PU.bits(y[b, :n[b]]), PU.bits(my)) and PU.bits(pk[b]) == PU.bits(mpeak), b
        assert pk[b] == (np.max(np.abs(y[b, :n[b]])) if n[b] else 0.0)                   # the peak over n[b], not over the pitch
        assert np.array_equal(q[b, :n[b]], PU.save_wavenet_wav_pcm(y[b, :n[b]])), b      # save_wavenet_wav's arithmetic on the device's own y
        assert np.array_equal(q[b, :n[b]], mq) and np.all(q[b, n[b]:] == 0) and np.all(y[b, n[b]:] == 0), b
        assert np.array_equal(PU.bits(pushed[b]), PU.bits(PU.chain(PU.decode(in_type, run), K)[0])), b
    assert np.array_equal(PU.bits(y2), PU.bits(y))


def _case_gain():
    B = 3
    rows = [PU.samples(0, 4099, seed=60 + b) for b in range(B)]
    st = _stage(B, 0, gain=4.0)
    y, q, cl = _push(st, _pack(rows, 4099, torch.float32), [4099] * B, restart=[1] * B)
    qo = _push(st, _pack(rows, 4099, torch.float32), [4099, 0, 7], restart=[1] * B, want_y=False)[1]      # PCM alone
    st.close()
    return rows, y, q, cl, qo


def test_gain_clamps_and_counts_the_clipped_samples():
    rows, y, q, cl, qo = _case_gain()
    for b, a in enumerate(rows):
        my, mq, mclip, _ = PU.mirror_push(0, a, K, gain=4.0)
        assert np.array_equal(q[b], mq) and cl[b] == mclip and mclip > 1000
        assert q[b].max() == 32767 and q[b].min() == -32767
    assert np.array_equal(qo[0], q[0]) and np.all(qo[1] == -77) and np.array_equal(qo[2, :7], q[2, :7]) and np.all(qo[2, 7:] == -77)


def _case_decode():
    from wavenet_vocoder import _ext
    res = []
    for in_type in (0, 1, 2):
        a = _pack([PU.samples(in_type, 4099, seed=30 + in_type), PU.samples(in_type, 4099, seed=40 + in_type)], 4099, TORCH_IN[in_type])
        if in_type == 0:
            a[0, 0], a[0, 7], a[1, 4098] = -0.0, 1e-42, -0.0
        st = _stage(2, in_type, k=0.0)
        y, _, _ = _push(st, a, [4099, 4099], restart=[1, 1])
        st.close()
        ref = a if in_type == 0 else _ext.inv_mulaw(a) if in_type == 1 else _ext.inv_mulaw_quantize(a)
        res.append((y, ref.cpu().numpy()))
    return res


def test_coefficient_zero_is_the_decode_kernels_bit_for_bit():
    for y, ref in _case_decode():
        assert np.array_equal(PU.bits(y), PU.bits(ref))


def test_two_runs_of_everything_are_bit_identical():
    def flat(x):
        if isinstance(x, (list, tuple)):
            return [t for v in x for t in flat(v)]
        return [np.asarray(x)]

    cases = [lambda: _case_mirror(2, 33), lambda: _case_mirror(1, 3), lambda: _case_boundaries(1), _case_restart, lambda: _case_finish(0), lambda: _case_finish(2),
             _case_gain, _case_decode]
    for case in cases:
        a, b = flat(case()), flat(case())
        assert len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_every_validation_code_on_a_handle():
    from wavenet_vocoder import _ext
    st = _stage(4, 2)
    lib, h = st.lib, st.h
    a = torch.zeros(5, 8, dtype=torch.int32, device='cuda')
    y = torch.zeros(5, 8, device='cuda'); q = torch.zeros(5, 8, dtype=torch.int16, device='cuda')
    P = _ext._ptr
    n3, neg = (ctypes.c_int32 * 3)(5, 0, 8), (ctypes.c_int32 * 3)(5, -1, 8)
    n5 = (ctypes.c_int32 * 5)(1, 1, 1, 1, 1)
    push = lambda i, ip, n, B, of, oq, op: lib.wn_post_push(h, P(i), ip, n, None, B, P(of), P(oq), op, None, _ext._stream())
    fin = lambda i, ip, n, B, of, oq, op: lib.wn_post_finish(h, P(i), ip, n, B, P(of), P(oq), op, None, _ext._stream())
    assert push(a, 8, n3, 3, y, q, 8) == 0 and push(a, 8, n3, 3, None, q, 8) == 0 and push(a, 8, n3, 3, y, None, 8) == 0
    assert push(None, 8, n3, 3, y, q, 8) == WN_E_ARG and push(a, 8, None, 3, y, q, 8) == WN_E_ARG
    assert push(a, 8, n3, 3, None, None, 8) == WN_E_ARG and b'both outputs' in lib.wn_post_last_error(h)
    assert push(a, 8, n3, 0, y, q, 8) == WN_E_ARG and push(a, 8, neg, 3, y, q, 8) == WN_E_ARG
    assert push(a, 8, n5, 5, y, q, 8) == WN_E_SHAPE and push(a, 7, n3, 3, y, q, 8) == WN_E_SHAPE and push(a, 8, n3, 3, y, q, 7) == WN_E_SHAPE
    assert fin(a, 8, n3, 3, y, q, 8) == 0 and fin(a, 8, n3, 3, y, None, 8) == 0
    assert fin(a, 8, n3, 3, None, q, 8) == WN_E_ARG and fin(a, 8, n5, 5, y, q, 8) == WN_E_SHAPE and fin(a, 8, n3, 3, y, q, 7) == WN_E_SHAPE
    assert fin(None, 8, n3, 3, y, q, 8) == WN_E_ARG and fin(a, 8, neg, 3, y, q, 8) == WN_E_ARG and fin(a, 8, n3, 0, y, q, 8) == WN_E_ARG
    torch.cuda.synchronize()
    st.close()
    with pytest.raises(_ext.WnError) as ei:
        st2 = _stage(2, 0); st2.push(torch.zeros(3, 4, device='cuda'))
    assert ei.value.code == WN_E_SHAPE
    with pytest.raises(TypeError):
        st2.push(torch.zeros(2, 4, dtype=torch.int32, device='cuda'))
    st2.close()


# ---- the synthesis routes
HEADS = {'raw': dict(), 'mulaw-quantize': dict(input_type='mulaw-quantize', out_channels=256, quantize_channels=256)}


@pytest.mark.parametrize('head', ['raw', 'mulaw-quantize'])
def test_routes_with_a_stage_equal_the_mirror_over_their_samples(head):
    """incremental(post=) and a SynthesisStream in 3 pushes with post= give the mirror over incremental()'s samples (finish / push arithmetic); a SlotSession
    whose slot is reopened once gives the mirror over each utterance's samples, restarted at the reopening; folded(post=) the mirror over its waveforms."""
    from test_hip_synth import _setup
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.wavenet import WaveNet, fold_capacity
    B, Tc = 2, 12
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, **HEADS[head])
    flat = upload_params(eng, params).cpu()
    eng.close()
    it = _ext.INPUT_TYPES[head]
    frames = [12, 9]
    plan = _ext.fold_plan(frames, 3, 1, 1, 4)
    cap = fold_capacity(frames, plan, cfg.hop)
    model = WaveNet(hp)
    model.build(max(B, cap[0]), max(T, cap[1]), params=flat)
    fin = model.output_stage(B)
    assert (fin.in_type, round(fin.deemphasis, 6), fin.gain) == (it, 0.97, 1.0)
    ref, (fy, fq) = model.incremental(None, c=c.cuda(), time_length=T, post=fin)
    torch.cuda.synchronize()
    ref = ref.cpu().numpy()
    for b in range(B):
        my, mq, _ = PU.mirror_finish(it, ref[b], K)
        assert np.array_equal(PU.bits(fy[b].cpu().numpy()), PU.bits(my)) and np.array_equal(fq[b].cpu().numpy(), mq), b
    # stream: same seed derivation as incremental
    model._synth_calls = 0
    st, chunked = model.stream(B), model.output_stage(B, gain=0.5)
    parts = [st.push(c[:, :, a:b].cuda(), final=(b == Tc), post=chunked, post_output='both') for a, b in ((0, 3), (3, 4), (4, 12))]
    torch.cuda.synchronize()
    assert np.array_equal(torch.cat([p[0] for p in parts], 1).cpu().numpy(), ref)
    sq, sy = (torch.cat([p[1][i] for p in parts], 1).cpu().numpy() for i in (0, 1))
    for b in range(B):
        my, mq, _, _ = PU.mirror_push(it, ref[b], K, gain=0.5)
        assert np.array_equal(PU.bits(sy[b]), PU.bits(my)) and np.array_equal(sq[b], mq), b
    # slots: slot 0 carries two utterances one after the other, slot 1 one
    sess = model.slots(B)
    got = {'a': [], 'b': [], 'c': []}
    sess.open(0, seed=41); sess.open(1, seed=43)
    r = sess.push({0: c[0, :, :5].cuda(), 1: c[1, :, :2].cuda()}, post=chunked, post_output='float'); got['a'].append(r[0]); got['c'].append(r[1])
    r = sess.push({0: (c[0, :, 5:7].cuda(), True), 1: c[1, :, 2:6].cuda()}, post=chunked, post_output='float'); got['a'].append(r[0]); got['c'].append(r[1])
    sess.open(0, seed=42)
    r = sess.push({0: (c[1, :, :6].cuda(), True), 1: (c[1, :, 6:8].cuda(), True)}, post=chunked, post_output='float'); got['b'].append(r[0]); got['c'].append(r[1])
    torch.cuda.synchronize(); sess.check(); sess.close()
    for key, frames_k in (('a', 7), ('b', 6), ('c', 8)):
        smp = torch.cat([p[0] for p in got[key]]).cpu().numpy()
        y = torch.cat([p[1] for p in got[key]]).cpu().numpy()
        assert smp.shape[0] == frames_k * cfg.hop
        assert np.array_equal(PU.bits(y), PU.bits(PU.chain(PU.decode(it, smp), K)[0])), key
    # folded: the waveforms are decoded already
    raw_stage = model.output_stage(2, in_type='raw')
    wavs, posts = model.folded([c[0], c[1, :, :9]], rows=plan, check=True, post=raw_stage)
    torch.cuda.synchronize()
    for u, w in enumerate(wavs):
        my, mq, _ = PU.mirror_finish(0, w.cpu().numpy(), K)
        assert w.shape[0] == frames[u] * cfg.hop
        assert np.array_equal(PU.bits(posts[u][0].cpu().numpy()), PU.bits(my)) and np.array_equal(posts[u][1].cpu().numpy(), mq), u
    if it != 0:
        with pytest.raises(ValueError):
            model.folded([c[0]], rows=1, post=fin)
    for s in (fin, chunked, raw_stage):
        s.close()
    model.engine.close()


# ---- the driver
ROUTES = {'oneshot': '', 'slots': ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,input_type=mulaw-quantize,quantize_channels=256,out_channels=256',
          'fold': ',mi355_synthesis_fold_rows=4,mi355_synthesis_fold_warm=1,mi355_synthesis_fold_fade=1,mi355_synthesis_fold_min_frames=4'}


FRAMES_DRV = (40, 45, 50)      # 640 ... 800 samples: at the 0.5 % of samples that flip by one LSB on these noise-like outputs, 2 % is several standard deviations away


@pytest.mark.parametrize('route', ['oneshot', 'slots', 'fold'])
def test_driver_output_hparams(tmp_path, route):
    """Synthesizer.synthesize on each route: the default hparams write the files of a run whose hparams lack the new keys (no behaviour change);
    mi355_output_stage=device without de-emphasis writes the host path's bytes; with mi355_output_deemphasis the device's files are within 1 LSB of the
    host path's (audio.inv_preemphasis, float64) on at most 2 % of the samples -- and not the files without it.  Measured on an MI355X: 0 ... 5 of
    640 ... 800 samples differ by one (at most 0.63 %)."""
    import hparams as H
    from scipy.io import wavfile
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

    def run(tag, extra='', drop=False):
        hp = H._build(); hp.parse(base + extra)
        if drop:
            for key in ('mi355_output_deemphasis', 'mi355_output_stage', 'mi355_output_gain'):
                hp._keys.remove(key); object.__delattr__(hp, key)
        out = str(tmp_path / tag); os.makedirs(out)
        s = Synthesizer(); s.load(ckpt, hp)
        files = s.synthesize(mels, None, names, out, None)
        s.model.engine.close()
        for st in s._post_stages.values():
            st.close()
        assert [os.path.basename(f) for f in files] == ['wavenet-audio-%s.wav' % n for n in names]
        return [open(f, 'rb').read() for f in files], [wavfile.read(f)[1].astype(np.int32) for f in files]

    plain = run('plain')
    assert run('nokeys', drop=True)[0] == plain[0]
    assert run('device', ',mi355_output_stage=device')[0] == plain[0]
    host = run('host_de', ',mi355_output_deemphasis=True')
    dev = run('device_de', ',mi355_output_deemphasis=True,mi355_output_stage=device')
    for i, (h, d, p) in enumerate(zip(host[1], dev[1], plain[1])):
        assert h.shape == d.shape == (FRAMES_DRV[i] * 16,)
        diff = np.abs(h - d)
        print('%s utterance %d: %d of %d samples differ, max %d' % (route, i, int(np.sum(diff > 0)), diff.size, int(diff.max())))
        assert diff.max() <= 1 and np.mean(diff > 0) <= 0.02, i
        assert np.mean(h != p) > 0.5, i                                                  # de-emphasis really changed the file
