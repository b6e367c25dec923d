"""Sample-rate conversion on the device (csrc/wn_resample.hip), at the smallest shapes where the kernel can go wrong: eight small (L, M, Z) configurations and
the defaults at 48 000 -> 22 050 and 22 050 -> 8 000, each over a ragged batch (lengths 0, 1, W, 2 W + 1 and rows whose last output falls on the first, the
last and the one-past-last slot of an output block) with pitches larger than the rows and canaries beyond them.  wn_resample_run equals the host hook BIT FOR
BIT and lies inside the float32 bound of tests/resample_ref.py against float64; a row's bits do not depend on the call; wn_resample_push in every cutting
equals run of the whole row bit for bit, with a restarted row and rows left alone; n_out equals ready differences; nothing allocates after create; and
SynthesisStream / SlotSession with resample= and Synthesizer with mi355_output_sample_rate on a tiny model."""
import ctypes

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
SENTINEL = -7.25
SMALL = [(2, 3, 4), (3, 2, 4), (1, 2, 4), (2, 1, 4), (5, 7, 3), (7, 5, 3), (147, 320, 4), (320, 147, 4)]      # (L, M, Z): sr_out = L, sr_in = M


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _block(L, M, Z):
    """outputs per workgroup, as csrc/wn_resample.h plans them"""
    W = R.plan(M, L, Z)[2]
    b = 1024
    while b > 64 and (b - 1) * M // L + 2 + 2 * W > 12288:
        b //= 2
    return b


def _n_for_outputs(k, L, M):
    """the shortest row with k outputs"""
    n = (k - 1) * M // L
    while R.num_out(n, L, M) < k:
        n += 1
    return n


def _lengths(L, M, Z):
    W, blk = R.plan(M, L, Z)[2], _block(L, M, Z)
    return [0, 1, W, 2 * W + 1, _n_for_outputs(blk + 1, L, M), _n_for_outputs(blk, L, M), _n_for_outputs(2 * blk + 1, L, M), 3 * W + 7]


def _batch(lens, seed, pad=5):
    rng = np.random.default_rng(seed)
    x = np.full((len(lens), max(lens) + pad), np.nan, np.float32)      # NaN beyond every row: a sample read past lengths[b] would show
    for b, n in enumerate(lens):
        x[b, :n] = rng.standard_normal(n).astype(np.float32)
    return x


def _run(rs, x, lens, pad=7):
    out = torch.full((len(lens), max(1, rs.num_out(max(lens))) + pad), SENTINEL, device='cuda')
    _, n_out = rs.run(_dev(x), lens, out=out)
    torch.cuda.synchronize()
    for b, n in enumerate(lens):
        assert n_out[b] == R.num_out(n, rs.L, rs.M)
        assert bool(torch.all(out[b, n_out[b]:] == SENTINEL)), (b, n_out[b])      # the canaries beyond the row's outputs
    return out, n_out


def _check_config(sr_in, sr_out, Z, lens, seed):
    from wavenet_vocoder import _ext
    L, M, W, T = R.plan(sr_in, sr_out, Z)
    x = _batch(lens, seed)
    rs = _ext.Resampler(sr_in, sr_out, len(lens), max(max(lens), 1), zeros=Z)
    assert (rs.L, rs.M, rs.W) == (L, M, W)
    out, n_out = _run(rs, x, lens)
    got = out.cpu().numpy()
    host = _ext.resample_rows_host([x[b, :n] for b, n in enumerate(lens)], sr_in, sr_out, Z)
    worst = 0.0
    for b, n in enumerate(lens):
        assert np.array_equal(got[b, :n_out[b]].view(np.int32), host[b].view(np.int32)), (b, n)
        if n:
            ref, bs = R.polyphase(x[b, :n], sr_in, sr_out, Z, return_bound_sum=True)
            bound = R.bound32(bs, T)
            assert np.all(np.abs(got[b, :n_out[b]] - ref) <= bound), (b, n)
            worst = max(worst, float((np.abs(got[b, :n_out[b]] - ref) / np.maximum(bound, 1e-300)).max()))
    print('%d -> %d, Z = %d: worst error / bound %.3f' % (sr_in, sr_out, Z, worst))
    rs.close()
    return x, got, n_out


@pytest.mark.parametrize('L,M,Z', SMALL)
def test_run_equals_the_hook_and_is_inside_the_float32_bound(L, M, Z):
    _check_config(M, L, Z, _lengths(L, M, Z), 100 + L)


@pytest.mark.parametrize('sr_in,sr_out,n', [(48000, 22050, 4800), (22050, 8000, 2205)])
def test_defaults_at_the_production_rates(sr_in, sr_out, n):
    W = R.plan(sr_in, sr_out)[2]
    _check_config(sr_in, sr_out, R.ZEROS, [n, 0, 1, W, 2 * W + 1], 7)


def test_identity_copies_the_bits():
    from wavenet_vocoder import _ext
    x = _batch([9, 0, 1030], 3)
    x[0, 3] = -0.0
    rs = _ext.Resampler(22050, 22050, 3, 2000)
    out, n_out = _run(rs, x, [9, 0, 1030])
    assert n_out == [9, 0, 1030] and rs.W == 0
    for b, n in enumerate([9, 0, 1030]):
        assert torch.equal(_bits(out[b, :n]), _bits(_dev(x[b, :n])))
    rs.close()


def test_a_rows_bits_do_not_depend_on_the_call():
    from wavenet_vocoder import _ext
    L, M, Z = 5, 7, 3
    n = _n_for_outputs(1024 + 17, L, M)
    x = _batch([n], 11, pad=0)
    alone = _ext.Resampler(M, L, 1, n, zeros=Z)
    a, _ = _run(alone, x, [n], pad=0)
    lens = [40, n + 31, n, 3]
    xb = _batch(lens, 12, pad=13)
    xb[2, :n] = x[0]
    batch = _ext.Resampler(M, L, 4, n + 31, zeros=Z)
    b4, n_out = _run(batch, xb, lens, pad=2)
    assert torch.equal(_bits(b4[2, :n_out[2]]), _bits(a[0, :n_out[2]]))
    xb2 = _batch([n, 5], 13, pad=1)
    xb2[0, :n] = x[0]
    b2, _ = _run(batch, xb2, [n, 5], pad=0)
    assert torch.equal(_bits(b2[0, :n_out[2]]), _bits(a[0, :n_out[2]]))
    alone.close(); batch.close()


def _cuts(n, W, kind, seed=0):
    if kind == 'random':
        rng = np.random.default_rng(seed)
        c = []
        while sum(c) < n:
            c.append(int(rng.integers(0, 2 * W + 3)))
    else:
        c = [kind] * (n // max(kind, 1) + 1) if kind > 0 else [0, n]
    out, pos = [], 0
    for v in c:
        v = min(v, n - pos)
        out.append(v); pos += v
        if pos == n and kind != 0:
            break
    return out


def _push_all(rs, sched, x, pad=3):
    """sched: a list of (n [B], restart [B] or None, final [B] or None, offsets [B]); every push into a sentinel-filled output; returns per-row device tensors
    and the n_out of every push"""
    B = x.shape[0]
    parts, counts = [[] for _ in range(B)], []
    for n, rst, fin, off in sched:
        blk = np.full((B, max(max(n), 1) + 2), np.nan, np.float32)
        for b in range(B):
            blk[b, :n[b]] = x[b, off[b]:off[b] + n[b]]
        out = torch.full((B, rs.num_out(max(n) + 2 * rs.W) + pad), SENTINEL, device='cuda')
        _, n_out = rs.push(_dev(blk), n=n, restart=rst, final=fin, out=out)
        for b in range(B):
            assert bool(torch.all(out[b, n_out[b]:] == SENTINEL)), (b, n_out[b])
            parts[b].append(out[b, :n_out[b]])
        counts.append(n_out)
    torch.cuda.synchronize()
    return [torch.cat(p) for p in parts], counts


@pytest.mark.parametrize('L,M,Z', [(2, 3, 4), (3, 2, 4), (5, 7, 3), (147, 320, 4), (320, 147, 4)])
def test_push_in_every_cutting_equals_run_bit_for_bit(L, M, Z):
    """three rows cut differently in one call (row 0 by the cutting under test, row 1 at random, row 2 in one piece after being left alone), for the cuttings
    1, W - 1, W, W + 1, 0 and random; n_out equals the differences of ready()"""
    from wavenet_vocoder import _ext
    W = R.plan(M, L, Z)[2]
    n = 3 * W + 5 + (M * 9) // L
    lens = [n, n - 3, W + 2]
    x = _batch(lens, 21 + L, pad=0)
    whole = _ext.Resampler(M, L, 3, n, zeros=Z)
    ref, ref_n = _run(whole, np.nan_to_num(x), lens)
    rs = _ext.Resampler(M, L, 3, n, zeros=Z)
    for kind in (1, W - 1, W, W + 1, 0, 'random'):
        c0, c1 = _cuts(lens[0], W, kind, 1), _cuts(lens[1], W, 'random', 2)
        K = max(len(c0), len(c1)) + 1
        sched, off, S = [], [0, 0, 0], [0, 0, 0]
        for k in range(K):
            nn = [c0[k] if k < len(c0) else 0, c1[k] if k < len(c1) else 0, lens[2] if k == K - 1 else 0]
            fin = [int(k == len(c0) - 1), int(k == len(c1) - 1), int(k == K - 1)]
            sched.append((nn, [int(k == 0)] * 3, fin, list(off)))
            off = [off[b] + nn[b] for b in range(3)]
        rows, counts = _push_all(rs, sched, np.nan_to_num(x))
        for b in range(3):
            assert rows[b].shape[0] == ref_n[b] and torch.equal(_bits(rows[b]), _bits(ref[b, :ref_n[b]])), (kind, b)
        for k, (nn, _, fin, _) in enumerate(sched):      # n_out is the difference of ready(): a row left alone (n = 0, not final) emits nothing
            for b in range(3):
                if nn[b] == 0 and not fin[b]:
                    assert counts[k][b] == 0
                    continue
                assert counts[k][b] == rs.ready(S[b] + nn[b], fin[b]) - rs.ready(S[b]), (kind, k, b)
                S[b] += nn[b]
    whole.close(); rs.close()


def test_a_row_restarted_mid_session_and_an_ended_row():
    from wavenet_vocoder import _ext
    L, M, Z = 5, 7, 3
    W = R.plan(M, L, Z)[2]
    n1, n2 = 2 * W + 3, 4 * W + 1
    x = _batch([n1 + n2, n1 + n2], 31, pad=0)
    rs = _ext.Resampler(M, L, 2, W + 1, zeros=Z)
    c, pos, sched = W + 1, 0, []
    while pos < n1 + n2:      # row 0 is cut off at n1 without a final push and restarted there; row 1 runs on
        m = min(c, (n1 if pos < n1 else n1 + n2) - pos)
        sched.append(([m, m], [int(pos in (0, n1)), int(pos == 0)], [int(pos + m == n1 + n2)] * 2, [pos, pos]))
        pos += m
    k = next(i for i, s in enumerate(sched) if s[1][0] and i > 0)
    before, _ = _push_all(rs, sched[:k], x)
    after, _ = _push_all(rs, sched[k:], x)
    whole = _ext.Resampler(M, L, 2, n1 + n2, zeros=Z)
    second = np.zeros_like(x); second[0, :n2] = x[0, n1:]; second[1] = x[1]
    ref, ref_n = _run(whole, second, [n2, n1 + n2])
    assert before[0].shape[0] == rs.ready(n1)
    assert torch.equal(_bits(after[0]), _bits(ref[0, :ref_n[0]]))
    assert torch.equal(_bits(torch.cat([before[1], after[1]])), _bits(ref[1, :ref_n[1]]))
    with pytest.raises(_ext.WnError) as e:
        rs.push(_dev(x[:, :3]), n=[0, 3])      # row 1 has ended: without a restart it is refused, and no row changes
    assert e.value.code == -5
    again, _ = _push_all(rs, [([0, 3], [0, 1], [0, 1], [0, 0])], x)
    one, one_n = _run(whole, x[1:2, :3], [3])
    assert torch.equal(_bits(again[1]), _bits(one[0, :one_n[0]]))
    rs.close(); whole.close()


def test_calls_allocate_nothing():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    rs = _ext.Resampler(7, 5, 3, 64, zeros=3)
    x = _dev(np.zeros((3, 64), np.float32))
    out = torch.zeros(3, 80, device='cuda')
    rs.push(x, restart=True, out=out)
    a, b = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    assert lib.wn_test_device_resources(a) == 0
    for k in range(6):
        rs.push(x, n=[64, 7 * (k % 2), 0], final=[0, 0, int(k == 5)], restart=[0, 0, int(k == 4)], out=out)
        rs.run(x, [64, 3, 0], out=out)
    torch.cuda.synchronize()
    assert lib.wn_test_device_resources(b) == 0
    assert list(a) == list(b)                      # no buffer, stream, event or graph came or went; no allocation was made
    rs.close()
    assert lib.wn_test_device_resources(b) == 0 and b[0] == a[0] - 2 and b[4] == a[4]      # the handle's two buffers are released with it


# ---- end to end on a tiny model
TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_output_denoise_fft=64,mi355_output_denoise_hop=16,mi355_output_denoise=0.5,preemphasize=True')


def _tiny(B):
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    hp = H._build(); hp.parse(TINY)
    model = WaveNet(hp)
    model.build(B, 16 * 16)
    return model, hp


def _whole(model, rate, y):
    """Resampler.run on one row of float32 samples, and its int16 cast by a raw stage at the model's gain"""
    rs = model.output_resampler(1, int(y.shape[0]), rate)
    z, n_out = rs.run(y.reshape(1, -1).contiguous())
    q = rs.tail.push(z, n=n_out, restart=True)
    torch.cuda.synchronize()
    rs.close()
    return z[0, :n_out[0]], q[0, :n_out[0]]


@pytest.mark.parametrize('with_denoise', [False, True])
def test_stream_with_resample_equals_run_on_the_concatenated_chunks(with_denoise):
    import denoise_ref as D
    model, hp = _tiny(2)
    rs = model.output_resampler(2, 16 * 16 + 64, 8000)
    rng = np.random.RandomState(6)
    c = torch.from_numpy(rng.uniform(0, 1, size=(2, 16, 14)).astype(np.float32)).cuda()
    kw = {}
    if with_denoise:
        kw['denoise'] = model.stream_denoiser(2, 16 * 16)
        kw['denoise'].set_profile(0.05 * D.noise_profile(64, 16))
    post = model.output_stage(2, in_type='raw') if with_denoise else model.output_stage(2)

    def run(**more):
        model._synth_calls = 0
        st = model.stream(2)
        return [st.push(c[:, :, a:b], final=(b == 14), post=post, **kw, **more) for a, b in ((0, 5), (5, 6), (6, 14))]
    flt = run(post_output='float')                               # the float chunks at the model rate
    got = run(post_output='both', resample=rs)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p[0] for p in got], 1), torch.cat([p[0] for p in flt], 1))      # the generated samples do not know about it
    y = torch.cat([p[1] for p in flt], 1)
    assert y.shape[1] == 224
    given = np.cumsum([p[1].shape[1] for p in flt])
    assert [p[1][1].shape[1] for p in got] == [rs.ready(given[0]), rs.ready(given[1]) - rs.ready(given[0]), rs.num_out(224) - rs.ready(given[1])]
    for b in range(2):
        z, q = _whole(model, 8000, y[b])
        assert z.shape[0] == rs.num_out(224) and float(z.abs().max()) > 0
        assert torch.equal(_bits(torch.cat([p[1][1][b] for p in got])), _bits(z)), b
        assert torch.equal(torch.cat([p[1][0][b] for p in got]), q), b
    for h in [rs, post] + list(kw.values()):
        h.close()
    model.engine.close()


def test_three_slots_with_resample_equal_run_on_the_concatenated_chunks():
    model, hp = _tiny(3)
    rs = model.output_resampler(3, 16 * 16, 48000)
    post = model.output_stage(3)
    rng = np.random.RandomState(8)
    c = torch.from_numpy(rng.uniform(0, 1, size=(3, 16, 14)).astype(np.float32)).cuda()

    def run(**kw):
        sess = model.slots(3)
        got = {'a': [], 'b': [], 'c': []}
        sess.open(0, seed=41); sess.open(2, seed=43)
        r = sess.push({0: c[0, :, :5], 2: c[1, :, :2]}, post=post, **kw); got['a'].append(r[0]); got['c'].append(r[2])
        r = sess.push({0: (c[0, :, 5:7], True), 2: c[1, :, 2:9]}, post=post, **kw); got['a'].append(r[0]); got['c'].append(r[2])
        sess.open(0, seed=42)                                    # slot 0 is opened anew: its rows in post and in the resampler start afresh
        r = sess.push({0: (c[2, :, :9], True), 2: (c[1, :, 9:14], True)}, post=post, **kw); got['b'].append(r[0]); got['c'].append(r[2])
        torch.cuda.synchronize(); sess.check(); sess.close()
        return got
    flt = run(post_output='float')
    got = run(post_output='float', resample=rs)
    for key, frames in (('a', 7), ('b', 9), ('c', 14)):
        assert torch.equal(torch.cat([p[0] for p in got[key]]), torch.cat([p[0] for p in flt[key]]))
        y = torch.cat([p[1] for p in flt[key]])
        z, _ = _whole(model, 48000, y)
        assert y.shape[0] == frames * 16 and z.shape[0] == rs.num_out(frames * 16)
        assert torch.equal(_bits(torch.cat([p[1] for p in got[key]])), _bits(z)), key
    rs.close(); post.close()
    model.engine.close()


@pytest.mark.parametrize('route', ['oneshot', 'slots'])
def test_synthesizer_writes_at_the_output_rate(tmp_path, route):
    """Synthesizer.synthesize: with mi355_output_sample_rate = 0, or without the new keys, the files are those of the default hparams byte for byte; at 8000 the
    'host' and the 'device' output stage both write 8 kHz files of ceil(n 160 / 441) samples whose PCM differs by at most 1 LSB (the de-emphasis in front is
    float64 on one side and float32 on the other), and which are not the model-rate files cut short."""
    import os
    import hparams as H
    from scipy.io import wavfile
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesizer import Synthesizer
    frames = (40, 45, 50)
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],wavenet_synthesis_batch_size=4')
    if route == 'slots':
        base += ',mi355_synthesis_slots=2,mi355_synthesis_chunk_frames=3,input_type=mulaw-quantize,quantize_channels=256,out_channels=256'
    rng = np.random.RandomState(5)
    mels = [rng.uniform(-4, 4, size=(f, 16)).astype(np.float32) for f in frames]
    names = ['u%d' % i for i in range(3)]
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(4, max(frames) * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()

    def run(tag, extra='', drop=False):
        hp = H._build(); hp.parse(base + extra)
        if drop:
            for key in ('mi355_output_sample_rate', 'mi355_resample_input'):
                hp._keys.remove(key); object.__delattr__(hp, key)
        out = str(tmp_path / tag); os.makedirs(out)
        s = Synthesizer(); s.load(ckpt, hp)
        files = s.synthesize(mels, None, names, out, None)
        s.model.engine.close()
        for st in list(s._post_stages.values()) + [h for h in [getattr(s, '_resampler', None)] if h is not None]:
            st.close()
        assert (getattr(s, '_resampler', None) is not None) == ('=8000' in extra and 'device' in extra)      # at 0 no handle exists
        return [open(f, 'rb').read() for f in files], [wavfile.read(f) for f in files]

    plain = run('plain')
    assert run('nokeys', drop=True)[0] == plain[0]
    assert run('zero', ',mi355_output_sample_rate=0,mi355_output_stage=device')[0] == plain[0]
    host = run('host8k', ',mi355_output_deemphasis=True,mi355_output_sample_rate=8000')
    dev = run('dev8k', ',mi355_output_deemphasis=True,mi355_output_sample_rate=8000,mi355_output_stage=device')
    for i, ((hr, h), (dr, d), (pr, p)) in enumerate(zip(host[1], dev[1], plain[1])):
        n = frames[i] * 16
        assert hr == dr == 8000 and pr == 22050 and p.shape == (n,)
        assert h.shape == d.shape == (-(-n * 160 // 441),)
        diff = np.abs(h.astype(np.int32) - d.astype(np.int32))
        print('%s utterance %d: %d of %d samples differ, max %d' % (route, i, int(np.sum(diff > 0)), diff.size, int(diff.max())))
        assert diff.max() <= 1, i
        # peak-normalised AFTER the conversion (the float32 product peak x (32767 / peak) may land just below 32767 and is truncated); another signal
        assert int(np.abs(h.astype(np.int32)).max()) >= 32766 and np.mean(h != p[:h.shape[0]]) > 0.5, i
