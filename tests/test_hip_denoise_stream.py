"""Streaming denoiser on the device (csrc/wn_denoise_stream.hip): a row pushed through wn_denoise_stream_push in any cutting equals wn_denoise_run of the whole
decoded row BIT FOR BIT (torch.equal on the int32 view) -- geometries (64, 16) and (96, 20) with 3 ragged rows over the cuttings of
tests/denoise_stream_ref.py, one case at (1024, 256), 65 rows (beyond one launch group), a row restarted mid-session; a row's bits do not depend on B, its
index, the pitches or its neighbours' cutting; in_type 1 / 2 decode as the output stage does; the streamed output against float64 under the rule of
tests/denoise_ref.py; SynthesisStream / SlotSession (narrow, and wide with 33 slots) with post= and denoise= on a tiny model against OutputDenoiser.apply
followed by the same OutputStage chain; and pushes allocate nothing."""
import ctypes

import numpy as np
import pytest
import torch

import denoise_ref as R
import denoise_stream_ref as S

pytestmark = pytest.mark.gpu
SENTINEL = -7.25


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stream(name, rows, max_push, in_type=0):
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    ds = _ext.DenoiseStream(n_fft, hop, rows, max_push, in_type)
    ds.set_profile(R.noise_profile(n_fft, hop))
    return ds


def _one_shot(name, dec, lens, strength):
    """wn_denoise_run on the decoded rows (device tensor [B, pitch]) -> device tensor"""
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES[name]
    d = _ext.SpectralDenoiser(n_fft, hop, len(lens), max(max(lens), 1))
    d.profile = R.noise_profile(n_fft, hop)
    out = d.apply(dec, lens, strength)
    torch.cuda.synchronize()
    d.close()
    return out


def _run(ds, pushes, strength, pad=3):
    """every push into a sentinel-filled output of its own pitch; asserts that nothing beyond n_out[b] is written; returns one device tensor per row"""
    B = len(pushes[0][1])
    parts = [[] for _ in range(B)]
    for blk, n, rs, fin in pushes:
        out = torch.full((B, max(n) + ds.n_fft + pad), SENTINEL, device='cuda')
        _, n_out = ds.push(_dev(blk), n=n, restart=rs, final=fin, strength=strength, out=out)
        for b in range(B):
            assert n_out[b] == 0 or not bool(torch.any(out[b, :n_out[b]] == SENTINEL))
            assert bool(torch.all(out[b, n_out[b]:] == SENTINEL)), (b, n_out[b])
            parts[b].append(out[b, :n_out[b]])
    torch.cuda.synchronize()
    return [torch.cat(p) for p in parts]


def _assert_rows(rows, ref, lens):
    for b, n in enumerate(lens):
        assert rows[b].shape[0] == n and torch.equal(_bits(rows[b]), _bits(ref[b, :n])), b


def _lens(name, cut):
    n_fft, hop = R.GEOMETRIES[name]
    return [4 * n_fft, 17, n_fft // 2 - 1] if cut == 'one' else [64 * hop + 1, 17, 32 * hop + 1]      # (single-sample pushes: short rows keep the test short)


@pytest.mark.parametrize('cut', S.CUTTINGS)
@pytest.mark.parametrize('name', ['A', 'B'])
def test_streamed_equals_run_bit_for_bit(name, cut):
    n_fft, hop = R.GEOMETRIES[name]
    lens = _lens(name, cut)
    ds = _stream(name, 3, max(lens))
    for kind, strength in (('tone', 1.0), ('above', 4.0), ('straddle', 0.0)):
        wav = R.batch(kind, lens, 400, n_fft)      # NaN beyond every row: a sample read past n[b] would show
        ref = _one_shot(name, _dev(np.nan_to_num(wav)), lens, strength)
        rows = _run(ds, S.blocks(wav, S.schedule(lens, cut, n_fft, hop)), strength)
        _assert_rows(rows, ref, lens)
    ds.close()


def test_production_geometry_in_pushes_of_2200():
    n_fft, hop = R.GEOMETRIES['P']
    lens = [3000, 2201, 700]
    ds = _stream('P', 3, 2200)
    wav = R.batch('tone', lens, 7, n_fft)
    ref = _one_shot('P', _dev(np.nan_to_num(wav)), lens, 1.0)
    rows = _run(ds, S.blocks(wav, S.schedule(lens, 2200, n_fft, hop)), 1.0)
    _assert_rows(rows, ref, lens)
    assert ds.ready(2200) == 1280 and ds.ready(2201, True) == 2201
    ds.close()


def test_65_rows_beyond_one_launch_group():
    n_fft, hop = R.GEOMETRIES['A']
    B = 65
    lens = [(37 * b) % 300 for b in range(B)]
    lens[64] = 299
    ds = _stream('A', B, 3 * hop + 2)
    wav = R.batch('straddle', lens, 3, n_fft)
    ref = _one_shot('A', _dev(np.nan_to_num(wav)), lens, 0.5)
    rows = _run(ds, S.blocks(wav, S.schedule(lens, 'ragged', n_fft, hop)), 0.5)
    _assert_rows(rows, ref, lens)
    ds.close()


@pytest.mark.parametrize('name', ['A', 'B'])
def test_a_row_restarted_mid_session(name):
    """row 0 is cut off mid-utterance (no final) and restarted with another signal while row 1 runs on: row 0's output from the restart on is the one-shot
    run of the second signal alone, row 1 is untouched by it; then row 1, ended, is restarted too"""
    n_fft, hop = R.GEOMETRIES[name]
    c, n1, n2 = hop + 1, 7 * hop + 5, 30 * hop + 3
    first, second, other = R.signal('above', n1, 1, n_fft), R.signal('tone', n2, 2, n_fft), R.signal('straddle', n1 + n2, 3, n_fft)
    ds = _stream(name, 2, c)
    seq0 = np.concatenate([first, second])
    pushes, pos = [], 0
    while pos < n1 + n2:
        m = min(c, (n1 if pos < n1 else n1 + n2) - pos)
        blk = np.full((2, c), np.nan, np.float32)
        blk[0, :m], blk[1, :m] = seq0[pos:pos + m], other[pos:pos + m]
        pushes.append((blk, [m, m], [int(pos == 0 or pos == n1), int(pos == 0)], [int(pos + m == n1 + n2)] * 2))
        pos += m
    k = next(i for i, p in enumerate(pushes) if p[2][0] and i > 0)
    before = _run(ds, pushes[:k], 1.0)
    after = _run(ds, pushes[k:], 1.0)
    ref2 = _one_shot(name, _dev(second[None]), [n2], 1.0)
    ref_other = _one_shot(name, _dev(other[None]), [n1 + n2], 1.0)
    assert before[0].shape[0] == ds.ready(n1)
    _assert_rows([after[0]], ref2, [n2])
    _assert_rows([torch.cat([before[1], after[1]])], ref_other, [n1 + n2])
    blk = np.full((2, c), np.nan, np.float32); blk[1, :c] = second[:c]
    again = _run(ds, [(blk, [0, c], [0, 1], [0, 1])], 1.0)      # row 1 ended above: a restart opens it again
    _assert_rows([again[1]], _one_shot(name, _dev(second[None, :c]), [c], 1.0), [c])
    from wavenet_vocoder import _ext
    with pytest.raises(_ext.WnError) as e:
        ds.push(_dev(blk), n=[0, c])                              # ... and without one it is refused
    assert e.value.code == -5
    ds.close()


def test_a_rows_bits_do_not_depend_on_the_call():
    """a row alone in a handle of one row, in pushes of hop + 1, against the same row at index 2 of a batch of 3 with other pitches whose neighbours are cut
    raggedly and end earlier or later"""
    n_fft, hop = R.GEOMETRIES['B']
    n = 40 * hop + 3
    x = R.signal('tone', n, 9, n_fft)
    alone = _stream('B', 1, hop + 1)
    a = _run(alone, S.blocks(x[None], S.schedule([n], 'hop+1', n_fft, hop)), 1.0, pad=0)[0]
    lens = [n + 70, 3 * hop, n]
    wav = R.batch('straddle', lens, 5, n_fft)
    wav[2, :n] = x
    nb, mine = S.schedule(lens[:2], 'ragged', n_fft, hop), S.schedule([n], 'hop+1', n_fft, hop)
    at = lambda s, k, w: s[k] if k < len(s) else ([0] * w, [0] * w)      # (a row that has ended is given nothing and left alone)
    sched = [(at(nb, k, 2)[0] + at(mine, k, 1)[0], at(nb, k, 2)[1] + at(mine, k, 1)[1]) for k in range(max(len(nb), len(mine)))]
    batch = _stream('B', 3, 3 * hop + 2)
    rows = _run(batch, S.blocks(wav, sched), 1.0, pad=11)
    assert torch.equal(_bits(rows[2]), _bits(a))
    _assert_rows([a], _one_shot('B', _dev(x[None]), [n], 1.0), [n])
    alone.close(); batch.close()


@pytest.mark.parametrize('in_type', [1, 2])
def test_in_type_decodes_as_the_output_stage_does(in_type):
    """mu-law floats / class ids pushed as they are == the rows decoded first (an OutputStage without de-emphasis: y has the bits of the decoded x) and run whole"""
    import hparams as H
    from wavenet_vocoder import _ext
    n_fft, hop = R.GEOMETRIES['A']
    rs = np.random.RandomState(4)
    lens = [20 * hop + 5, 33]
    x = rs.randint(0, 256, (2, lens[0])).astype(np.int32) if in_type == 2 else rs.uniform(-1, 1, (2, lens[0])).astype(np.float32)
    stage = _ext.OutputStage(H._build(), 2, deemphasis=0.0, in_type=in_type)
    dec = stage.push(_dev(x), n=lens, restart=True, pcm=False, float_out=True)
    ref = _one_shot('A', dec, lens, 1.0)
    ds = _stream('A', 2, hop + 1, in_type)
    rows = _run(ds, S.blocks(x, S.schedule(lens, 'hop+1', n_fft, hop)), 1.0)
    _assert_rows(rows, ref, lens)
    ds.close(); stage.close()


def test_streamed_output_against_float64():
    n_fft, hop = R.GEOMETRIES['B']
    lens = [64 * hop + 1, 17, 32 * hop + 1]
    prof = R.noise_profile(n_fft, hop)
    ds = _stream('B', 3, 3 * hop + 2)
    wav = R.batch('tone', lens, 8, n_fft)
    rows = _run(ds, S.blocks(wav, S.schedule(lens, 'ragged', n_fft, hop)), 1.0)
    got = np.full(wav.shape, np.nan, np.float32)
    for b, r in enumerate(rows):
        got[b, :lens[b]] = r.cpu().numpy()
    w, _ = R.check_rows(got, wav, lens, prof, 1.0, n_fft, hop)
    print('streamed B tone: worst error / bound %.3f' % w)
    assert w <= 1.0
    ds.close()


def test_pushes_allocate_nothing():
    from wavenet_vocoder import _ext
    lib = _ext.load_library()
    n_fft, hop = R.GEOMETRIES['A']
    ds = _stream('A', 3, 40)
    x = _dev(np.zeros((3, 40), np.float32))
    out = torch.zeros(3, 40 + n_fft, device='cuda')
    ds.push(x, restart=True, strength=1.0, out=out)
    a, b = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    assert lib.wn_test_device_resources(a) == 0
    for k in range(6):
        ds.push(x, n=[40, 7 * (k % 2), 0], final=[0, 0, int(k == 5)], restart=[0, 0, int(k == 4)], strength=1.0, out=out)
    ds.set_profile(R.noise_profile(n_fft, hop))
    torch.cuda.synchronize()
    assert lib.wn_test_device_resources(b) == 0
    assert list(a) == list(b)                      # no buffer, stream, event or graph came or went; no allocation was made
    ds.close()
    assert lib.wn_test_device_resources(b) == 0 and b[0] == a[0] - 7 and b[4] == a[4]      # the handle's seven buffers are released with it


# ---- end to end on a tiny model
TINY = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
        'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_output_denoise_fft=64,mi355_output_denoise_hop=16,mi355_output_denoise=0.5')
HEADS = {'raw': '', 'mulaw-quantize': ',input_type=mulaw-quantize,quantize_channels=256,out_channels=256'}


def _chain_reference(model, den, samples, strength):
    """one utterance's model-domain samples -> decoded (the output stage's decode, no filter), OutputDenoiser.apply, then the model's raw output stage from
    y[-1] = 0: the float chunk a whole-utterance run would play"""
    n = int(samples.shape[0])
    dec_stage = model.output_stage(1, deemphasis=0.0)
    dec = dec_stage.push(samples.reshape(1, -1).contiguous(), restart=True, pcm=False, float_out=True)
    y = den.apply(dec, [n], strength)
    raw = model.output_stage(1, in_type='raw')
    res = raw.push(y, restart=True, pcm=False, float_out=True)[0]
    torch.cuda.synchronize()
    dec_stage.close(); raw.close()
    return res


@pytest.mark.parametrize('route,head', [('stream', 'mulaw-quantize'), ('slots', 'mulaw-quantize'), ('slots', 'raw'), ('wide_slots', 'raw')])
def test_routes_with_post_and_denoise_equal_the_whole_utterance_chain(route, head):
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    hp = H._build(); hp.parse(TINY + HEADS[head])
    B = 33 if route == 'wide_slots' else 2
    model = WaveNet(hp)
    model.build(B, 16 * 16)
    den = model.denoiser(1, 16 * 16)
    den.profile = 0.05 * R.noise_profile(64, 16)
    ds = model.stream_denoiser(B, 16 * 16, source=den)      # the profile travels device to device
    post = model.output_stage(B, in_type='raw')
    rs = np.random.RandomState(6)
    c = torch.from_numpy(rs.uniform(0, 1, size=(3, 16, 14)).astype(np.float32)).cuda()
    if route == 'stream':
        def run(**kw):
            model._synth_calls = 0
            st = model.stream(2)
            return [st.push(c[:2, :, a:b], final=(b == 14), **kw) for a, b in ((0, 5), (5, 6), (6, 14))]
        plain = run()
        parts = run(post=post, post_output='float', denoise=ds)
        torch.cuda.synchronize()
        smp = torch.cat([p[0] for p in parts], 1)
        assert torch.equal(smp, torch.cat(plain, 1))                                      # the generated samples do not know about the denoiser
        chunks = torch.cat([p[1] for p in parts], 1)
        given = np.cumsum([p[0].shape[1] for p in parts])
        assert given[-1] == 224 and [p[1].shape[1] for p in parts] == [ds.ready(given[0]), ds.ready(given[1]) - ds.ready(given[0]), 224 - ds.ready(given[1])]
        for b in range(2):
            assert torch.equal(_bits(chunks[b]), _bits(_chain_reference(model, den, smp[b], 0.5))), b
            assert float(chunks[b].abs().max()) > 0 and not torch.equal(chunks[b], _chain_reference(model, den, smp[b], 0.0))      # the denoiser did act, and left something
        with pytest.raises(ValueError):
            model.stream(2).push(c[:2, :, :3], post=model.output_stage(2), denoise=ds)      # a stage that would decode again is refused before anything runs
    else:
        hi = B - 1

        def run(**kw):
            sess = getattr(model, route)(B, steps_per_graph=24) if route == 'wide_slots' else model.slots(B)
            got = {'a': [], 'b': [], 'c': []}
            sess.open(0, seed=41); sess.open(hi, seed=43)
            r = sess.push({0: c[0, :, :5], hi: c[1, :, :2]}, **kw); got['a'].append(r[0]); got['c'].append(r[hi])
            r = sess.push({0: (c[0, :, 5:7], True), hi: c[1, :, 2:9]}, **kw); got['a'].append(r[0]); got['c'].append(r[hi])
            sess.open(0, seed=42)                                                         # slot 0 is opened anew: its rows in ds and post start afresh
            r = sess.push({0: (c[2, :, :9], True), hi: (c[1, :, 9:14], True)}, **kw); got['b'].append(r[0]); got['c'].append(r[hi])
            torch.cuda.synchronize(); sess.check(); sess.close()
            return got
        plain = run()
        got = run(post=post, post_output='float', denoise=ds, denoise_strength=0.25)
        for key, frames in (('a', 7), ('b', 9), ('c', 14)):
            smp = torch.cat([p[0] for p in got[key]])
            assert smp.shape[0] == frames * 16 and torch.equal(smp, torch.cat(plain[key]))
            y = torch.cat([p[1] for p in got[key]])
            assert torch.equal(_bits(y), _bits(_chain_reference(model, den, smp, 0.25))), key
            assert float(y.abs().max()) > 0 and not torch.equal(y, _chain_reference(model, den, smp, 0.0)), key      # the denoiser did act, and left something
    for h in (ds, post, den):
        h.close()
    model.engine.close()
