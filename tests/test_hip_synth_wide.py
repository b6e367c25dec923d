"""Wide synthesis (wn_synthesize_wide): more than 32 utterances in one launch-per-layer run.

The step kernels of csrc/wn_synth.hip take a tile of 32 streams per blockIdx.y; a stream's arithmetic is the one of the <= 32 run, so
  1. every tile of a wide run equals synthesize(steps_per_graph > 0) of its streams bit for bit (samples and raw outputs),
  2. device noise / the temperature pair are those of the full B,
  3. every element of a teacher-forced run sits within F = 4 x the storage-rounding yardstick of the float64 reference (tests/synth_ref.py),
  4. the wide owner shares nothing with the <= 32 owner but the context, 5. an inference-only context may hold more than 32 streams,
  6. the driver (Synthesizer.synthesize with mi355_synthesis_wide_rows) writes what WaveNet.wide returns.
Models: synth_ref.MODELS on hip_util.SMALL (hop 16, R = 64).  T = 256: the d = 32 ring of s6 has 128 slots, steps 128 ... 192 read wrapped
rows; steps_per_graph = 24: 10 replays + 16 single steps.  With WN_PARITY_REPORT_DIR set, case 3 writes wide_parity.json."""
import json
import os

import numpy as np
import pytest
import torch

import synth_ref as SR
from hip_util import upload_params
from test_hip_synth import _noise

pytestmark = pytest.mark.gpu

T = 256
SPG = 24
WN_E_SHAPE, WN_E_UNSUPPORTED, WN_E_STATE = -2, -4, -5
_CASE = {}
PARITY = {}


def _case(model, B, T_=T):
    if (model, B, T_) not in _CASE:
        _CASE[(model, B, T_)] = SR.make_case(model, B, T_)
    return _CASE[(model, B, T_)]


def _engine(model, B, T_=T, extra=None, **kw):
    from wavenet_vocoder import _ext
    hp, cfg, params, ti, wav, c, g = _case(model, B, T_)
    if extra:
        hp = SR.make_case(model, 1, T_, extra)[0]
    eng = _ext.Engine(hp, kw.pop('max_batch', B), T_, **kw)
    eng.pack_weights(upload_params(eng, params))
    return eng, cfg


def _bufs(cfg, B, T_=T):
    return (torch.empty(B, T_, dtype=torch.float32 if cfg.scalar_input else torch.int32, device='cuda'),
            torch.empty(B, cfg.out_channels, T_, device='cuda'))


def _wide(eng, cfg, c, g, noise, ti=None, seed=0, spg=SPG):
    B = c.shape[0]
    if g is not None:
        eng.set_global_condition(g.cuda())
    out, raw = _bufs(cfg, B, c.shape[-1] * cfg.hop)
    eng.synthesize_wide(c.contiguous().cuda(), None if noise is None else noise.contiguous().cuda(), out, raw, None if ti is None else ti.contiguous().cuda(),
                        steps_per_graph=spg, seed=seed)
    torch.cuda.synchronize()
    eng.synth_check()
    assert eng.synth_path == 'graph'
    return out.cpu(), raw.cpu()


def _narrow(eng, cfg, c, g, noise, spg=SPG):
    B = c.shape[0]
    if g is not None:
        eng.set_global_condition(g.cuda())
    out, raw = _bufs(cfg, B, c.shape[-1] * cfg.hop)
    eng.synthesize(c.contiguous().cuda(), noise.contiguous().cuda(), out, raw, None, steps_per_graph=spg)
    torch.cuda.synchronize()
    eng.synth_check()
    return out.cpu(), raw.cpu()


# ---- 1. row identity with the runs of <= 32 streams --------------------------------------------------------------------------------------
@pytest.mark.parametrize('model,B', [('s6', 33), ('s6', 64), ('s6', 70), ('s6_gauss', 70), ('s6_softmax', 70), ('s6_gin', 70), ('s6_gin_raw_1d', 70)])
def test_every_tile_equals_the_run_of_its_streams(model, B):
    hp, cfg, params, ti, wav, c, g = _case(model, B)
    eng, _ = _engine(model, B)
    nz = _noise(cfg, T, B, seed=4)[0]
    out, raw = _wide(eng, cfg, c, g, nz)
    assert torch.isfinite(raw).all()
    for k in range((B + 31) // 32):
        sl = slice(32 * k, min(32 * k + 32, B))
        o, r = _narrow(eng, cfg, c[sl], None if g is None else g[sl], nz[:, sl])
        assert torch.equal(out[sl], o), 'samples of tile %d differ from the run of its %d streams' % (k, sl.stop - sl.start)
        assert torch.equal(raw[sl], r), 'raw outputs of tile %d differ from the run of its %d streams' % (k, sl.stop - sl.start)
    eng.close()


def test_up_to_32_streams_is_the_launch_per_layer_run():
    B = 8
    hp, cfg, params, ti, wav, c, g = _case('s6', B)
    eng, _ = _engine('s6', B)
    nz = _noise(cfg, T, B, seed=4)[0]
    out, raw = _wide(eng, cfg, c, g, nz)
    o, r = _narrow(eng, cfg, c, g, nz)
    assert torch.equal(out, o) and torch.equal(raw, r)
    eng.close()


# ---- 2. noise ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['s6', 's6_gauss'])
def test_device_noise_and_temperature_are_those_of_the_full_batch(model):
    B, seed = 70, 1234
    hp, cfg, params, ti, wav, c, g = _case(model, B)
    eng, _ = _engine(model, B)
    nz = eng.fill_noise(torch.empty(T, B, eng.noise_per_step, device='cuda'), B, T, seed)
    a = _wide(eng, cfg, c, g, None, seed=seed)
    b = _wide(eng, cfg, c, g, nz)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    tempered = eng.temper_noise(nz, 0.7, 0.85)
    ref = _wide(eng, cfg, c, g, tempered)
    eng.set_temperature(0.7, 0.85)
    hot = _wide(eng, cfg, c, g, None, seed=seed)
    hot2 = _wide(eng, cfg, c, g, nz)
    eng.set_temperature(1.0, 1.0)
    assert torch.equal(hot[0], ref[0]) and torch.equal(hot[1], ref[1])
    assert torch.equal(hot2[0], ref[0]) and torch.equal(hot2[1], ref[1])
    assert not torch.equal(ref[0], a[0])
    eng.close()


# ---- 3. every step against float64 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('model', ['s6', 's8x2', 's6_softmax'])
def test_teacher_forced_every_step_against_float64(model):
    """|dev - ref| <= 4 Y[o] for every element of raw [70, O, 256]; Y: the bf16 storage-rounding yardstick of synth_ref (check_steps)."""
    B = 70
    hp, cfg, params, ti, wav, c, g = _case(model, B)
    eng, _ = _engine(model, B)
    nz = _noise(cfg, T, B, seed=0)[0]
    out, raw = _wide(eng, cfg, c, g, nz, ti=ti)
    eng.close()
    with torch.no_grad():
        ref = SR.synth_ref(params, cfg, ti, c, g)
        emul = SR.synth_ref(params, cfg, ti, c, g, store='bf16', path='launch')
    rec = SR.check_steps(raw, ref, emul, SR.FACTOR['bf16'], cfg, 'launch', what='wide-%s' % model)
    print('\nwide-%s: worst err / Y = %.2f (F = %g) at stream %d step %d channel %d' % (model, rec['worst_ratio'], rec['factor'], rec['stream'], rec['step'], rec['channel']))
    PARITY[model] = dict(rec, B=B, T=T, steps_per_graph=SPG)
    d = os.environ.get('WN_PARITY_REPORT_DIR')
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, 'wide_parity.json'), 'w') as f:
            json.dump({'factor': SR.FACTOR['bf16'], 'floor': SR.FLOOR, 'worst_ratio_per_case': {k: v['worst_ratio'] for k, v in PARITY.items()}, 'cases': PARITY}, f, indent=1)


# ---- 4. state ----------------------------------------------------------------------------------------------------------------------------
def test_wide_and_narrow_runs_leave_one_another_alone():
    B = 70
    hp, cfg, params, ti, wav, c, g = _case('s6', B)
    eng, _ = _engine('s6', B)
    nz = _noise(cfg, T, B, seed=4)[0]
    w0 = _wide(eng, cfg, c, g, nz)
    w1 = _wide(eng, cfg, c, g, nz)
    assert torch.equal(w0[0], w1[0]) and torch.equal(w0[1], w1[1])
    n_graph = _narrow(eng, cfg, c[:8], None, nz[:, :8])
    n_pipe = _narrow(eng, cfg, c[:8], None, nz[:, :8], spg=0)
    w2 = _wide(eng, cfg, c, g, nz)
    assert torch.equal(w0[0], w2[0]) and torch.equal(w0[1], w2[1])
    assert torch.equal(w0[0][:8], n_graph[0]) and torch.equal(w0[1][:8], n_graph[1])
    n_graph2 = _narrow(eng, cfg, c[:8], None, nz[:, :8])
    n_pipe2 = _narrow(eng, cfg, c[:8], None, nz[:, :8], spg=0)
    assert torch.equal(n_graph[0], n_graph2[0]) and torch.equal(n_graph[1], n_graph2[1])
    assert torch.equal(n_pipe[0], n_pipe2[0]) and torch.equal(n_pipe[1], n_pipe2[1])
    eng.close()


def test_wide_run_ends_an_open_stream_and_checks_its_shapes():
    from wavenet_vocoder import _ext
    B = 70
    hp, cfg, params, ti, wav, c, g = _case('s6', B)
    eng, _ = _engine('s6', B)
    nz = _noise(cfg, T, B, seed=4)[0]
    eng.stream_begin(2, seed=1, steps_per_graph=SPG)
    _wide(eng, cfg, c, g, nz)
    with pytest.raises(_ext.WnError) as e:
        eng.stream_push(c[:2, :, :4].contiguous().cuda(), torch.empty(2, 64, device='cuda'), final=True)
    assert e.value.code == WN_E_STATE
    out, raw = _bufs(cfg, B + 1)
    with pytest.raises(_ext.WnError) as e:      # B > max_batch
        eng.synthesize_wide(torch.zeros(B + 1, cfg.cin_channels, T // cfg.hop, device='cuda'), None, out, raw, None, steps_per_graph=SPG)
    assert e.value.code == WN_E_SHAPE
    out, raw = _bufs(cfg, B, T + cfg.hop)
    with pytest.raises(_ext.WnError) as e:      # B * T beyond max_batch * max_time
        eng.synthesize_wide(torch.zeros(B, cfg.cin_channels, T // cfg.hop + 1, device='cuda'), None, out, raw, None, steps_per_graph=SPG)
    assert e.value.code == WN_E_SHAPE
    eng.close()


def test_fp32_mode_is_unsupported():
    from wavenet_vocoder import _ext
    B = 33
    eng, cfg = _engine('s6', B, extra=dict(mi355_compute_dtype='fp32'))
    out, raw = _bufs(cfg, B)
    with pytest.raises(_ext.WnError) as e:
        eng.synthesize_wide(torch.zeros(B, cfg.cin_channels, T // cfg.hop, device='cuda'), None, out, raw, None, steps_per_graph=SPG)
    assert e.value.code == WN_E_UNSUPPORTED
    eng.close()


# ---- 5. an inference-only context of more than 32 streams --------------------------------------------------------------------------------
def test_inference_only_context_of_70_streams():
    import ctypes
    B = 70
    hp, cfg, params, ti, wav, c, g = _case('s6', B)
    eng, _ = _engine('s6', B, inference_only=True)
    nz = _noise(cfg, T, B, seed=4)[0]
    w0 = _wide(eng, cfg, c, g, None, seed=9)
    res0, res1 = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 5)()
    assert eng.lib.wn_test_device_resources(res0) == 0
    w1 = _wide(eng, cfg, c, g, None, seed=9)
    assert eng.lib.wn_test_device_resources(res1) == 0
    assert list(res0) == list(res1), 'a wide run on an inference-only context took or released a device resource'
    assert torch.equal(w0[0], w1[0]) and torch.equal(w0[1], w1[1])
    small, _ = _engine('s6', B, inference_only=True, max_batch=8)
    for spg in (SPG, 0):
        a = _narrow(eng, cfg, c[:8], None, nz[:, :8], spg=spg)
        b = _narrow(small, cfg, c[:8], None, nz[:, :8], spg=spg)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    small.close()
    eng.close()


# ---- 6. the driver -----------------------------------------------------------------------------------------------------------------------
def test_driver_wide_route(tmp_path, monkeypatch):
    """run_synthesis / Synthesizer.synthesize with mi355_synthesis_wide_rows = 64 on 40 utterances of 3 ... 16 frames (one run of 40 streams): 40 wavs and
    map.txt in input order, every wav the one WaveNet.wide gives for the same inputs; mi355_output_stage = device writes the host path's bytes, and with
    mi355_output_deemphasis it is within the bound of test_hip_post.py::test_driver_output_hparams (at most 1 LSB on at most 2 % of the samples).  That
    bound is a rate: on utterances of 48 ... 256 samples one flipped sample is already 2.1 % ... 0.4 %, so the rate is taken over the 40 utterances of
    the call together (about 6 000 samples) and the 1 LSB holds for every utterance."""
    import types
    import hparams as H
    from scipy.io import wavfile
    from datasets.audio import save_wavenet_wav
    from wavenet_vocoder import util
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesize import run_synthesis
    from wavenet_vocoder.synthesizer import Synthesizer, _interp
    monkeypatch.setattr(util, 'plot_spectrogram', lambda *a, **k: None)      # (the plots are not what this test is about)
    monkeypatch.setattr(util, 'waveplot', lambda *a, **k: None)
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],wavenet_synthesis_batch_size=64,mi355_synthesis_wide_rows=64')
    rng = np.random.RandomState(5)
    U = 40
    frames = [3 + (7 * i) % 14 for i in range(U)]                            # 3 ... 16, in no order
    mels = [rng.uniform(-4, 4, size=(frames[i], 16)).astype(np.float32) for i in range(U)]
    names = ['mel-%02d' % i for i in range(U)]
    mels_dir = tmp_path / 'mels'; mels_dir.mkdir()
    for n, m in zip(names, mels):
        np.save(str(mels_dir / (n + '.npy')), m)
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(4, 16 * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    state = model.state_dict()
    model.engine.close()
    # the driver: 40 wavs and map.txt in input order
    out = str(tmp_path / 'out')
    run_synthesis(types.SimpleNamespace(model='WaveNet', mels_dir=str(mels_dir), speaker_id=None), ckpt, out, hp0)
    wav_dir = os.path.join(out, 'wavs')
    rows = [l.split('|') for l in open(os.path.join(wav_dir, 'map.txt')).read().strip().split('\n')]
    assert [os.path.basename(r[0]) for r in rows] == [n + '.npy' for n in names]
    assert [os.path.basename(r[1]) for r in rows] == ['wavenet-audio-%s.wav' % n for n in names]
    assert sorted(f for f in os.listdir(wav_dir) if f.endswith('.wav')) == ['wavenet-audio-%s.wav' % n for n in names]
    plain = [open(r[1], 'rb').read() for r in rows]
    # every wav is WaveNet.wide of the same inputs (a fresh model: the same call counter, so the same seeds)
    model = WaveNet(hp0)
    model.build(U, 16 * 16, inference_only=True)
    model.load_state_dict(state)
    rng_ = (-hp0.max_abs_value, hp0.max_abs_value) if hp0.symmetric_mels else (0, hp0.max_abs_value)
    cl = []
    for m in mels:
        m = np.clip(m, rng_[0], rng_[1]) if hp0.clip_for_wavenet else m
        m = _interp(m, rng_).astype(np.float32) if hp0.normalize_for_wavenet else m
        cl.append(torch.from_numpy(np.ascontiguousarray(m.T)))
    samples, info = model.wide(cl, rows=64)
    assert info['plan'][0] == [sorted(range(U), key=lambda i: -frames[i])] and model.engine.synth_path == 'graph'
    for i, s in enumerate(samples):
        assert s.shape[0] == frames[i] * 16
        ref = str(tmp_path / 'ref.wav')
        save_wavenet_wav(s.float().cpu().numpy(), ref, sr=hp0.sample_rate)
        assert open(ref, 'rb').read() == plain[i], 'utterance %d differs from WaveNet.wide' % i
    model.engine.close()

    def run(tag, extra):
        hp = H._build(); hp.parse(base + extra)
        od = str(tmp_path / tag); os.makedirs(od)
        s = Synthesizer(); s.load(ckpt, hp)
        files = s.synthesize(mels, None, names, od, None)
        s.model.engine.close()
        for st in s._post_stages.values():
            st.close()
        assert [os.path.basename(f) for f in files] == ['wavenet-audio-%s.wav' % n for n in names]
        return [open(f, 'rb').read() for f in files], [wavfile.read(f)[1].astype(np.int32) for f in files]

    assert run('device', ',mi355_output_stage=device')[0] == plain
    host = run('host_de', ',mi355_output_deemphasis=True')
    dev = run('device_de', ',mi355_output_deemphasis=True,mi355_output_stage=device')
    flips = total = 0
    for i, (h, d) in enumerate(zip(host[1], dev[1])):
        assert h.shape == d.shape == (frames[i] * 16,)
        diff = np.abs(h - d)
        assert diff.max() <= 1, i
        flips += int(np.sum(diff > 0)); total += diff.size
    print('\nwide driver: %d of %d samples differ by one LSB between the device and the host output stage' % (flips, total))
    assert flips <= 0.02 * total
    assert host[0] != plain                                                                      # de-emphasis really changed the files


def test_driver_wide_route_hooks(tmp_path):
    """the wide route with the reconstruction and the pitch check on, host and device output stage: one row per utterance in reconstruction.tsv / pitch.tsv,
    in input order, and the wavs byte-identical to the run with both off"""
    import hparams as H
    from wavenet_vocoder.models.wavenet import WaveNet
    from wavenet_vocoder.synthesizer import Synthesizer
    base = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,hop_size=16,'
            'upsample_scales=[4,4],n_fft=256,win_size=256,mi355_pitch_window=64,mi355_pitch_fmin=552,mi355_pitch_fmax=4410,wavenet_synthesis_batch_size=64,'
            'mi355_synthesis_wide_rows=64')
    rng = np.random.RandomState(6)
    frames = [30, 44, 37, 50, 41]
    mels = [rng.uniform(-4, 4, size=(f, 16)).astype(np.float32) for f in frames]
    refs = [rng.uniform(-0.5, 0.5, size=f * 16).astype(np.float32) for f in frames]
    names = ['u%d' % i for i in range(len(frames))]
    hp0 = H._build(); hp0.parse(base)
    model = WaveNet(hp0)
    model.build(4, max(frames) * 16)
    ckpt = str(tmp_path / 'model.pt')
    torch.save(model.state_dict(), ckpt)
    model.engine.close()

    def run(tag, extra='', pitch=False):
        hp = H._build(); hp.parse(base + extra)
        od = str(tmp_path / tag); os.makedirs(od)
        s = Synthesizer(); s.load(ckpt, hp)
        if pitch:
            s.pitch_references = [r.copy() for r in refs]
        files = s.synthesize(mels, None, names, od, None)
        s.model.engine.close()
        for st in s._post_stages.values():
            st.close()
        for chk in (s._recon, s._pitch_chk):
            if chk is not None:
                chk.close()
        return [open(f, 'rb').read() for f in files], od

    plain, out0 = run('plain')
    assert not os.path.exists(os.path.join(out0, 'reconstruction.tsv')) and not os.path.exists(os.path.join(out0, 'pitch.tsv'))
    for tag, extra in (('host', ''), ('device', ',mi355_output_stage=device')):
        got, od = run(tag, extra + ',mi355_reconstruction_check=True,mi355_pitch_check=True', pitch=True)
        assert got == plain, tag
        for tsv in ('reconstruction.tsv', 'pitch.tsv'):
            rows = [l.split('\t') for l in open(os.path.join(od, tsv)).read().strip().split('\n')]
            assert [r[0] for r in rows if r[0] in names] == names, (tag, tsv, [r[0] for r in rows])
