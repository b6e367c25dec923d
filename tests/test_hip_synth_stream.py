"""Streaming synthesis (wn_synth_stream_begin / _push): mel frames pushed as they arrive give the same bits as ONE wn_synthesize over the
concatenated frames -- out_samples and out_raw compared with torch.equal -- on the persistent pipeline (paper model, hparams.py's default model on
three instances), the launch-per-layer graph path, across ring wraps, training steps between pushes and utterances longer than max_time."""
import numpy as np
import pytest
import torch

from hip_util import make_hp, oracle_cfg, synth_batch, upload_params
from oracle import mulaw as M
from oracle import wavenet_oracle as O
from test_hip_synth import _noise, _setup
from test_hip_synth_pipe import PAPER_FULL

pytestmark = pytest.mark.gpu

WN_E_SHAPE, WN_E_STATE = -2, -5


def _alloc(eng, cfg, B, n):
    scalar = cfg.input_type != 'mulaw-quantize'
    out = torch.full((B, n), -7, device='cuda', dtype=torch.float32 if scalar else torch.int32)
    raw = torch.full((B, cfg.out_channels, n), float('nan'), device='cuda')
    return out, raw


def _oneshot(eng, cfg, c, noise=None, ti=None, seed=0, spg=0):
    B, T = c.shape[0], c.shape[-1] * cfg.hop
    out, raw = _alloc(eng, cfg, B, T)
    eng.synthesize(c.cuda(), None if noise is None else noise.cuda(), out, raw, ti, steps_per_graph=spg, seed=seed)
    torch.cuda.synchronize(); eng.synth_check()
    return out.cpu(), raw.cpu(), eng.synth_config()


def _stream(eng, cfg, c, pushes, noise=None, ti=None, seed=0, spg=0, between=None):
    """pushes: frame counts; the last one is pushed with final=1.  noise [T, B, nps] / ti [B, T] of the whole utterance are cut per push
    (the span a push generates is known before it is enqueued: wn_synth_stream_lookahead)."""
    B, Tc, hop = c.shape[0], c.shape[-1], cfg.hop
    assert sum(pushes) == Tc
    left, right = eng.stream_lookahead()
    eng.stream_begin(B, seed=seed, steps_per_graph=spg)
    outs, raws, done, pushed = [], [], 0, 0
    cd = c.cuda()
    for i, k in enumerate(pushes):
        final = i == len(pushes) - 1
        pushed += k
        gen_end = pushed if final else max(done, pushed - right)
        n = (gen_end - done) * hop
        t0 = done * hop
        out, raw = _alloc(eng, cfg, B, max(n, 1))
        nz = None if noise is None else noise[t0:t0 + n].contiguous().cuda()
        tt = None if ti is None else ti[:, t0:t0 + n].contiguous()
        got = eng.stream_push(cd[:, :, pushed - k:pushed].contiguous() if k else None, out, raw, nz, tt, final=final)
        assert got == n
        done = gen_end
        outs.append(out[:, :n]); raws.append(raw[:, :, :n])
        if between is not None:
            between(i)
    torch.cuda.synchronize(); eng.synth_check()
    assert done == Tc
    return torch.cat(outs, 1).cpu(), torch.cat(raws, 2).cpu(), eng.synth_config()


def _same(a, b):
    assert a[0].shape == b[0].shape and a[1].shape == b[1].shape
    assert torch.equal(a[0], b[0]), 'out_samples differ at %d positions' % int((a[0] != b[0]).sum())
    assert torch.equal(a[1], b[1]), 'out_raw differs at %d positions (max %.3e)' % (int((a[1] != b[1]).sum()), float((a[1] - b[1]).abs().max()))


# irregular schedules: 1-frame pushes, empty pushes, pushes shorter than the lookahead, a final push carrying frames
SCHED_80 = [1, 0, 7, 1, 13, 2, 0, 9, 16, 1, 5, 3, 22]
SCHED_80B = [3, 1, 1, 0, 24, 8, 11, 0, 17, 15]


@pytest.mark.parametrize('B', [1, 8])
def test_stream_paper_model_pipeline_bit_identical(B):
    """C4's model (24 layers / 2 stacks, 10-MoL, '2D'), 80 frames = 22 000 steps: every d = 2048 queue wraps several times, chunk edges fall on
    both sides of a wrap; device noise (offset fill across pushes) and explicit noise; the stream runs the same pipeline configuration."""
    Tc = 80
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, **PAPER_FULL)
    assert eng.stream_lookahead() == (0, 0)
    ref = _oneshot(eng, cfg, c, seed=1234)
    got = _stream(eng, cfg, c, SCHED_80, seed=1234)
    assert ref[2]['path'] == 'pipeline' and got[2] == ref[2]
    _same(got, ref)
    nz, _ = _noise(cfg, T, B, seed=4)
    ref = _oneshot(eng, cfg, c, noise=nz)
    got = _stream(eng, cfg, c, SCHED_80B, noise=nz)
    _same(got, ref)
    print('\npaper model B=%d: stream == one-shot over %d samples (%s)' % (B, T, ref[2]))
    eng.close()


def test_stream_default_model_subpixel_three_instances():
    """hparams.py's own model (20 layers, R = 128, Gaussian head, 'SubPixel' [11, 25]: two frames of context on each side) at its
    synthesis batch of 20 streams on three pipeline instances."""
    hp = make_hp()
    cfg = oracle_cfg(hp)
    assert cfg.upsample_type == 'SubPixel' and cfg.out_channels == 2
    B, Tc = 20, 12
    T = Tc * cfg.hop
    from wavenet_vocoder import _ext
    eng = _ext.Engine(hp, B, T)
    params = O.init_params(cfg, seed=11, bias_scale=0.05)
    eng.pack_weights(upload_params(eng, params))
    _, c = synth_batch(cfg, B, T, seed=3)
    left, right = eng.stream_lookahead()
    assert (left, right) == (2, 2)
    ref = _oneshot(eng, cfg, c, seed=99)
    assert ref[2]['path'] == 'pipeline' and ref[2]['instances'] == 3
    got = _stream(eng, cfg, c, [1, 1, 0, 3, 2, 4, 1], seed=99)          # pushes shorter than the lookahead; the final one brings the held-back frames
    assert got[2] == ref[2]
    _same(got, ref)
    k_last = Tc - (Tc - 1 - right)                                           # the final push generates the held-back frames and its own
    feats = torch.empty(B, cfg.cin_channels, k_last * cfg.hop, device='cuda')
    eng.upsampled_features(feats)
    full = torch.empty(B, cfg.cin_channels, T, device='cuda')
    eng.synthesize(c.cuda(), None, torch.empty(B, T, device='cuda'), seed=99)
    eng.upsampled_features(full)
    torch.cuda.synchronize()
    assert torch.equal(feats.cpu(), full.cpu()[:, :, T - k_last * cfg.hop:])
    eng.close()


def test_stream_launch_per_layer_mulaw_speaker_teacher_forced():
    """The launch-per-layer hipGraph path (steps_per_graph = 8), mu-law-quantize categorical head, speaker embedding, teacher forcing; push
    lengths whose sample counts are not multiples of 8."""
    B, Tc = 3, 19
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, input_type='mulaw-quantize', out_channels=256, quantize_channels=256,
                                             gin_channels=16, use_speaker_embedding=True, n_speakers=4, upsample_scales=[3, 5], hop_size=15)
    eng.set_global_condition(torch.tensor([2, 0, 3], dtype=torch.int32, device='cuda'))
    ti = torch.from_numpy(M.mulaw_quantize(wav.numpy())).int()
    ti[:, T // 2:] = ti[:, :T - T // 2].flip(1)          # (the second half is not the utterance: the fed-back ids matter)
    ti = ti.contiguous().cuda()
    ref = _oneshot(eng, cfg, c, ti=ti, seed=5, spg=8)
    assert ref[2]['path'] == 'graph'
    got = _stream(eng, cfg, c, [1, 2, 0, 5, 1, 3, 7], ti=ti, seed=5, spg=8)
    _same(got, ref)
    ref = _oneshot(eng, cfg, c, seed=6, spg=8)                                    # free running: the fed-back class ids cross the push edges
    got = _stream(eng, cfg, c, [4, 4, 0, 1, 10], seed=6, spg=8)
    _same(got, ref)
    eng.close()


def test_stream_isolated_from_training_steps():
    """A training context: wn_train_fwd + wn_train_bwd between pushes (eval use) rewrite the conditioning, the gate-bias table and the
    activations; the stream keeps its own state and still equals the one-shot run (pipeline, global conditioning)."""
    B, Tc = 4, 24
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, gin_channels=8, use_speaker_embedding=False)
    g = torch.randn(B, 8, generator=torch.Generator().manual_seed(2)).cuda()
    eng.set_global_condition(g)
    ref = _oneshot(eng, cfg, c, seed=21)
    assert ref[2]['path'] == 'pipeline'
    wav2, c2 = synth_batch(cfg, B, T, seed=8)
    x = wav2.view(B, 1, T).contiguous().cuda(); y = wav2.view(B, T, 1).contiguous().cuda()
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda'); loss = torch.zeros(1, device='cuda')
    grads = torch.empty(eng.n_params, device='cuda')
    g2 = torch.randn(B, 8, generator=torch.Generator().manual_seed(3)).cuda()

    def train(i):
        # (set_global_condition would end the stream: the training step runs under the condition already set; its forward rewrites the
        # context's conditioning, bias table and activations from other frames)
        eng.train_fwd(x, c2.cuda(), y, ln, 77 + i, loss)
        eng.train_bwd(grads)

    eng.set_global_condition(g)
    got = _stream(eng, cfg, c, [5, 1, 7, 0, 11], seed=21, between=train)
    _same(got, ref)
    assert torch.isfinite(loss).all()
    # ... and wn_set_global_condition / wn_synthesize / wn_pack_weights end it
    eng.set_global_condition(g2)
    eng.stream_begin(B, seed=21)
    eng.set_global_condition(g2)
    out, raw = _alloc(eng, cfg, B, 4 * cfg.hop)
    with pytest.raises(Exception) as ei:
        eng.stream_push(c[:, :, :4].contiguous().cuda(), out, raw)
    assert getattr(ei.value, 'code', None) == WN_E_STATE
    eng.close()


def test_stream_longer_than_max_time_inference_only():
    """An inference-only context sized for 16 frames (max_time 4 400 at hop 275): sixteen pushes of 8 frames produce 35 200 samples, equal to
    one run on a context large enough for all of them; the stream never allocates (wn_workspace_bytes unchanged)."""
    from wavenet_vocoder import _ext
    B, Tc = 2, 128
    hp = make_hp(**dict(__import__('hip_util').SMALL, **PAPER_FULL))
    cfg = oracle_cfg(hp)
    T = Tc * cfg.hop
    params = O.init_params(cfg, seed=11, bias_scale=0.05)
    big = _ext.Engine(hp, B, T, inference_only=True)
    big.pack_weights(upload_params(big, params))
    _, c = synth_batch(cfg, B, T, seed=3)
    ref = _oneshot(big, cfg, c, seed=77)
    big.close()
    small = _ext.Engine(hp, B, 16 * cfg.hop, inference_only=True)
    small.pack_weights(upload_params(small, params))
    ws = small.lib.wn_workspace_bytes(small.h)
    free0 = torch.cuda.mem_get_info()[0]
    got = _stream(small, cfg, c, [8] * 16, seed=77)
    assert small.lib.wn_workspace_bytes(small.h) == ws
    assert got[2] == ref[2]
    _same(got, ref)
    print('\n%d samples through a context of max_time %d; free device memory %d -> %d' % (T, 16 * cfg.hop, free0, torch.cuda.mem_get_info()[0]))
    small.close()


def test_stream_state_errors():
    from wavenet_vocoder import _ext
    B, Tc = 2, 8
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc)
    cd = c.cuda()
    out, raw = _alloc(eng, cfg, B, T)

    def code(fn):
        with pytest.raises(_ext.WnError) as ei:
            fn()
        return ei.value.code

    push = lambda k=2, final=False: eng.stream_push(cd[:, :, :k].contiguous(), out, raw, final=final)
    assert code(push) == WN_E_STATE                                           # before begin
    eng.stream_begin(B, seed=1)
    assert push(2, final=True) == 2 * cfg.hop
    assert code(push) == WN_E_STATE                                           # after final
    eng.stream_begin(B, seed=1)
    push()
    eng.synthesize(cd, None, out, raw, seed=1)
    assert code(push) == WN_E_STATE                                           # after wn_synthesize
    eng.stream_begin(B, seed=1)
    push()
    eng.pack_weights(upload_params(eng, params))
    assert code(push) == WN_E_STATE                                           # after wn_pack_weights
    eng.stream_begin(B, seed=1)
    push()
    eng.pipeline_dtype(True)
    assert code(push) == WN_E_STATE                                           # after wn_synth_pipe_dtype
    eng.stream_begin(B, seed=1)
    big = torch.cat([cd, cd], 2).contiguous()                                 # 16 frames > max_time / hop = 8 in one push
    assert code(lambda: eng.stream_push(big, out, raw)) == WN_E_SHAPE
    assert push(8, final=True) == T                                           # (a rejected push leaves the stream as it was)
    torch.cuda.synchronize(); eng.synth_check()
    eng.close()


def test_facade_stream_equals_incremental():
    """WaveNet.stream(): pushes of mel frames give the samples WaveNet.incremental generates for the same call (same seed derivation)."""
    from wavenet_vocoder.models.wavenet import WaveNet
    B, Tc = 3, 20
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc)
    flat = upload_params(eng, params)
    eng.close()
    model = WaveNet(hp)
    model.build(B, T, params=flat.cpu())
    ref = model.incremental(None, c=c.cuda(), time_length=T).cpu()
    model._synth_calls = 0
    st = model.stream(B)
    assert st.lookahead == (0, 0)
    parts = [st.push(c[:, :, a:b].cuda(), final=(b == Tc)) for a, b in ((0, 1), (1, 1), (1, 9), (9, 20))]
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([p.cpu() for p in parts], 1), ref)


def test_stream_fp32_mode_resize():
    """fp32 mode (mi355_compute_dtype='fp32': fp32 weights, queues and accumulation, launch-per-layer) with 'Resize' upsampling (one frame of
    context on each side): the conditioning of a push comes from a window whose first rows are context."""
    B, Tc = 2, 11
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, mi355_compute_dtype='fp32', upsample_type='Resize')
    assert eng.stream_lookahead() == (1, 1)
    ref = _oneshot(eng, cfg, c, seed=31, spg=8)
    assert ref[2]['path'] == 'graph-fp32'
    got = _stream(eng, cfg, c, [1, 2, 0, 3, 1, 4], seed=31, spg=8)
    assert got[2]['path'] == 'graph-fp32'
    _same(got, ref)
    eng.close()


@pytest.mark.parametrize('pushes', [[2, 2, 2], [2, 2, 3]])
@pytest.mark.parametrize('dtype', ['bf16', 'fp32'])
def test_stream_replays_the_step_graph_across_pushes(dtype, pushes):
    """The captured step graph (steps_per_graph = 4) is REPLAYED by a later push when every pointer and size it carries is the same, and captured
    again when one differs.  Pushes 1 and 2 write into the same output tensors (copied out in between; device noise, no lookahead: the noise buffer and
    the conditioning rows are the same too), so push 2 replays push 1's graph 8 times from another t0; push 3 writes into other tensors -- and, with 3
    frames, at another pitch -- so the graph is captured again.  32 / 48 samples per push wrap every queue (4 and 8 slots) several times."""
    B, Tc = 3, sum(pushes)
    kw = dict(mi355_compute_dtype='fp32') if dtype == 'fp32' else {}
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, **kw)
    path = 'graph-fp32' if dtype == 'fp32' else 'graph'
    assert eng.stream_lookahead() == (0, 0)
    ref = _oneshot(eng, cfg, c, seed=17, spg=4)
    assert ref[2]['path'] == path
    cd, hop = c.cuda(), cfg.hop
    eng.stream_begin(B, seed=17, steps_per_graph=4)
    shared = _alloc(eng, cfg, B, pushes[0] * hop)
    outs, raws, f0 = [], [], 0
    for i, k in enumerate(pushes):
        out, raw = shared if i < 2 else _alloc(eng, cfg, B, k * hop)
        assert eng.stream_push(cd[:, :, f0:f0 + k].contiguous(), out, raw, final=(i == len(pushes) - 1)) == k * hop
        outs.append(out.clone()); raws.append(raw.clone())
        f0 += k
    torch.cuda.synchronize(); eng.synth_check()
    assert eng.synth_config()['path'] == path
    _same((torch.cat(outs, 1).cpu(), torch.cat(raws, 2).cpu()), ref)
    eng.close()


@pytest.mark.parametrize('utype', ['SubPixel', 'Resize'])
def test_stream_launch_per_layer_with_lookahead(utype):
    """The launch-per-layer path (steps_per_graph = 8) with a nonzero lookahead: the window offset / stride of its conditioning rows."""
    B, Tc = 3, 13
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc, upsample_type=utype)
    left, right = eng.stream_lookahead()
    assert left > 0 and right > 0
    ref = _oneshot(eng, cfg, c, seed=41, spg=8)
    assert ref[2]['path'] == 'graph'
    got = _stream(eng, cfg, c, [1, 1, 2, 0, 5, 1, 3], seed=41, spg=8)
    _same(got, ref)
    eng.close()


def test_stream_poisoned_by_a_flagged_pipeline_run(monkeypatch):
    """A pipeline run of the stream whose abort flag is raised (the WN_PIPE_TEST_ABORT hook sets the flag as a timed-out hand-off would, no
    fault involved) is reported by wn_synth_check, and every later push returns WN_E_STATE until the next begin."""
    from wavenet_vocoder import _ext
    B, Tc = 2, 8
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc)
    cd = c.cuda()
    out, raw = _alloc(eng, cfg, B, T)
    eng.stream_begin(B, seed=3)
    monkeypatch.setenv('WN_PIPE_TEST_ABORT', '1')
    eng.stream_push(cd[:, :, :2].contiguous(), out, raw)
    monkeypatch.delenv('WN_PIPE_TEST_ABORT')
    torch.cuda.synchronize()
    with pytest.raises(_ext.WnError) as ei:
        eng.synth_check()
    assert ei.value.code == -3
    with pytest.raises(_ext.WnError) as ei:
        eng.stream_push(cd[:, :, 2:4].contiguous(), out, raw)
    assert ei.value.code == WN_E_STATE
    eng.stream_begin(B, seed=3)                                              # a new stream is clean
    assert eng.stream_push(cd, out, raw, final=True) == T
    torch.cuda.synchronize(); eng.synth_check()
    eng.close()


def test_stream_push_checks_the_frame_shape():
    from wavenet_vocoder import _ext
    B, Tc = 2, 4
    hp, cfg, eng, params, wav, c, T = _setup(B, Tc)
    out, raw = _alloc(eng, cfg, B, T)
    eng.stream_begin(B)
    with pytest.raises(ValueError):
        eng.stream_push(c[:1].contiguous().cuda(), out, raw)                 # batch of 1 into a stream of 2
    eng.stream_end()
    with pytest.raises(_ext.WnError):
        eng.stream_push(c.cuda(), out, raw)
    eng.close()


def test_synthesize_driver_chunked_wavs_byte_identical(tmp_path):
    """synthesize.py (wavenet_synthesize from a checkpoint) with mi355_synthesis_chunk_frames=3 writes the same wav files, byte for byte, as the
    one-call path (= 0)."""
    import os
    import types
    import hparams as H
    from test_hip_drivers import _dataset
    from wavenet_vocoder.train import wavenet_train
    from wavenet_vocoder.synthesize import wavenet_synthesize
    root = str(tmp_path)
    meta = _dataset(root)
    hp = H._build()
    hp.parse('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,out_channels=30,'
             'hop_size=16,upsample_scales=[4,4],max_time_steps=512,wavenet_batch_size=4,wavenet_test_batches=1,wavenet_synthesis_batch_size=2,'
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
        for chunk, od in ((0, 'one/'), (3, 'chunked/')):
            hp.set_hparam('mi355_synthesis_chunk_frames', chunk)
            wavenet_synthesize(types.SimpleNamespace(model='WaveNet', mels_dir=mels_dir, output_dir=od, speaker_id=None), hp, save_dir)
    finally:
        os.chdir(cwd)
    a = sorted(os.listdir(os.path.join(root, 'wavenet_one', 'wavs'))); b = sorted(os.listdir(os.path.join(root, 'wavenet_chunked', 'wavs')))
    wavs = [f for f in a if f.endswith('.wav')]
    assert a == b and len(wavs) == 3
    for f in wavs:
        assert open(os.path.join(root, 'wavenet_one', 'wavs', f), 'rb').read() == open(os.path.join(root, 'wavenet_chunked', 'wavs', f), 'rb').read(), f
