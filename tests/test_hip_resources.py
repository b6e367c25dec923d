"""Ownership of device resources (csrc/wn_dev.h): every buffer, stream, event and graph exec a context creates is released with it, and an
inference-only context takes no memory after wn_create.  Checked on the library's own counters (wn_test_device_resources: live buffers, streams,
events, graph execs, buffer allocations ever) -- hipMemGetInfo moves with the other processes of a shared device, a count of our handles does not.
Every assertion is on DELTAS around the life of one engine: other engines of the pytest process may be alive.  SMALL shape throughout (what can
go wrong is host bookkeeping); the numbers the engines compute are the business of the parity tests."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from hip_util import SMALL, make_hp

pytestmark = pytest.mark.gpu

B, T, TC = 3, 128, 8          # hop 16
GIN = dict(gin_channels=16, use_speaker_embedding=True, n_speakers=4)
TRAIN = dict(SMALL, wavenet_dropout=0.05, wavenet_weight_normalization=True, **GIN)


def counters():
    from wavenet_vocoder import _ext
    v = (ctypes.c_int64 * 5)()
    assert _ext.load_library().wn_test_device_resources(v) == 0
    return np.array(list(v), dtype=np.int64)


def make_engine(over, inference_only=False, pack=True):
    from wavenet_vocoder import _ext
    hp = make_hp(**over)
    eng = _ext.Engine(hp, B, T, inference_only=inference_only)
    if pack:
        eng.pack_weights(weights(eng))
    return eng


def weights(eng):
    g = torch.Generator().manual_seed(7)
    return (0.05 * torch.randn(eng.n_params, generator=g)).cuda()


def batch(eng, nb=B):
    g = torch.Generator().manual_seed(11)
    wav = (0.3 * torch.randn(nb, T, generator=g)).clamp(-0.999, 0.999)
    c = torch.rand(nb, eng.cfg.cin_channels, TC, generator=g).cuda()
    return wav.view(nb, 1, T).contiguous().cuda(), wav.view(nb, T, 1).contiguous().cuda(), c


def speakers(eng, nb):
    if eng.cfg.gin_channels > 0:
        eng.set_global_condition(torch.arange(nb, dtype=torch.int32).cuda() % 4)


def train_step(eng, seed, optimise=False):
    x, y, c = batch(eng)
    ln = torch.tensor([T, T - 17, T - 40], dtype=torch.int32, device='cuda')
    loss = torch.zeros(1, device='cuda'); grads = torch.zeros(eng.n_params, device='cuda')
    speakers(eng, B)
    eng.train_fwd(x, c, y, ln, seed, loss)
    eng.train_bwd(grads)
    if optimise:
        p = (0.05 * torch.randn(eng.n_params)).cuda()
        eng.optim_step(p, grads, torch.zeros_like(p), torch.zeros_like(p), p.clone(), 1e-3, 0)
    torch.cuda.synchronize()
    return x, y, c, ln


def synth_calls(eng, spgs):
    """whole utterances at B = 1 then 3 on every path of `spgs` (every grow path runs), a stream of two pushes, a slot session of two pushes"""
    slots = eng.cfg.compute_dtype == 0          # (slot sessions are not built for the fp32 mode)
    for spg in spgs:
        for nb in (1, B):
            _, _, c = batch(eng, nb)
            speakers(eng, nb)
            out = torch.empty(nb, T, device='cuda')
            eng.synthesize(c, None, out, steps_per_graph=spg, seed=3)
            torch.cuda.synchronize(); eng.synth_check()
        _, _, c = batch(eng)
        speakers(eng, B)
        out = torch.empty(B, T, device='cuda')
        eng.stream_begin(B, seed=5, steps_per_graph=spg)
        n = eng.stream_push(c[:, :, :3].contiguous(), out) + eng.stream_push(c[:, :, 3:].contiguous(), out, final=True)
        torch.cuda.synchronize(); eng.synth_check()
        assert n == T
        if slots:
            eng.slots_begin(B, steps_per_graph=spg)
            for s in range(B):
                eng.slot_open(s, seed=s, g=torch.tensor([s % 4], dtype=torch.int32).cuda() if eng.cfg.gin_channels > 0 else None)
            n = eng.slots_push(c[:, :, :3].contiguous(), [3] * B, [False] * B, out)
            n = [a + b for a, b in zip(n, eng.slots_push(c[:, :, 3:].contiguous(), [TC - 3] * B, [True] * B, out))]
            torch.cuda.synchronize(); eng.synth_check()
            assert n == [T] * B


def run_training(eng):
    eng.profile(True)                            # event pairs around every gate launch (wn_ctx::pev)
    x, y, c, ln = train_step(eng, 1, optimise=True)
    assert eng.profile_result()[1] > 0
    eng.profile(False)
    eng.trace_arm(1)
    train_step(eng, 2)
    assert len(eng.trace_read()) > 0
    stats = torch.zeros(B, 3, device='cuda')
    eng.eval_fwd(x, c, y, ln, stats)
    for parts in (2, 3):                         # the third part stream is created on demand
        eng.set_batch_parts(parts)
        train_step(eng, 3 + parts)


def run_training_f32(eng):
    train_step(eng, 1)


def run_synth_training_ctx(eng):
    synth_calls(eng, (8, 0))                     # launch-per-layer graphs of 8 steps (a graph exec exists), then the pipeline
    assert eng.synth_path == 'pipeline'


def run_synth_f32(eng):
    synth_calls(eng, (8,))
    assert eng.synth_path == 'graph-fp32'


def run_mel(_):
    from wavenet_vocoder import _ext
    from mel_util import make_signal, mel_hparams, run_analyzer
    wavs = [make_signal('harmonic', 9 * 275 + 7, 1), make_signal('noise', 4 * 275, 2)]
    an = _ext.MelAnalyzer(mel_hparams(), len(wavs), max(len(w) for w in wavs))
    run_analyzer(an, wavs)
    an.close()


CASES = {
    'training': (TRAIN, False, run_training),
    'training_fp32': (dict(TRAIN, mi355_compute_dtype='fp32'), False, run_training_f32),
    'synthesis_on_training_context': (dict(SMALL, **GIN), False, run_synth_training_ctx),
    'synthesis_fp32': (dict(SMALL, mi355_compute_dtype='fp32', **GIN), False, run_synth_f32),
    'synthesis_inference_only': (dict(SMALL, **GIN), True, run_synth_training_ctx),
    'mel_analyzer': (None, False, run_mel),
}


@pytest.mark.parametrize('name', list(CASES))
def test_everything_a_context_creates_is_released_with_it(name):
    """create, exercise, destroy: live buffers, streams, events and graph execs are back where they were (and something was created in between)"""
    over, inference_only, run = CASES[name]
    gc.collect()
    before = counters()
    eng = make_engine(over, inference_only) if over is not None else None
    run(eng)
    torch.cuda.synchronize()
    during = counters()
    if eng is not None:
        eng.close()
    del eng
    gc.collect()
    after = counters()
    print('\n%s: live (buffers, streams, events, graph execs) +%s while alive, %s after close; %d allocations' %
          (name, (during[:4] - before[:4]).tolist(), (after[:4] - before[:4]).tolist(), after[4] - before[4]))
    assert after[4] > before[4]                                      # the case did allocate through the library
    assert (after[:4] - before[:4]).tolist() == [0, 0, 0, 0]
    if name == 'training':
        assert during[1] - before[1] >= 3 and during[2] - before[2] > 40      # st2, st3, a third part stream; the bucket / part events and the profile's pairs
    if name in ('synthesis_on_training_context', 'synthesis_inference_only'):
        assert during[3] - before[3] == 1                            # the step graph of the launch-per-layer path


def test_inference_only_context_allocates_nothing_after_create():
    """The contract of cfg.inference_only (include/wavenet_mi355.h): whole utterances at B = 1 and B = max_batch, a stream of three pushes and a slot
    session in which a slot is opened, finished and reopened -- all within pipe_cap, on the path wn_create pre-sized -- take no buffer.  Counted from
    wn_create itself.  The one allocation after it is not a synthesis call's: the FIRST wn_pack_weights of any context builds the job table of the pack
    launch (wn_launch_pack: pack_jobs_dev, once); a second pack takes nothing."""
    eng = make_engine(dict(SMALL, **GIN), inference_only=True, pack=False)
    created = counters()[4]
    eng.pack_weights(weights(eng))
    assert counters()[4] == created + 1                              # the pack job table, and nothing else
    eng.pack_weights(weights(eng))
    created += 1
    assert counters()[4] == created
    assert eng.pipeline_eligible(B)
    _, _, c = batch(eng)
    out = torch.empty(B, T, device='cuda')
    for nb in (1, B):
        speakers(eng, nb)
        eng.synthesize(c[:nb].contiguous(), None, out[:nb], seed=1)
        torch.cuda.synchronize(); eng.synth_check()
        assert eng.synth_path == 'pipeline'
    speakers(eng, B)
    eng.stream_begin(B, seed=2)
    n = sum(eng.stream_push(c[:, :, a:b].contiguous(), out, final=b == TC) for a, b in ((0, 2), (2, 5), (5, TC)))
    torch.cuda.synchronize(); eng.synth_check()
    assert n == T
    eng.slots_begin(B)
    for rep in range(2):
        eng.slot_open(0, seed=rep, g=torch.tensor([rep], dtype=torch.int32).cuda())
        assert eng.slots_push(c[:, :, :2].contiguous(), [2, 0, 0], [True, False, False], out) == [2 * eng.hop, 0, 0]
        assert eng.slot_frames_done(0) == -1                         # finished: the slot is idle again
    torch.cuda.synchronize(); eng.synth_check()
    assert counters()[4] == created
    eng.close()
