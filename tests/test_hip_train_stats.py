"""Training summaries on the device (csrc/wn_stats.hip): the histogram kernels and the per-tensor statistics against the numpy reference of
tests/stats_util.py (counts, extremes and non-finite counters equal; sums inside the derived any-order bound) and, bit for bit, against the host hook, a
second run and other pitches; the statistics of a real gradient buffer against torch float64; and the training driver with the key on and off, whose steps
must not differ in a single bit."""
import json
import os
import types

import numpy as np
import pytest
import torch

import stats_util as SU

pytestmark = pytest.mark.gpu

NET = ('layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,hop_size=16,upsample_scales=[4,4],'
       'wavenet_test_batches=1,wavenet_learning_rate=1e-3,wavenet_dropout=0.05,wavenet_clip_gradients=True')
TINY = NET + ',max_time_steps=512,wavenet_batch_size=4'
# The driver run compares LOGGED losses bit for bit.  The training loss kernels add one partial per workgroup of 256 positions to a scalar with a float
# atomic, so the logged loss of a batch of more than 512 positions depends on the order in which its workgroups retire -- from run to run of
# the same code, key or no key.  2 x 256 positions are two workgroups: (0 + a) + b == (0 + b) + a, the logged loss is a function of the step alone, and a
# difference between the two runs is the summary's doing.  The kernels' other paths are covered by the shapes above.
DRIVE = NET + ',max_time_steps=256,wavenet_batch_size=2'
HEADS = {'mol': 'input_type=raw,out_channels=30', 'gaussian': 'input_type=raw,out_channels=2',
         'softmax': 'input_type=mulaw-quantize,quantize_channels=256,out_channels=256'}


@pytest.fixture(scope='module')
def stats():
    from wavenet_vocoder import _ext
    _, table = SU.tensor_table()
    s = _ext.TrainStats(8, 4200, table)
    yield s
    s.close()


@pytest.fixture(scope='module')
def references():
    """numpy reference and host-hook result of every (shape, value set), computed once"""
    from wavenet_vocoder import _ext
    out = {}
    for B, T, pitch in SU.SHAPES:
        ln = SU.ragged_lengths(B, T)
        for name, x in SU.value_sets(B, T).items():
            out[(B, T, name)] = (x, ln, SU.reference_hist(x, ln), _ext.TrainStats.histogram_host(x, ln))
    return out


@pytest.mark.parametrize('name', ['edges', 'audio', 'log_scales'])
@pytest.mark.parametrize('B,T,pitch', SU.SHAPES)
def test_histogram_against_numpy_and_bit_identical_to_the_hook(stats, references, B, T, pitch, name):
    x, ln, ref, hook = references[(B, T, name)]
    dev_ln = torch.from_numpy(ln).cuda()
    got = stats.histogram(torch.from_numpy(SU.with_pitch(x, pitch, ln)).cuda(), dev_ln, T=T)
    SU.check_hist(got, ref, 'device %s %s' % ((B, T, pitch), name))
    assert got['num'] + got['n_nan'] + got['n_pos_inf'] + got['n_neg_inf'] == int(ln.sum())
    assert SU.same_hist(got, hook), 'device and host hook differ'
    assert SU.same_hist(got, stats.histogram(torch.from_numpy(SU.with_pitch(x, pitch, ln)).cuda(), dev_ln, T=T)), 'a second run differs'
    for p2, poison in ((T, 0.0), (pitch + 13, np.inf)):                    # other pitches, other poison in the gap and beyond the lengths
        assert SU.same_hist(got, stats.histogram(torch.from_numpy(SU.with_pitch(x, p2, ln, poison=poison)).cuda(), dev_ln, T=T)), (p2, poison)


def test_histogram_of_every_edge_value_without_lengths_and_of_a_channel(stats):
    from wavenet_vocoder import _ext
    e = np.random.RandomState(5).permutation(SU.edge_values()).astype(np.float32)
    x = np.resize(e, (2, 4200)).astype(np.float32)                          # every edge value, two segments per row
    got = stats.histogram(torch.from_numpy(x).cuda())
    SU.check_hist(got, SU.reference_hist(x), 'device all edges')
    assert SU.same_hist(got, _ext.TrainStats.histogram_host(x))
    other = SU.value_sets(2, 4200)['log_scales']
    both = torch.from_numpy(np.stack([x, other], 1)).cuda()                 # [B, 2, T]: a channel by pointer offset and pitch
    ln = torch.tensor([4200, 77], dtype=torch.int32, device='cuda')
    for ch, dense in ((0, x), (1, other)):
        a, b = stats.histogram(both, ln, channel=ch), stats.histogram(torch.from_numpy(dense).cuda(), ln)
        assert SU.same_hist(a, b), ch
        SU.check_hist(a, SU.reference_hist(dense, [4200, 77]), 'device channel %d' % ch)
    empty = stats.histogram(torch.full((3, 9), float('nan'), device='cuda'), torch.zeros(3, dtype=torch.int32, device='cuda'))
    assert empty['num'] == 0 and empty['min'] == 0.0 and empty['max'] == 0.0 and empty['sum'] == 0.0 and empty['n_nan'] == 0 and int(empty['bucket'].sum()) == 0


def test_histogram_shape_errors_reach_no_kernel(stats):
    from wavenet_vocoder import _ext
    for shape in ((9, 16), (2, 4201)):
        with pytest.raises(_ext.WnError) as ei:
            stats.histogram(torch.zeros(*shape, device='cuda'))
        assert ei.value.code == -2


@pytest.mark.parametrize('inside', [False, True])
def test_tensor_statistics_against_numpy_and_bit_identical_to_the_hook(stats, inside):
    from wavenet_vocoder import _ext
    flat, table = SU.tensor_table(inside=inside)
    ref, bound = SU.reference_tensors(flat, table)
    dev = torch.from_numpy(flat).cuda()
    got = stats.tensor_stats(dev)
    SU.check_tensors(got, ref, bound, 'device tensors')
    assert got.tobytes() == _ext.TrainStats.tensor_stats_host(flat, table).tobytes(), 'device and host hook differ'
    assert got.tobytes() == stats.tensor_stats(dev).tobytes(), 'a second run differs'


def _model(head):
    import hparams as H
    from wavenet_vocoder.feeder import SyntheticFeeder
    from wavenet_vocoder.models import create_model
    hp = H._build().parse(TINY + ',' + HEADS[head])
    model = create_model('WaveNet', hp)
    model.build(4, 512)
    return hp, model, SyntheticFeeder(hp, 4, 512)


def test_gradient_norms_of_a_model_against_torch_float64(tmp_path):
    """one step of the drivers test's tiny model, clipping on: every tensor's sum of squares inside the bound of torch float64 on the same slice of
    model.grads (the unclipped gradient), max |x| equal, and the scalar the loop writes is the largest norm"""
    from wavenet_vocoder import train as T
    hp, model, feeder = _model('mol')
    x, y, lengths, c, g = batch = feeder.next_train_batch()
    model.initialize(y, c, g, lengths, x=x, keep_y_hat=True)
    model.add_loss()
    step = model.add_optimizer(0)
    stats = model.train_stats()
    assert stats is model.train_stats() and stats.names == list(model.engine.layout)
    got = stats.tensor_stats(model.grads)
    grads = model.grads.double().cpu()
    norms = []
    for i, (name, (shape, off)) in enumerate(model.engine.layout.items()):
        v = grads[off:off + int(np.prod(shape))]
        want = float((v * v).sum())
        assert abs(got[i, 0] - want) <= SU.gamma(v.numel()) * want, (name, got[i, 0], want)
        assert got[i, 1] == float(v.abs().max()) and got[i, 2] == 0 and got[i, 3] == v.numel(), name
        norms.append(float(np.sqrt(got[i, 0])))
    assert max(norms) > 0
    ev = str(tmp_path)
    row = T.add_train_stats(model, batch, step, ev, hp)
    assert row['wavenet_stats/max_gradient_norm'] == max(norms) and row['wavenet_stats/max_gradient_norm_tensor'] == stats.names[int(np.argmax(norms))]
    assert row['wavenet_stats/global_gradient_norm'] == pytest.approx(float(grads.norm()), rel=1e-12)
    assert row['wavenet_stats/clipped_tensors'] == sum(n > hp.wavenet_gradient_max_norm for n in norms) and row['wavenet_stats/nonfinite_gradients'] == 0
    params = stats.tensor_stats(model.params)                              # the same call on the parameters: their norms
    assert np.all(params[:, 2] == 0) and abs(float(params[:, 0].sum()) - float((model.params.double() ** 2).sum())) <= 1e-9 * float(params[:, 0].sum())
    model.engine.close()


def _drive(root, head, on, monkeypatch):
    import hparams as H
    from wavenet_vocoder import train as T
    seen, sums = [], []

    late_cls = getattr(T._LateScalars, '_real', T._LateScalars)             # (the originals, not the wrappers of an earlier call)
    real = getattr(T.add_train_stats, '_real', T.add_train_stats)

    class Late(late_cls):
        _real = late_cls

        def pop_ready(self, keep=1):
            out = super().pop_ready(keep)
            seen.extend(out)
            return out

    def recording(model, batch, step, *a, **k):
        sums.append((step, int(batch[2].sum().item())))
        return real(model, batch, step, *a, **k)

    recording._real = real
    monkeypatch.setattr(T, '_LateScalars', Late)
    monkeypatch.setattr(T, 'add_train_stats', recording)
    hp = H._build().parse(DRIVE + ',mi355_synthetic_data=True,' + HEADS[head] + ',mi355_train_stats=%s' % on)
    log_dir = os.path.join(root, 'logs-%s' % on); os.makedirs(log_dir)
    args = types.SimpleNamespace(base_dir=root, model='WaveNet', restore=False, wavenet_train_steps=4, checkpoint_interval=100, summary_interval=2,
                                 eval_interval=100, embedding_interval=100, eval_max_time=0)
    save_dir = T.wavenet_train(args, log_dir, hp, 'no_such_map.txt')
    assert save_dir is not None, 'the driver returns None when training raised'
    sd = torch.load(os.path.join(save_dir, 'wavenet_model.ckpt-4.pt'), map_location='cpu')
    return os.path.join(log_dir, 'wavenet_events'), [(s, v[0]) for s, v in seen], sd, sums


OLD_KEYS = {'step', 'wavenet_loss', 'wavenet_learning_rate', 'wavenet_max_gradient_norm', 'audio_samples_per_sec'}


@pytest.mark.parametrize('head', ['mol', 'gaussian', 'softmax'])
def test_driver_writes_the_summaries_and_the_run_is_bit_identical_with_the_key_on_and_off(tmp_path, monkeypatch, head):
    from wavenet_vocoder import _ext
    root = str(tmp_path)
    ev_off, loss_off, sd_off, sums_off = _drive(root, head, False, monkeypatch)
    ev_on, loss_on, sd_on, sums_on = _drive(root, head, True, monkeypatch)
    # off: no new file, no call, today's keys
    assert sorted(os.listdir(ev_off)) == ['scalars.jsonl'] and sums_off == []
    rows_off = [json.loads(l) for l in open(os.path.join(ev_off, 'scalars.jsonl'))]
    assert [set(r) for r in rows_off] == [OLD_KEYS, OLD_KEYS]
    # on: the three files exist and parse
    assert sorted(os.listdir(ev_on)) == ['gradient_norms.jsonl', 'histograms.jsonl', 'scalars.jsonl'] and [s for s, _ in sums_on] == [2, 4]
    rows_on = [json.loads(l) for l in open(os.path.join(ev_on, 'scalars.jsonl'))]
    new = {'wavenet_stats/max_gradient_norm', 'wavenet_stats/max_gradient_norm_tensor', 'wavenet_stats/global_gradient_norm', 'wavenet_stats/clipped_tensors',
           'wavenet_stats/nonfinite_gradients'}
    assert [set(r) for r in rows_on] == [OLD_KEYS | new] * 2
    for r, o in zip(rows_on, rows_off):
        for k in new - {'wavenet_stats/max_gradient_norm_tensor'}:
            assert np.isfinite(r[k]), k
        assert 0 < r['wavenet_stats/max_gradient_norm'] <= r['wavenet_stats/global_gradient_norm'] and r['wavenet_stats/nonfinite_gradients'] == 0
        assert r['wavenet_max_gradient_norm'] == o['wavenet_max_gradient_norm'] and r['wavenet_loss'] == o['wavenet_loss']      # today's keys, today's values
    gn = [json.loads(l) for l in open(os.path.join(ev_on, 'gradient_norms.jsonl'))]
    assert [g['step'] for g in gn] == [2, 4] and all(len(g['names']) == len(g['norm']) == len(g['max_abs']) == len(g['nonfinite']) > 10 for g in gn)
    assert max(gn[1]['norm']) == rows_on[1]['wavenet_stats/max_gradient_norm'] and max(gn[1]['max_abs']) == pytest.approx(rows_on[1]['wavenet_max_gradient_norm'], rel=1e-6)
    hs = [json.loads(l) for l in open(os.path.join(ev_on, 'histograms.jsonl'))]
    tags = ['gradient_norm', 'wav_outputs 0', 'wav_targets 0'] + (['gaussian_means 0', 'gaussian_log_scales 0'] if head == 'gaussian' else [])
    assert [(h['step'], h['tag']) for h in hs] == [(s, t) for s in (2, 4) for t in tags]
    for h in hs:
        counts = _ext.TrainStats.decode(h)
        want = len(gn[0]['names']) if h['tag'] == 'gradient_norm' else dict(sums_on)[h['step']]
        assert h['num'] == int(counts.sum()) == want and h['n_nan'] == h['n_pos_inf'] == h['n_neg_inf'] == 0, h['tag']
        assert np.isfinite([h['min'], h['max'], h['sum'], h['sum_squares']]).all() and h['min'] <= h['max']
        if h['tag'].startswith('wav_'):
            assert -1.0 <= h['min'] and h['max'] <= 1.0, h['tag']
    # the summary does not disturb the step: losses and the final state, bit for bit
    assert [s for s, _ in loss_on] == [1, 2, 3, 4] and loss_on == loss_off, (loss_on, loss_off)
    for k in ('params', 'adam_m', 'adam_v', 'ema'):
        assert torch.equal(sd_on[k], sd_off[k]), k
    assert sd_on['global_step'] == sd_off['global_step'] == 4
