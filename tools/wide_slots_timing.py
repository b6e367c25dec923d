"""Wide slot sessions against padded wide runs (GPU): what continuous batching at 64 ... 1 024 slots delivers on a ragged list of utterances.

For every model (paper: 24 layers / 2 stacks, R = 256; hparams: hparams.py's own), list (the first --first and all lengths of
tests/golden/slot_lengths.json, a SYNTHETIC list) and width B, two arms, each in a child process of its own on an inference-only context:
  session   ONE WaveNet.wide_slots session of min(B, utterances) slots driven by slot_plan with a tick of --tick frames; the context's max_time covers
            one push (tick + lookahead frames), whatever the utterances' lengths;
  padded    WaveNet.wide(rows = B) over the same list: sorted, cut into runs of <= B, every run padded to its own longest (the baseline); the context's
            max_time covers the longest utterance.
Reported per arm: useful samples per second (samples of the utterances / time between device events around the arm, nothing counted for padding or
dummy steps), steps run and us per step (the session's per-push step against the lockstep wide step at the same width), and device memory taken
(torch.cuda.mem_get_info before the context is built minus the minimum seen until the arm ends).  Profiler off; --out writes the JSON
(profiles/wide_slots_timing.json) and keeps the entries of earlier invocations, so a session may be split with --models / --lists / --widths."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd')):
    sys.path.insert(0, p)

PAPER = ('layers=24,stacks=2,residual_channels=256,gate_channels=512,skip_out_channels=256,cin_channels=80,num_mels=80,out_channels=30,'
         'upsample_type=2D,upsample_scales=[5,5,11],hop_size=275,legacy=False,residual_legacy=False')


def _ev():
    import torch
    e = torch.cuda.Event(enable_timing=True); e.record(); return e


def _lengths(a):
    frames = [int(v) for v in json.load(open(os.path.join(ROOT, 'tests', 'golden', 'slot_lengths.json')))['frames']]
    return frames[:a.first] if a.list == 'first' else frames


def _model(a, B, T):
    import hparams as H
    import torch
    from wavenet_vocoder.models.modules import initialize_parameters
    from wavenet_vocoder.models.wavenet import WaveNet
    hp = H._build()
    if a.model == 'paper':
        hp.parse(PAPER)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    model = WaveNet(hp)
    model.build(B, T, inference_only=True)
    model.params.copy_(initialize_parameters(hp, model.engine.layout, seed=5).cuda()); model._dirty = True
    return hp, model, free0


def arm_session(a):
    import torch
    from wavenet_vocoder.models.wavenet import slot_plan
    lengths = _lengths(a)
    hop_of = lambda hp: int(np.prod(hp.upsample_scales))
    B = min(a.width, len(lengths))
    import hparams as H
    hp0 = H._build()
    if a.model == 'paper':
        hp0.parse(PAPER)
    hop = hop_of(hp0)
    hp, model, free0 = _model(a, B, (a.tick + 8) * hop)
    right = model.engine.stream_lookahead()[1]
    assert (a.tick + right) * hop <= model.max_time
    c = torch.randn(hp.cin_channels, sum(lengths), generator=torch.Generator().manual_seed(1)).cuda()
    start = np.concatenate([[0], np.cumsum(lengths)])
    sess = model.wide_slots(B, steps_per_graph=32)
    owner, sent, got, steps, pushes = [None] * B, [0] * len(lengths), 0, 0, 0
    low = torch.cuda.mem_get_info()[0]
    e0 = _ev()
    for opens, frames, final in slot_plan(lengths, B, a.tick):
        for b, u in opens:
            sess.open(b, seed=1 + u)
            owner[b] = u
        items = {}
        for b in range(B):
            u = owner[b]
            if u is None:
                continue
            items[b] = (c[:, start[u] + sent[u]:start[u] + sent[u] + frames[b]], final[b])
            sent[u] += frames[b]
        res = sess.push(items)
        n = [int(v.shape[0]) for v in res.values()]
        got += sum(n); steps += max(n); pushes += 1
        for b in items:
            if final[b]:
                owner[b] = None
        if pushes % 16 == 0:
            low = min(low, torch.cuda.mem_get_info()[0])
    e1 = _ev()
    torch.cuda.synchronize(); sess.check(); sess.close()
    low = min(low, torch.cuda.mem_get_info()[0])
    assert got == sum(lengths) * hop and model.engine.synth_path == 'graph'
    sec = e0.elapsed_time(e1) / 1e3
    model.engine.close()
    print('ARM ' + json.dumps({'slots': B, 'utterances': len(lengths), 'useful_samples': got, 'seconds': sec, 'useful_samples_per_s': got / sec, 'steps': steps, 'pushes': pushes,
                               'us_per_step': sec * 1e6 / steps, 'occupancy': got / (steps * B), 'device_bytes': int(free0 - low), 'max_time': model.max_time}))


def arm_padded(a):
    import torch
    lengths = _lengths(a)
    import hparams as H
    hp0 = H._build()
    if a.model == 'paper':
        hp0.parse(PAPER)
    hop = int(np.prod(hp0.upsample_scales))
    B = min(a.width, len(lengths))
    hp, model, free0 = _model(a, B, max(lengths) * hop)
    g = torch.Generator().manual_seed(1)
    big = torch.randn(hp.cin_channels, sum(lengths), generator=g).cuda()
    start = np.concatenate([[0], np.cumsum(lengths)])
    cl = [big[:, start[u]:start[u + 1]] for u in range(len(lengths))]
    e0 = _ev()
    samples, info = model.wide(cl, rows=a.width, check=False)
    e1 = _ev()
    torch.cuda.synchronize(); model.engine.synth_check()
    low = torch.cuda.mem_get_info()[0]
    runs = info['plan'][0]
    steps = sum(max(lengths[u] for u in r) for r in runs) * hop
    got = sum(int(s.shape[0]) for s in samples)
    assert got == sum(lengths) * hop and model.engine.synth_path == 'graph'
    sec = e0.elapsed_time(e1) / 1e3
    model.engine.close()
    print('ARM ' + json.dumps({'rows': a.width, 'runs': [len(r) for r in runs], 'utterances': len(lengths), 'useful_samples': got, 'seconds': sec, 'useful_samples_per_s': got / sec,
                               'steps': steps, 'us_per_step': sec * 1e6 / steps, 'occupancy': got / sum(len(r) * max(lengths[u] for u in r) * hop for r in runs),
                               'device_bytes': int(free0 - low), 'max_time': model.max_time}))


def _child(arm, a, model, lst, width, limit):
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--arm', arm, '--model', model, '--list', lst, '--width', str(width),
                        '--tick', str(a.tick), '--first', str(a.first)], capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith('ARM ')]
    if p.returncode != 0 or not line:
        raise RuntimeError('arm %s %s %s B=%s failed (%d): %s' % (arm, model, lst, width, p.returncode, p.stderr[-1500:]))
    return json.loads(line[-1][4:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', default=None)
    ap.add_argument('--model', default='paper')
    ap.add_argument('--list', default='first')
    ap.add_argument('--width', type=int, default=64)
    ap.add_argument('--models', default='paper,hparams')
    ap.add_argument('--lists', default='first,all')
    ap.add_argument('--widths', default='64,256,1024')
    ap.add_argument('--tick', type=int, default=8)
    ap.add_argument('--first', type=int, default=100)
    ap.add_argument('--limit', type=int, default=540, help='seconds per child')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.arm:
        return {'session': arm_session, 'padded': arm_padded}[a.arm](a)
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))
    res['method'] = ('useful samples / device-event time of the arm; every arm a child process on an inference-only context; device_bytes: free device memory before '
                     'the context minus the minimum seen; tick %d frames; lengths: tests/golden/slot_lengths.json (synthetic)' % a.tick)
    for model in a.models.split(','):
        for lst in a.lists.split(','):
            for width in [int(w) for w in a.widths.split(',')]:
                key = '%s.%s.%d' % (model, lst if lst == 'all' else 'first%d' % a.first, width)
                row = res.setdefault(key, {})
                for arm in ('session', 'padded'):
                    row[arm] = r = _child(arm, a, model, lst, width, a.limit)
                    print('%s %s: %.3f M useful samples/s, %d steps at %.1f us, occupancy %.2f, %.2f GB' % (
                        key, arm, r['useful_samples_per_s'] / 1e6, r['steps'], r['us_per_step'], r['occupancy'], r['device_bytes'] / 1e9), flush=True)
                row['session_over_padded'] = row['session']['useful_samples_per_s'] / row['padded']['useful_samples_per_s']
                row['memory_padded_over_session'] = row['padded']['device_bytes'] / max(1, row['session']['device_bytes'])
                if a.out:
                    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                    json.dump(res, open(a.out, 'w'), indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
