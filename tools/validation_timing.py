#!/usr/bin/env python3
"""Timing of the validation pass on the C2 training workload (24 layers, R256 / G512 / S256, dropout 0.05; B = 8 x 11 000, resident
synthetic batch), device events:

  * wn_eval_fwd against wn_train_fwd (forward + loss) on the SAME context in one process, alternating the two, >= 50 timed calls each after
    warming both: medians and the spread of each;
  * a full WaveNet.validate over 64 utterances (8 batches), host loop and the final device-to-host copy included;
  * for comparison, eval_step's teacher-forced incremental run on one crop of the same batch;
  * wn_score alone against wn_loss at the same shape.

    python tools/validation_timing.py [--calls 60] [--out profiles/validation_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def spread(ms):
    q = statistics.quantiles(ms, n=20)
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'p05_ms': q[0], 'p95_ms': q[-1], 'spread_p95_minus_p05_ms': q[-1] - q[0],
            'calls': len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); fn(); b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=60)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'validation_timing.json'))
    args = ap.parse_args()
    import bench
    from wavenet_vocoder.feeder import SyntheticFeeder
    from wavenet_vocoder.models import create_model
    hp, B, T = bench.build_hparams('c2')
    torch.cuda.set_device(0)
    model = create_model('WaveNet', hp)
    feeder = SyntheticFeeder(hp, B, T)
    T = feeder.T
    model.build(B, T)
    model._ensure_packed()
    eng = model.engine
    x, y, lengths, c, _ = feeder.next_train_batch()
    loss = torch.zeros(1, device='cuda'); stats = torch.empty(B, 3, device='cuda'); nll = torch.empty(B, T, device='cuda')
    y_hat = torch.empty(B, hp.out_channels, T, device='cuda')
    train = lambda i: eng.train_fwd(x, c, y, lengths, 1000 + i, loss)
    evalf = lambda i: eng.eval_fwd(x, c, y, lengths, stats)
    for i in range(args.warmup):
        train(i); evalf(i)
    torch.cuda.synchronize()
    ev = {'train_fwd': [], 'eval_fwd': []}
    for i in range(args.calls):          # alternating: both see the same clocks and the same neighbours
        ev['train_fwd'].append(timed(lambda: train(i)))
        ev['eval_fwd'].append(timed(lambda: evalf(i)))
    torch.cuda.synchronize()
    res = {k: spread([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    res['eval_minus_train_median_ms'] = res['eval_fwd']['median_ms'] - res['train_fwd']['median_ms']
    res['eval_within_train_spread'] = res['eval_minus_train_median_ms'] <= res['train_fwd']['spread_p95_minus_p05_ms']
    # wn_score alone against wn_loss on the same y_hat
    eng.train_fwd(x, c, y, lengths, 1, loss, y_hat)
    ev = {'wn_loss': [], 'wn_score': [], 'wn_score_with_nll': []}
    for i in range(args.warmup + args.calls):
        a = timed(lambda: eng.loss(y_hat, y, lengths, 1, loss))
        b = timed(lambda: eng.score(y_hat, y, lengths, 1, stats))
        d = timed(lambda: eng.score(y_hat, y, lengths, 1, stats, nll))
        if i >= args.warmup:
            ev['wn_loss'].append(a); ev['wn_score'].append(b); ev['wn_score_with_nll'].append(d)
    torch.cuda.synchronize()
    res.update({k: spread([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()})
    # a whole validation pass: 64 utterances in 8 batches, host loop + the one device-to-host copy
    batches = [feeder.next_train_batch() for _ in range(8)]
    model.validate(batches[:2])
    torch.cuda.synchronize()
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        out = model.validate(batches)
        wall.append((time.perf_counter() - t0) * 1e3)
    res['validate_64_utterances'] = {'wall_ms_median': statistics.median(wall), 'wall_ms_all': wall, 'utterances': len(out['utterances']), 'samples': out['count'],
                                     'loss': out['loss']}
    # eval_step's way: item 0 of one batch, teacher forced through the incremental loop (wavenet.py:342-405)
    model.initialize(y, c, None, lengths)          # (first call: builds the synthesis state)
    torch.cuda.synchronize()
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        model.initialize(y, c, None, lengths)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res['eval_step_incremental_one_crop'] = {'wall_ms_median': statistics.median(wall), 'wall_ms_all': wall, 'samples': int(lengths[0]) // hp.hop_size * hp.hop_size,
                                             'loss': float(model.eval_loss.item())}
    res['workload'] = 'C2: %d layers / %d stacks, R%d G%d S%d, dropout %.2f, B = %d x T = %d' % (hp.layers, hp.stacks, hp.residual_channels, hp.gate_channels,
                                                                                               hp.skip_out_channels, hp.wavenet_dropout, B, T)
    res['device'] = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
