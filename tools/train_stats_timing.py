#!/usr/bin/env python3
"""Device time of one training-summary pass (csrc/wn_stats.hip) at the benchmark's C2 shape -> profiles/train_stats_timing.json.

    python tools/train_stats_timing.py [--repeats 30] [--out profiles/train_stats_timing.json] [--bench parent1.json branch1.json ...]

The pass of a summary step: the per-tensor statistics of the flat gradient buffer (13.7 M floats in the C2 layout, one read) and the histograms of
[8, 11000] signals -- two for the mixture-of-logistics and softmax heads (outputs, targets), four for the Gaussian head (plus means and log-scales as
channels of y_hat [8, 2, 11000]).  Per piece and for the whole pass: median and the p05 - p95 spread over `repeats` event-bracketed calls after 3 warm-up
calls, through the Python surface (TrainStats.tensor_stats / .histogram: the launches AND the copy of the result to the host, as the training loop calls
them) and for the launches alone (the C entry points, results left on the device).  Beside them what the loop did before at the same place,
``grads.abs().max().item()``, on the same buffer in the same process.  --bench: result lines of bench.py runs (the parent commit and this build,
alternating, taken in the same session) are copied in, with the spread between the parent's own runs.  Nothing here is a threshold; the numbers are one
box's."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tacotron-2_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

B, T = 8, 11000


def _stats(ms):
    s = sorted(ms)
    p = lambda q: s[min(len(s) - 1, int(round(q * (len(s) - 1))))]
    return {'median_ms': statistics.median(ms), 'p05_ms': p(0.05), 'p95_ms': p(0.95), 'calls': len(ms)}


def _events(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_stats_timing.json'))
    ap.add_argument('--bench', nargs='*', default=[], help='files of bench.py result lines; the file name (without .json) names the run')
    args = ap.parse_args()
    import hparams as base
    import paper_hparams as paper
    from wavenet_vocoder import _ext
    hp = base._build(dict(paper.PAPER_OVERRIDES, stacks=2))
    eng = _ext.Engine(hp, B, T)
    layout, n_params = eng.layout, eng.n_params
    eng.close()
    stats = _ext.TrainStats(B, T, layout)
    g = torch.Generator(device='cuda').manual_seed(0)
    grads = torch.randn(n_params, device='cuda', generator=g) * 1e-3
    y_hat = torch.randn(B, 2, T, device='cuda', generator=g)
    out, tgt = torch.tanh(torch.randn(B, T, device='cuda', generator=g)), torch.tanh(torch.randn(B, T, device='cuda', generator=g))
    ln = torch.full((B,), T, dtype=torch.int32, device='cuda')
    lib, h = stats.lib, stats.h
    st = _ext._stream
    ptr = _ext._ptr

    def raw_hist(x, off=0, pitch=T):
        assert lib.wn_stats_histogram(h, ctypes.c_void_p(x.data_ptr() + 4 * off), pitch, ptr(ln), B, T, ptr(stats._bucket), ptr(stats._summary), st()) == 0

    def raw_tensors():
        assert lib.wn_stats_tensors(h, ptr(grads), ptr(stats._tout), st()) == 0

    def pass_surface(gaussian):
        stats.tensor_stats(grads); stats.histogram(out, ln); stats.histogram(tgt, ln)
        if gaussian:
            stats.histogram(y_hat, ln, channel=0); stats.histogram(y_hat, ln, channel=1)

    def pass_launches(gaussian):
        raw_tensors(); raw_hist(out); raw_hist(tgt)
        if gaussian:
            raw_hist(y_hat, 0, 2 * T); raw_hist(y_hat, T, 2 * T)

    r = args.repeats
    res = {'what': 'training-summary pass on an MI355X at C2 (gradient buffer of %d floats in %d tensors, histograms of %d x %d): hipEvent medians of %d calls after 3 '
                   'warm-up calls' % (n_params, len(layout), B, T, r),
           'device': torch.cuda.get_device_name(0),
           'bytes_read': {'tensor_stats': 4 * n_params, 'histogram': 4 * B * T},
           'launches': {'tensor_stats': 2, 'histogram': 2},
           'surface_with_host_copy': {
               'tensor_stats': _events(lambda: stats.tensor_stats(grads), r),
               'histogram': _events(lambda: stats.histogram(out, ln), r),
               'pass_2_histograms': _events(lambda: pass_surface(False), r),
               'pass_4_histograms': _events(lambda: pass_surface(True), r)},
           'launches_alone': {
               'tensor_stats': _events(raw_tensors, r),
               'histogram': _events(lambda: raw_hist(out), r),
               'histogram_channel_view': _events(lambda: raw_hist(y_hat, T, 2 * T), r),
               'pass_2_histograms': _events(lambda: pass_launches(False), r),
               'pass_4_histograms': _events(lambda: pass_launches(True), r)},
           'parent_grads_abs_max_item': _events(lambda: float(grads.abs().max().item()), r)}
    ts = res['launches_alone']['tensor_stats']
    ts['GB_per_s'] = 4 * n_params / (ts['median_ms'] * 1e-3) / 1e9
    hs = res['launches_alone']['histogram']
    hs['GB_per_s'] = 4 * B * T / (hs['median_ms'] * 1e-3) / 1e9
    # the pass is right while it is timed: the host hook gives the same bits on the same data
    a, b = stats.histogram(out, ln), _ext.TrainStats.histogram_host(out.cpu().numpy(), ln.cpu().numpy())
    res['bits_equal_to_host_hook'] = bool(np.array_equal(a['bucket'], b['bucket']) and a['sum'] == b['sum'] and a['sum_squares'] == b['sum_squares'])
    if args.bench:
        runs = {}
        for path in args.bench:
            lines = [json.loads(l) for l in open(path) if l.strip().startswith('{')]
            d = lines[-1]
            runs[os.path.splitext(os.path.basename(path))[0]] = {'value': d['value'], 'ms_per_step': d['ms_per_step'], 'steps': d['steps'], 'warmup': d['warmup'],
                                                                  'final_loss': d.get('final_loss')}
        res['bench_headline'] = {'metric': 'wavenet_train_audio_samples_per_sec (bench.py --gpus 1, C2), runs alternated in one session', 'runs': runs}
        par = [v['value'] for k, v in runs.items() if k.startswith('parent')]
        br = [v['value'] for k, v in runs.items() if k.startswith('branch')]
        if len(par) >= 2 and br:
            spread = (max(par) - min(par)) / statistics.mean(par)
            diff = (statistics.mean(br) - statistics.mean(par)) / statistics.mean(par)
            res['bench_headline'].update({'parent_spread_rel': spread, 'branch_minus_parent_rel': diff, 'inside_parent_spread': bool(abs(diff) <= spread)})
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    stats.close()


if __name__ == '__main__':
    main()
