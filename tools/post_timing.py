#!/usr/bin/env python3
"""Device time of the output stage (wn_post_finish / wn_post_push, csrc/wn_post.hip) -> profiles/post_timing.json.

    python tools/post_timing.py [--repeats 30] [--out profiles/post_timing.json]

Cases: wn_post_finish (float32 + int16) at 1 x 110 250 and 20 x 110 250 samples (5 s at 22.05 kHz), wn_post_push (int16) at 20 x 2 200 (one
8-frame tick of a slot session at hop 275), for the three input types, k = 0.97.  Per case: median and the p05 - p95 spread over `repeats`
event-bracketed calls after 3 warm-up calls.  Beside each: the span the call follows (one-shot, folded and slot-push times of
profiles/fold_timing.json / slots_timing.json, measured earlier on the paper model) and the call's share of it, and the host path it replaces at
the same shape, timed on this host: .cpu() of the samples + decode (numpy) + scipy lfilter + save_wavenet_wav's arithmetic.  Nothing here is a
threshold; the numbers are one box's."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tacotron-2_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

K = 0.97


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


def _host_path(dev, in_type, finish, repeats):
    """what the stage replaces: the samples to the host, the decode, lfilter (float64), the int16 arithmetic of save_wavenet_wav (finish) or a gain (push)"""
    import post_util as PU
    from scipy import signal
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a = dev.cpu().numpy()
        for row in a:
            y = signal.lfilter([1.0], [1.0, -K], PU.decode(in_type, row))
            if finish:
                PU.save_wavenet_wav_pcm(y)
            else:
                PU.pcm(y.astype(np.float32), PU.push_scale(1.0))
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def _spans():
    """seconds of the span each case follows, from the earlier profiles (paper model, 5 s utterance; 20 slots, 8-frame pushes)"""
    out = {}
    try:
        f = json.load(open(os.path.join(ROOT, 'profiles', 'fold_timing.json')))['models']['paper_5s']
        out['one_shot_5s_s'] = f['one_shot']['median_s']
        out['folded_20_rows_5s_s'] = f['points']['20']['median_s']
    except Exception as e:      # noqa: BLE001
        out['fold_timing'] = 'not read (%s)' % type(e).__name__
    try:
        s = json.load(open(os.path.join(ROOT, 'profiles', 'slots_timing.json')))['session_vs_stream']['20']['session']
        out['slot_push_20x2200_s'] = s['us_per_sample_8_frame_pushes'] * 2200 * 1e-6
    except Exception as e:      # noqa: BLE001
        out['slots_timing'] = 'not read (%s)' % type(e).__name__
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--host-repeats', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'post_timing.json'))
    args = ap.parse_args()
    assert args.repeats >= 20
    import hparams as H
    import post_util as PU
    from wavenet_vocoder import _ext
    hp = H._build()
    spans = _spans()
    res = {'what': 'output stage: hipEvent time per call (median, p05 - p95) after 3 warm-up calls; k = 0.97; one box', 'device': torch.cuda.get_device_name(0),
           'spans_it_follows': spans, 'cases': {}}
    shapes = (('finish_1x110250', True, 1, 110250, ('one_shot_5s_s', 'folded_20_rows_5s_s')), ('finish_20x110250', True, 20, 110250, ('one_shot_5s_s',)),
              ('push_20x2200', False, 20, 2200, ('slot_push_20x2200_s',)))
    for name, finish, B, n, follows in shapes:
        for in_type, tname in ((0, 'raw'), (1, 'mulaw'), (2, 'mulaw-quantize')):
            rows = np.stack([PU.samples(in_type, n, seed=b) for b in range(B)])
            dev = torch.from_numpy(rows).cuda()
            st = _ext.OutputStage(hp, B, deemphasis=K, in_type=in_type)
            y = torch.zeros(B, n, device='cuda'); q = torch.zeros(B, n, dtype=torch.int16, device='cuda')
            nn = (ctypes.c_int32 * B)(*([n] * B))
            if finish:
                fn = lambda: st.lib.wn_post_finish(st.h, _ext._ptr(dev), n, nn, B, _ext._ptr(y), _ext._ptr(q), n, None, _ext._stream())
            else:
                fn = lambda: st.lib.wn_post_push(st.h, _ext._ptr(dev), n, nn, None, B, None, _ext._ptr(q), n, None, _ext._stream())
            case = {'device': _events(fn, args.repeats), 'host_path': _host_path(dev, in_type, finish, args.host_repeats)}
            case['share_of_span'] = {k: case['device']['median_ms'] * 1e-3 / spans[k] for k in follows if isinstance(spans.get(k), float)}
            case['host_over_device'] = case['host_path']['median_ms'] / case['device']['median_ms']
            case['ns_per_sample_of_the_longest_row'] = case['device']['median_ms'] * 1e6 / n
            res['cases']['%s_%s' % (name, tname)] = case
            st.close()
            print(name, tname, json.dumps(case), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print('wrote', args.out)


if __name__ == '__main__':
    main()
