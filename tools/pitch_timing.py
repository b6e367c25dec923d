#!/usr/bin/env python3
"""Device time of the pitch check (PitchTracker.run and .compare, csrc/wn_pitch.hip) -> profiles/pitch_timing.json.

    python tools/pitch_timing.py [--repeats 30] [--out profiles/pitch_timing.json]

Cases: 1 x 5 s and 20 x 5 s pairs of 22.05 kHz at the production geometry (401 frames, lags 1 ... 368, 1024 terms each).  Per case: median and the
p05 - p95 spread over `repeats` event-bracketed calls after 3 warm-up calls, for one wn_pitch_run (one signal of the pair), for the pair's check -- two
runs and one compare into preallocated outputs -- and for PitchCheck.score as the drivers call it (with its allocations and the one copy of [B, 9] floats
to the host).  Beside a run: its (difference, fused multiply-add) pairs, B x frames x tau_max x window, and the two 4-byte LDS reads each pair takes,
divided by the time: the kernel is bound by LDS reads (csrc/wn_pitch.hip), so that rate against the chip's LDS bandwidth is what to read.  Beside
them the numpy float64 evaluation of tests/pitch_ref.py of the same pairs on this host, and the device time per utterance as a share of the synthesis
span it follows (one-shot and folded times of profiles/fold_timing.json, measured earlier on the paper model).  Nothing here is a threshold; the numbers
are one box's."""
import argparse
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

SECONDS = 5


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


def _host_path(gen, ref, geo, repeats):
    """the numpy float64 evaluation of the same pairs: both tracks and the comparison (tests/pitch_ref.py)"""
    import pitch_ref as PR
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fa, fb = [], []
        for g, r in zip(gen, ref):
            fb.append([p['f0'] for p in PR.track(g, geo)[1]])
            fa.append([p['f0'] for p in PR.track(r, geo)[1]])
        PR.compare(fa, fb, [len(f) for f in fa])
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--host-repeats', type=int, default=1)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pitch_timing.json'))
    args = ap.parse_args()
    import hparams as H
    import pitch_ref as PR
    from wavenet_vocoder import _ext
    from wavenet_vocoder.pitch import PitchCheck
    hp = H._build()
    geo = _ext.pitch_geometry(hp)
    n = SECONDS * hp.sample_rate
    F = 1 + n // geo['hop']
    fold = json.load(open(os.path.join(ROOT, 'profiles', 'fold_timing.json')))['models']['paper_5s']
    spans = {'one_shot_s': fold['one_shot']['median_s'], 'folded_20_rows_s': fold['points']['20']['median_s']}
    res = {'what': 'pitch check on an MI355X: hipEvent medians of %d calls after 3 warm-up calls; pairs of %d s signals of %d Hz, %d frames x %d lags x %d terms' % (
               args.repeats, SECONDS, hp.sample_rate, F, geo['tau_max'], geo['window']),
           'device': torch.cuda.get_device_name(0), 'geometry': geo, 'spans_of_profiles_fold_timing_json': spans, 'cases': {}}
    for B in (1, 20):
        gen = [PR.signal(geo, n, 200 + b) for b in range(B)]
        ref = [PR.signal(geo, n, 300 + b) for b in range(B)]
        g, r = torch.from_numpy(np.stack(gen)).cuda(), torch.from_numpy(np.stack(ref)).cuda()
        chk = PitchCheck(hp, B, n)
        trk = chk.tracker
        lengths, frames = [n] * B, [F] * B
        out_g = (torch.zeros(B, F, device='cuda'), torch.zeros(B, F, device='cuda'))
        out_r = (torch.zeros(B, F, device='cuda'), torch.zeros(B, F, device='cuda'))
        table = torch.zeros(B, 9, device='cuda')
        case = {'B': B, 'samples': n, 'frames': F}
        st = _events(lambda: trk.run(g, lengths, out=out_g), args.repeats)
        st['pairs'] = B * F * geo['tau_max'] * geo['window']
        st['Gpairs_per_s'] = st['pairs'] / (st['median_ms'] * 1e-3) / 1e9
        st['LDS_read_TB_per_s'] = 2 * 4 * st['pairs'] / (st['median_ms'] * 1e-3) / 1e12
        case['wn_pitch_run'] = st
        case['wn_pitch_compare'] = _events(lambda: trk.compare(out_r[0], out_g[0], frames, out=table), args.repeats)

        def pair():
            trk.run(g, lengths, out=out_g); trk.run(r, lengths, out=out_r); trk.compare(out_r[0], out_g[0], frames, out=table)

        case['run_run_compare'] = _events(pair, args.repeats)
        case['score'] = _events(lambda: chk.score(g, r, lengths), args.repeats)
        case['host_numpy_float64'] = _host_path(gen, ref, geo, args.host_repeats)
        case['host_over_device'] = case['host_numpy_float64']['median_ms'] / case['score']['median_ms']
        per_utt_ms = case['run_run_compare']['median_ms'] / B
        case['check_share_of_span'] = {k: per_utt_ms * 1e-3 / v for k, v in spans.items()}
        res['cases']['%dx%ds' % (B, SECONDS)] = case
        print(json.dumps({'case': '%dx%ds' % (B, SECONDS), **case}))
        chk.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
