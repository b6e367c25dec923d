#!/usr/bin/env python3
"""Device time of a streaming-denoiser push (csrc/wn_denoise_stream.hip) -> profiles/denoise_stream_timing.json.

    python tools/denoise_stream_timing.py [--out profiles/denoise_stream_timing.json]

hipEvent medians of 30 pushes after 3 warm-ups (p05 / p95 beside them) of DenoiseStream.push with 8 mel frames (2 200 samples) per row at 1 / 20 / 64 / 256
rows in the default geometry (1024, 256), every row in steady state (each push analyses 8 or 9 new frames in ONE mostly empty 32-frame tile per row).  Beside
each: (a) SpectralDenoiser.apply on the same total samples (B rows of 2 200), and (b) the synthesis push the denoiser follows, from the recorded figures of
profiles/slots_timing.json (1 and 20 rows: the session's us per sample at 8-frame pushes) and profiles/wide_slots_timing.json (64 and 256 rows: us per step
of the wide path); the ratios are reported, no threshold is set.  The shader and memory clocks (rocm-smi --showclocks) are read right after every timed loop."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron-2_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from wavenet_vocoder import _ext      # noqa: E402
from denoise_timing import clocks     # noqa: E402

N_FFT, HOP, PUSH = 1024, 256, 2200
WIDTHS = (1, 20, 64, 256)


def events_of(fn, calls=30, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': float(np.median(ms)), 'p05_ms': float(np.percentile(ms, 5)), 'p95_ms': float(np.percentile(ms, 95)), 'calls': calls, 'clocks_after': clocks()}


def synthesis_push_ms():
    """the push of 8 frames the denoiser follows, per width, from the recorded profiles: (ms, where the figure comes from)"""
    res = {}
    try:
        s = json.load(open(os.path.join(ROOT, 'profiles', 'slots_timing.json')))['session_vs_stream']
        for B in (1, 20):
            res[B] = (s[str(B)]['session']['us_per_sample_8_frame_pushes'] * PUSH * 1e-3, 'profiles/slots_timing.json session_vs_stream/%d/session/us_per_sample_8_frame_pushes x 2200' % B)
    except Exception as e:      # noqa: BLE001
        res['slots_timing.json'] = 'not read (%s)' % type(e).__name__
    try:
        w = json.load(open(os.path.join(ROOT, 'profiles', 'wide_slots_timing.json')))['existing_paths']['wide_vs_parent']['summary']
        for B in (64, 256):
            v = w['paper_%d.us_per_step' % B]
            res[B] = (float(v.get('this_median', np.median(v['this']))) * PUSH * 1e-3, 'profiles/wide_slots_timing.json existing_paths/wide_vs_parent paper_%d.us_per_step x 2200' % B)
    except Exception as e:      # noqa: BLE001
        res['wide_slots_timing.json'] = 'not read (%s)' % type(e).__name__
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'denoise_stream_timing.json'))
    args = ap.parse_args()
    res = {'what': 'tools/denoise_stream_timing.py: hipEvent medians of 30 pushes after 3 warm-ups, geometry (1024, 256), pushes of 8 mel frames = 2200 samples per row, rows in steady '
                   'state; clocks_after: rocm-smi --showclocks right after the timed loop of the case',
           'device': torch.cuda.get_device_name(0), 'cases': {},
           'not_measured': ['the synthesis push itself (the figures of profiles/slots_timing.json and profiles/wide_slots_timing.json are taken as recorded, paper model)',
                            'pushes that end or restart rows (the final push analyses up to ceil(n_fft / hop) / 2 + 1 more frames per row)',
                            'in_type 1 / 2 (the decode while staging)', 'geometries other than (1024, 256)', 'packing frames of several rows into one tile (not built)',
                            'the denoiser running beside the next synthesis push on another stream']}
    synth = synthesis_push_ms()
    rs = np.random.RandomState(0)
    for B in WIDTHS:
        x = torch.from_numpy((0.1 * rs.randn(B, PUSH)).astype(np.float32)).cuda()
        d = _ext.SpectralDenoiser(N_FFT, HOP, B, PUSH)
        d.fit(x, [PUSH] * B)
        ds = _ext.DenoiseStream(N_FFT, HOP, B, PUSH)
        ds.take_profile(d)
        out = torch.empty(B, PUSH + N_FFT, device='cuda')
        whole = torch.empty_like(x)
        ds.push(x, restart=True, strength=1.0, out=out)
        case = {'rows': B, 'samples_per_row': PUSH,
                'stream_push': events_of(lambda: ds.push(x, strength=1.0, out=out)),
                'one_shot_run_same_samples': events_of(lambda: d.apply(x, [PUSH] * B, 1.0, out=whole))}
        case['stream_over_one_shot'] = case['stream_push']['median_ms'] / case['one_shot_run_same_samples']['median_ms']
        if B in synth:
            case['synthesis_push_ms'], case['synthesis_push_source'] = synth[B]
            case['stream_share_of_synthesis_push'] = case['stream_push']['median_ms'] / case['synthesis_push_ms']
        res['cases']['%d rows' % B] = case
        ds.close(); d.close()
    res['synthesis_figures_not_read'] = {k: v for k, v in synth.items() if isinstance(k, str)}
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res['cases'], indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
