#!/usr/bin/env python3
"""Device time and parity of the sample-rate conversion (csrc/wn_resample.hip) -> profiles/resample_timing.json, profiles/resample_parity.json.

    python tools/resample_timing.py [--out profiles/resample_timing.json] [--parity profiles/resample_parity.json]

Timing: hipEvent medians of 30 calls after 3 warm-ups (p05 / p95 beside them) of Resampler.run on 1 x 5 s and 20 x 5 s at 48 000 -> 22 050 and at
22 050 -> 8 000, and of Resampler.push on 20 rows of 2 200 samples (8 mel frames) at 22 050 -> 8 000 in steady state.  Beside each the host path it
replaces: .cpu(), scipy.signal.upfirdn in float64 with the same filter, wall clock, median of 3.  The shader and memory clocks (rocm-smi --showclocks) are
read right after every timed loop.  No time is fixed in advance: the shares of the 0.332 s folded span (profiles/fold_timing.json) and of the 102 ms slot push
(profiles/slots_timing.json) are reported as measured.
Parity: for every configuration of tests/test_hip_resample.py the worst |device - float64| over the bound of a T-term float32 fmaf chain, and whether the
device equals the host hook bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tacotron-2_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from wavenet_vocoder import _ext      # noqa: E402
from denoise_timing import clocks     # noqa: E402
import resample_ref as R              # noqa: E402

FOLDED_SPAN_MS, SLOT_PUSH_MS = 332.0, 102.0
SMALL = [(3, 2, 4), (2, 3, 4), (2, 1, 4), (1, 2, 4), (7, 5, 3), (5, 7, 3), (320, 147, 4), (147, 320, 4)]      # (sr_in, sr_out, Z)


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


def host_path_ms(x_dev, sr_in, sr_out, reps=3):
    """what the device call replaces: the rows to the host, scipy.signal.upfirdn in float64 row by row (tests/resample_ref.py's construction)"""
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        x = x_dev.cpu().numpy()
        for row in x:
            R.upfirdn_reference(row, sr_in, sr_out)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def timing():
    res = {}
    rng = np.random.RandomState(0)
    for sr_in, sr_out in ((48000, 22050), (22050, 8000)):
        for B in (1, 20):
            n = 5 * sr_in
            x = torch.from_numpy((0.1 * rng.randn(B, n)).astype(np.float32)).cuda()
            rs = _ext.Resampler(sr_in, sr_out, B, n)
            out = torch.empty(B, rs.num_out(n), device='cuda')
            case = {'rows': B, 'samples_per_row': n, 'outputs_per_row': rs.num_out(n), 'taps': 2 * rs.W, 'table_floats': rs.L * 2 * rs.W,
                    'run': events_of(lambda: rs.run(x, out=out)), 'host_upfirdn_float64_ms': host_path_ms(x, sr_in, sr_out)}
            case['gfma_per_s'] = B * rs.num_out(n) * 2 * rs.W / case['run']['median_ms'] * 1e-6
            case['share_of_folded_span_0.332_s'] = case['run']['median_ms'] / FOLDED_SPAN_MS
            case['host_over_device'] = case['host_upfirdn_float64_ms'] / case['run']['median_ms']
            res['run %d x 5 s %d -> %d' % (B, sr_in, sr_out)] = case
            rs.close()
    B, n, sr_in, sr_out = 20, 2200, 22050, 8000
    x = torch.from_numpy((0.1 * rng.randn(B, n)).astype(np.float32)).cuda()
    rs = _ext.Resampler(sr_in, sr_out, B, n)
    out = torch.empty(B, rs.num_out(n + 2 * rs.W) + 1, device='cuda')
    rs.push(x, restart=True, out=out)
    case = {'rows': B, 'samples_per_row': n, 'taps': 2 * rs.W, 'push': events_of(lambda: rs.push(x, out=out)), 'host_upfirdn_float64_ms': host_path_ms(x, sr_in, sr_out)}
    case['share_of_slot_push_102_ms'] = case['push']['median_ms'] / SLOT_PUSH_MS
    case['host_over_device'] = case['host_upfirdn_float64_ms'] / case['push']['median_ms']
    res['push %d x %d %d -> %d' % (B, n, sr_in, sr_out)] = case
    rs.close()
    return res


def parity():
    res = {}
    rng = np.random.default_rng(1)
    for sr_in, sr_out, Z, n in [c + (None,) for c in SMALL] + [(48000, 22050, 64, 4800), (22050, 8000, 64, 2205)]:
        L, M, W, T = R.plan(sr_in, sr_out, Z)
        n = n or 3 * W + 2100
        x = rng.standard_normal(n).astype(np.float32)
        rs = _ext.Resampler(sr_in, sr_out, 1, n, zeros=Z)
        y, n_out = rs.run(torch.from_numpy(x[None]).cuda())
        y = y.cpu().numpy()[0, :n_out[0]]
        host = _ext.resample_rows_host([x], sr_in, sr_out, Z)[0]
        ref, bs = R.polyphase(x, sr_in, sr_out, Z, return_bound_sum=True)
        bound = R.bound32(bs, T)
        res['%d -> %d, Z = %d, n = %d' % (sr_in, sr_out, Z, n)] = {
            'taps': T, 'worst_abs_error': float(np.abs(y - ref).max()), 'worst_error_over_bound': float((np.abs(y - ref) / np.maximum(bound, 1e-300)).max()),
            'device_equals_host_hook_bit_for_bit': bool(np.array_equal(y.view(np.int32), host.view(np.int32)))}
        rs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_timing.json'))
    ap.add_argument('--parity', default=os.path.join(ROOT, 'profiles', 'resample_parity.json'))
    args = ap.parse_args()
    par = {'what': 'tools/resample_timing.py: Resampler.run on unit-variance noise against tests/resample_ref.py (float64); bound = 1.01 (T + 2) 2^-24 sum_j |c_j x_j| per output',
           'device': torch.cuda.get_device_name(0), 'cases': parity()}
    with open(args.parity, 'w') as f:
        json.dump(par, f, indent=1, sort_keys=True)
    res = {'what': 'tools/resample_timing.py: hipEvent medians of 30 calls after 3 warm-ups; host_upfirdn_float64_ms: .cpu() + scipy.signal.upfirdn in float64 per row, wall clock, '
                   'median of 3; clocks_after: rocm-smi --showclocks right after the timed loop of the case',
           'device': torch.cuda.get_device_name(0), 'cases': timing(),
           'not_measured': ['the conversion beside the next synthesis push on another stream', 'pushes that end or restart rows', 'rates other than the two pairs',
                            'the first call of a handle (the table of up to a few hundred KB is then read from HBM, not from L2)']}
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps({'timing': res['cases'], 'parity': par['cases']}, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
