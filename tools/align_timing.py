#!/usr/bin/env python3
"""Device time of the alignment check (Aligner.run, csrc/wn_align.hip, and AlignmentCheck.score) -> profiles/align_timing.json.

    python tools/align_timing.py [--repeats 30] [--no-host] [--out profiles/align_timing.json]

Cases: 1 x (400, 430), 20 x (400, 430) and 1 x (2000, 2100) frames of 80 mels, 13 coefficients, each with band = 0 and with band = 1.  Per case: median and the
p05 - p95 spread over `repeats` event-bracketed calls after 3 warm-up calls, for one wn_align_run into preallocated outputs (all four launches), for the
recurrence and back-trace alone (wn_test_align_dp on the handle's own cost matrix) and -- the back-trace is one lane following pointers -- for the same on a
matrix of ONE row of the same width, whose recurrence is 64 times shorter while its back-trace has as many column steps: the split the record states.  Beside
them the cells per second of the recurrence, the float64 numpy reference of tests/align_ref.py on this host (the Python double loop the module replaces) and,
for the first two cases, AlignmentCheck.score as the drivers call it on signals of as many frames (analysis, alignment, two F0 tracks, the comparison, one copy
to the host).  The shader clock is read after each loop.  Nothing here is a threshold; the numbers are one box's."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tacotron-2_amd'), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

CASES = [(1, 400, 430), (20, 400, 430), (1, 2000, 2100)]
M, K = 80, 13


def clocks():
    try:
        r = subprocess.run(['rocm-smi', '--showclocks'], capture_output=True, text=True, timeout=30)
        return [l.strip() for l in r.stdout.splitlines() if 'sclk' in l or 'mclk' in l][:4]
    except Exception as e:      # noqa: BLE001
        return 'not read (%s)' % type(e).__name__


def _stats(ms):
    s = sorted(ms)
    p = lambda q: s[min(len(s) - 1, int(round(q * (len(s) - 1))))]
    return {'median_ms': statistics.median(ms), 'p05_ms': p(0.05), 'p95_ms': p(0.95), 'calls': len(ms)}


def events(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    st = _stats(ms)
    st['clocks_after'] = clocks()
    return st


def mels(B, Fa, Fb, seed):
    rng = np.random.RandomState(seed)
    a, b = np.zeros((B, M, Fa), np.float32), np.zeros((B, M, Fb), np.float32)
    for r in range(B):
        x = np.cumsum(rng.randn(Fa, M), axis=0).astype(np.float32) * 0.3
        pos = np.clip(np.round(np.linspace(0, Fa - 1, Fb) + 6.0 * np.sin(np.arange(Fb) / 40.0)).astype(int), 0, Fa - 1)
        a[r], b[r] = x.T, (x[pos] + 0.1 * rng.randn(Fb, M).astype(np.float32)).T
    return a, b


def host_reference(a, b, band):
    """the float64 numpy evaluation of row 0: cepstra, cost matrix, the double loop of the recurrence, the back-trace"""
    import align_ref as R
    t0 = time.perf_counter()
    ca, cb = R.cepstra(a[0].T, 1.0, K)[0], R.cepstra(b[0].T, 1.0, K)[0]
    cost = R.cost_matrix(ca, cb)[0]
    dm = R.recurrence(cost, band)
    path = R.backtrace(dm, band)
    return {'ms_per_pair': (time.perf_counter() - t0) * 1e3, 'n_path': len(path), 'mcd_dtw': R.path_cost(path, cost) / len(path)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--no-host', action='store_true', help='leave the float64 host reference out (seconds to minutes per case)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'align_timing.json'))
    args = ap.parse_args()
    import hparams as H
    from wavenet_vocoder import _ext
    from wavenet_vocoder.alignment import AlignmentCheck
    hp = H._build()
    hop = int(hp.hop_size)
    res = {'what': 'alignment check on an MI355X: hipEvent medians of %d calls after 3 warm-up calls; %d mels, %d cepstral coefficients' % (args.repeats, M, K),
           'device': torch.cuda.get_device_name(0), 'cases': {}}
    for B, Fa, Fb in CASES:
        a, b = mels(B, Fa, Fb, 7)
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        for band in (0, 1):
            al = _ext.Aligner(M, B, Fa, Fb, n_cep=K, band=band)
            out = al.run(da, db, [Fa] * B, [Fb] * B)
            case = {'B': B, 'frames_a': Fa, 'frames_b': Fb, 'band': band, 'cells': B * Fa * Fb}
            st = events(lambda: al.run(da, db, [Fa] * B, [Fb] * B, out=out), args.repeats)
            st['Mcells_per_s'] = case['cells'] / (st['median_ms'] * 1e-3) / 1e6
            case['wn_align_run'] = st
            cost = torch.from_numpy(al.copy_stage('cost')).cuda()
            case['recurrence_and_backtrace'] = events(lambda: al.run_dp(cost, [Fa] * B, [Fb] * B, out=out), args.repeats)
            case['one_row_recurrence_and_backtrace'] = events(lambda: al.run_dp(cost, [1] * B, [Fb] * B, out=out), args.repeats)
            torch.cuda.synchronize()
            case['mcd_dtw_row0'] = float(al.run(da, db, [Fa] * B, [Fb] * B)['summary'][0, 4])
            if not args.no_host:
                case['host_numpy_float64'] = host_reference(a, b, band)
                case['host_over_device_per_pair'] = case['host_numpy_float64']['ms_per_pair'] / (st['median_ms'] / B)
            al.close()
            if band == 0 and Fa <= 430:
                ng, nr = (Fb - 1) * hop, (Fa - 1) * hop
                rng = np.random.RandomState(3)
                g, r = torch.from_numpy(0.1 * rng.randn(B, ng).astype(np.float32)).cuda(), torch.from_numpy(0.1 * rng.randn(B, nr).astype(np.float32)).cuda()
                chk = AlignmentCheck(hp, B, max(ng, nr), band=0)
                case['score'] = events(lambda: chk.score(g, [ng] * B, r, [nr] * B), args.repeats)
                chk.close()
            name = '%dx(%d,%d)_band%d' % (B, Fa, Fb, band)
            res['cases'][name] = case
            print(json.dumps({'case': name, **case}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
