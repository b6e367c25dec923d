#!/usr/bin/env python3
"""Device time of the reconstruction check (ReconstructionCheck.score and wn_melcmp_run alone, csrc/wn_melcmp.hip) -> profiles/melcmp_timing.json.

    python tools/melcmp_timing.py [--repeats 30] [--out profiles/melcmp_timing.json]

Cases: 1 x 5 s and 20 x 5 s of 22.05 kHz under hparams.py's analysis (400 frames of 80 mels per utterance).  Per case: median and the p05 - p95 spread
over `repeats` event-bracketed calls after 3 warm-up calls, for score() (analysis, comparison and the one copy of [B, 9] floats to the host) and for
wn_melcmp_run alone, without and with per_frame; beside the latter the bytes the call must move -- two reads of a and b, 2 x 2 x B x F x M x 4 -- divided
by its time.  Beside them the host path the check replaces at the same shape, timed on this host in this session: .cpu() of the samples +
datasets.audio.melspectrogram in float64 per utterance + the numpy distances of tests/melcmp_util.py; and the device time as a share of the synthesis
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


def _host_path(wav, lengths, c, frames, hp, unit_db, alarm_db, repeats):
    """what the check replaces: the samples to the host, the float64 numpy analysis per utterance, the numpy distances"""
    import melcmp_util as MU
    from datasets import audio
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = wav.cpu().numpy()
        cn = c.cpu().numpy()
        for b, n in enumerate(lengths):
            a = audio.melspectrogram(audio.preemphasis(x[b, :n].astype(np.float64), hp.preemphasis, hp.preemphasize), hp)
            MU.reference(a[None], cn[b:b + 1], [frames[b]], 13, unit_db, alarm_db)
        ms.append((time.perf_counter() - t0) * 1e3)
    return _stats(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=30)
    ap.add_argument('--host-repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'melcmp_timing.json'))
    args = ap.parse_args()
    import hparams as H
    from datasets.audio import get_hop_size
    from wavenet_vocoder.reconstruction import ReconstructionCheck
    hp = H._build()
    hop, M = get_hop_size(hp), int(hp.num_mels)
    Tc = SECONDS * hp.sample_rate // hop
    n = Tc * hop
    fold = json.load(open(os.path.join(ROOT, 'profiles', 'fold_timing.json')))['models']['paper_5s']
    spans = {'one_shot_s': fold['one_shot']['median_s'], 'folded_20_rows_s': fold['points']['20']['median_s']}
    res = {'what': 'reconstruction check on an MI355X: hipEvent medians of %d calls after 3 warm-up calls; %d s utterances of %d Hz, %d frames x %d mels' % (
               args.repeats, SECONDS, hp.sample_rate, Tc, M),
           'device': torch.cuda.get_device_name(0), 'spans_of_profiles_fold_timing_json': spans, 'cases': {}}
    rng = np.random.RandomState(0)
    for B in (1, 20):
        chk = ReconstructionCheck(hp, B, n)
        wav = torch.from_numpy((0.1 * rng.randn(B, n)).astype(np.float32)).cuda()
        lengths, frames = [n] * B, [Tc] * B
        c = torch.from_numpy(rng.uniform(-4, 4, size=(B, M, Tc)).astype(np.float32)).cuda()
        a = chk.analyzer.run(wav, lengths, channels_first=True)
        case = {'B': B, 'samples': n, 'frames': Tc}
        case['score'] = _events(lambda: chk.score(wav, lengths, c), args.repeats)
        case['analysis_alone'] = _events(lambda: chk.analyzer.run(wav, lengths, channels_first=True), args.repeats)
        for key, pf in (('wn_melcmp_run', False), ('wn_melcmp_run_per_frame', True)):
            st = _events(lambda: chk.compare.run(a, c, frames, per_frame=pf), args.repeats)      # (with the binding's three output allocations, as score() calls it)
            st['bytes_moved'] = 2 * 2 * B * Tc * M * 4
            st['GB_per_s'] = st['bytes_moved'] / (st['median_ms'] * 1e-3) / 1e9
            case[key] = st
        case['host_path'] = _host_path(wav, lengths, c, frames, hp, chk.unit_db, chk.alarm_db, args.host_repeats)
        case['host_over_device'] = case['host_path']['median_ms'] / case['score']['median_ms']
        per_utt_ms = case['score']['median_ms'] / B
        case['score_share_of_span'] = {k: per_utt_ms * 1e-3 / v for k, v in spans.items()}
        res['cases']['%dx%ds' % (B, SECONDS)] = case
        print(json.dumps({'case': '%dx%ds' % (B, SECONDS), **{k: v for k, v in case.items()}}))
        chk.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
