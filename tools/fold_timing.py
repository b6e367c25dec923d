"""Folded-synthesis timing (GPU, one process): wall time of ONE utterance of --seconds (5 and 20) through wn_synthesize_folded at --rows rows, next to
the one-shot wn_synthesize of the same utterance in the same session (the parent's path, which folding does not touch) and next to the prediction
n_max x (per-sample cost at that many slots) from profiles/slots_timing.json.  Models: 'paper' (24 layers, R = S = 256, pipeline), 'hparams' (hparams.py's
model, pipeline on several instances), 'c5' (BASELINE configs[4]'s widths R = S = 512: the launch-per-layer path).  Every point is the median of --runs
device-event timings after a warm-up, with the p95 - p05 spread; a point whose single run exceeds --long-s is run --long-runs times and says so in its
`runs` field.  Device time of the whole-utterance upsample, the fold kernel and the unfold kernel comes from the library's own events
(wn_test_fold_times).  One JSON line; --out writes it to a file (profiles/fold_timing.json) after every point.  No pass / fail threshold."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd')):
    sys.path.insert(0, p)

MODELS = {
    'paper': ('layers=24,stacks=2,residual_channels=256,gate_channels=512,skip_out_channels=256,cin_channels=80,num_mels=80,out_channels=30,'
              'upsample_type=2D,upsample_scales=[5,5,11],hop_size=275,legacy=False,residual_legacy=False'),
    'hparams': '',
    'c5': ('out_channels=2,residual_channels=512,gate_channels=1024,skip_out_channels=512,layers=30,stacks=3,legacy=True,residual_legacy=True,'
           'upsample_type=SubPixel,upsample_scales=[15,20],hop_size=300,sample_rate=24000,cdf_loss=False'),
}


def _ev():
    import torch
    e = torch.cuda.Event(enable_timing=True); e.record(); return e


def _stats(v):
    v = np.asarray(v, float)
    return {'median_s': float(np.median(v)), 'spread_p95_p05_s': float(np.percentile(v, 95) - np.percentile(v, 5)), 'runs': int(v.size), 'all_s': [float(x) for x in v]}


def _predicted_us(slots_timing, rows):
    """per-sample cost at `rows` slots from profiles/slots_timing.json (paper model: sessions of 1, 8, 12, 20 slots; linear between, the last slope beyond)"""
    pts = sorted((int(k), v['session']['us_per_sample_8_frame_pushes']) for k, v in slots_timing['session_vs_stream'].items())
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    if rows <= xs[-1]:
        return float(np.interp(rows, xs, ys)), 'interpolated between measured slot counts %s' % xs
    slope = (ys[-1] - ys[-2]) / (xs[-1] - xs[-2])
    return float(ys[-1] + slope * (rows - xs[-1])), 'EXTRAPOLATED beyond %d slots with the last measured slope' % xs[-1]


def _timed(fn, runs, long_s, long_runs):
    import torch
    out = []
    n = runs
    while len(out) < n:
        e0 = _ev(); fn(); e1 = _ev(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / 1e3)
        if len(out) == 1 and out[0] > long_s:
            n = long_runs
    return out


def measure(a, name, res, flush):
    import torch
    import hparams as H
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.modules import initialize_parameters
    hp = H._build()
    if MODELS[name]:
        hp.parse(MODELS[name])
    hop = int(np.prod(hp.upsample_scales))
    rows_list = [int(r) for r in a.rows.split(',')]
    slots_timing = json.load(open(os.path.join(ROOT, 'profiles', 'slots_timing.json')))
    lib = _ext.load_library()
    for seconds in [float(s) for s in a.seconds.split(',')]:
        F = int(round(seconds * hp.sample_rate / hop))
        T = F * hop
        eng = _ext.Engine(hp, max(rows_list), T, inference_only=True)
        eng.pack_weights(initialize_parameters(hp, eng.layout, seed=5).cuda())
        c = torch.randn(1, hp.cin_channels, F, generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty(1, T, device='cuda')
        wav = torch.empty(1, T, device='cuda')
        key = '%s_%gs' % (name, seconds)
        entry = {'frames': F, 'samples': T, 'hop': hop, 'warm': a.warm, 'fade': a.fade, 'min_keep': a.min_keep, 'points': {}}
        res['models'][key] = entry
        # warm-up of both paths at a short length (code objects, the pipeline's weight images, the step graphs)
        eng.synthesize(c[:, :, :8].contiguous(), None, out[:, :8 * hop].contiguous(), seed=1)
        eng.synthesize_folded(c[:, :, :32].contiguous(), [32], _ext.fold_plan([32], 2, 2, 1, 4), wav[:, :32 * hop].contiguous(), seed=1)
        torch.cuda.synchronize(); eng.synth_check()
        if not a.no_one_shot:
            entry['one_shot'] = dict(_stats(_timed(lambda: eng.synthesize(c, None, out, seed=1), a.runs, a.long_s, a.long_runs)), path=eng.synth_path)
            eng.synth_check(); flush()
        assert lib.wn_test_fold_timing(eng.h, 1) == 0
        for rows in rows_list:
            plan = _ext.fold_plan([F], rows, a.warm, a.fade, a.min_keep)
            n_max = max(r[2] for r in plan) * hop
            t = _timed(lambda: eng.synthesize_folded(c, [F], plan, wav, seed=1), a.runs, a.long_s, a.long_runs)
            eng.synth_check()
            ms = (ctypes.c_double * 3)()
            assert lib.wn_test_fold_times(eng.h, ms) == 0
            pt = dict(_stats(t), rows_asked=rows, rows=len(plan), n_max=n_max, path=eng.synth_path, config=eng.synth_config(),
                      device_ms={'upsample_whole_utterance': ms[0], 'fold_kernel': ms[1], 'unfold_kernel': ms[2]})
            if name == 'paper':
                us, how = _predicted_us(slots_timing, len(plan))
                pt['predicted_s'] = n_max * us * 1e-6
                pt['predicted_from'] = '%d samples x %.2f us (%s)' % (n_max, us, how)
                pt['measured_over_predicted'] = pt['median_s'] / pt['predicted_s']
            if 'one_shot' in entry:
                pt['speedup_over_one_shot'] = entry['one_shot']['median_s'] / pt['median_s']
            pt['real_time_factor'] = pt['median_s'] / (T / float(hp.sample_rate))
            entry['points'][str(rows)] = pt
            flush()
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--models', default='paper,hparams,c5')
    ap.add_argument('--seconds', default='5,20')
    ap.add_argument('--rows', default='1,4,8,12,16,20,32')
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--long-s', type=float, default=1e9, help='a point whose first run takes longer than this is run --long-runs times in all')
    ap.add_argument('--long-runs', type=int, default=5)
    ap.add_argument('--warm', type=int, default=4)
    ap.add_argument('--fade', type=int, default=2)
    ap.add_argument('--min-keep', type=int, default=8, help='the planner never cuts below this many new frames per row (the façade default of 40 would stop a 5 s utterance at 10 rows)')
    ap.add_argument('--no-one-shot', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = {'what': 'wall time of one utterance: folded (wn_synthesize_folded) vs one-shot (wn_synthesize), device events, same session', 'models': {}}
    if a.out and os.path.exists(a.out):      # points of an earlier call are kept: long models are measured in calls of their own
        res = json.load(open(a.out))

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, 'w'), indent=1)

    for name in a.models.split(','):
        measure(a, name, res, flush)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
