"""Sampling-temperature timing (GPU); device events on the caller's stream after a warm-up, one JSON line (--out writes it to a file:
profiles/temperature_timing.json).  Three measurements:

1. fill kernels: the plain device-noise fill (wn_fill_noise), the fill of a run at (0.7, 0.85) (the same kernel with the tempering fused into its
   store: wn_test_fill_noise_tempered) and the stand-alone wn_temper_noise at [T = 110275, B = 20, nps = 11] (MoL: 5 s of audio for 20 streams) and
   [T = 22050, B = 8, nps = 256] (softmax: 1 s for 8): median and p95 - p05 of --fill-repeats launches, and the tempered fill as a share of the span
   it precedes (T x the measured time per sample of the paper model at 20 streams);
2. existing paths unchanged: one wn_synthesize of the paper model at 1 and 20 streams and of hparams.py's model at 20 streams at (1, 1), per sample
   (the fill included), of THIS build and -- with --parent-lib PATH, a libwavenet_mi355.so built from the parent commit -- of the parent, alternating,
   --repeats times each, every arm in a child process of its own (WN_MI355_TEST_LIB selects the library).  Criterion (the one DESIGN 3.4 used for the
   slot sessions): this build's median inside the parent's min ... max widened by the parent's spread;
3. tempered runs: the same legs of this build at (0.7, 0.85) -- the sampling kernels are the same code, so there is no criterion of its own."""
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
TINY = 'layers=4,stacks=2,residual_channels=64,gate_channels=128,skip_out_channels=64,cin_channels=16,num_mels=16,upsample_type=2D,upsample_scales=[4,4],hop_size=16'
TAU = (0.7, 0.85)
NEW_SYMBOLS = ('wn_synth_set_temperature', 'wn_synth_get_temperature', 'wn_synth_set_slot_temperature', 'wn_temper_noise', 'wn_test_temper_noise',
               'wn_test_fill_noise_tempered')


def _ev():
    import torch
    e = torch.cuda.Event(enable_timing=True); e.record(); return e


def _hp(spec=None):
    import hparams as H
    hp = H._build()
    if spec:
        hp.parse(spec)
    return hp


def _engine(hp, B, T):
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.modules import initialize_parameters
    eng = _ext.Engine(hp, B, T, inference_only=True)
    eng.pack_weights(initialize_parameters(hp, eng.layout, seed=5).cuda())
    return eng


def _tolerate_missing_temperature_symbols():
    """the parent build has no temperature entry points: the binding resolves every name at load time, so give it stubs for those (that arm never calls them)"""
    import ctypes
    base = ctypes.CDLL

    class Lib(base):
        def __getattr__(self, name):
            try:
                return base.__getattr__(self, name)
            except AttributeError:
                if name not in NEW_SYMBOLS:
                    raise
                return ctypes.CFUNCTYPE(ctypes.c_int)(lambda *x: -4)
    ctypes.CDLL = Lib


def _stats(ms):
    v = np.asarray(ms, float) * 1e3
    return {'median_us': float(np.median(v)), 'p95_minus_p05_us': float(np.percentile(v, 95) - np.percentile(v, 5)), 'launches': int(v.size)}


def measure_fills(a):
    import torch
    res = {}
    for name, spec, T, B in (('mol', TINY + ',out_channels=30', 110275, 20), ('softmax', TINY + ',input_type=mulaw-quantize,quantize_channels=256,out_channels=256', 22050, 8)):
        hp = _hp(spec)
        eng = _engine(hp, 1, 16)                                 # (the fills take the head from the context and the shape from the call)
        nps = eng.noise_per_step
        nz, out = torch.empty(T, B, nps, device='cuda'), torch.empty(T, B, nps, device='cuda')
        legs = {'plain_fill': lambda: eng.fill_noise(nz, B, T, 3), 'tempered_fill': lambda: eng.fill_noise_tempered(nz, B, T, 3, *TAU),
                'temper_noise': lambda: eng.temper_noise(nz, *TAU, out=out)}
        row = {'shape': [T, B, nps], 'bytes': int(nz.numel()) * 4}
        for leg, fn in legs.items():
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.fill_repeats):
                e0 = _ev(); fn(); e1 = _ev(); torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            row[leg] = _stats(ms)
        res[name] = row
        eng.close()
    return res


def arm_legs(a):
    """one child: one wn_synthesize per leg of the library this process loaded, at (1, 1) and -- this build -- at TAU"""
    parent = bool(os.environ.get('WN_MI355_TEST_LIB'))
    if parent:
        _tolerate_missing_temperature_symbols()
    import torch
    res = {}
    for name, spec, B in (('paper_1', PAPER, 1), ('paper_20', PAPER, 20), ('hparams_20', None, 20)):
        hp = _hp(spec)
        hop = int(np.prod(hp.upsample_scales))
        Tc = a.frames; T = Tc * hop
        eng = _engine(hp, B, T)
        c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty(B, T, device='cuda')
        eng.synthesize(c[:, :, :8].contiguous(), None, out[:, :8 * hop].contiguous(), seed=1)
        torch.cuda.synchronize(); eng.synth_check()
        row = {}
        for key, pair in (('at_1', None), ('at_tau', TAU)):
            if pair is not None:
                if parent:
                    continue
                eng.set_temperature(*pair)
            e0 = _ev(); eng.synthesize(c, None, out, seed=1); e1 = _ev(); torch.cuda.synchronize(); eng.synth_check()
            row[key + '_us_per_sample'] = e0.elapsed_time(e1) * 1e3 / T
            row[key + '_whole_run_ms'] = e0.elapsed_time(e1)
        row['path'] = eng.synth_path
        res[name] = row
        eng.close()
    print('ARM ' + json.dumps(res))


def measure_legs(a):
    libs = [('this', None)] + ([('parent', a.parent_lib)] if a.parent_lib else [])
    runs = {k: [] for k, _ in libs}
    for r in range(a.repeats):
        for k, lib in reversed(libs) if r % 2 else libs:
            env = dict(os.environ)
            if lib:
                env['WN_MI355_TEST_LIB'] = os.path.abspath(lib)
            p = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.abspath(__file__), '--arm', 'legs', '--frames', str(a.frames)],
                               env=env, capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith('ARM ')]
            if p.returncode != 0 or not line:
                raise RuntimeError('arm %s failed (%d): %s' % (k, p.returncode, p.stderr[-800:]))      # (nothing more is started on the device)
            runs[k].append(json.loads(line[-1][4:]))
    out = {'frames': a.frames, 'repeats': a.repeats, 'temperature': list(TAU), 'runs': runs, 'unchanged': {}, 'tempered': {}}
    for leg in runs['this'][0]:
        tv = [r[leg]['at_1_us_per_sample'] for r in runs['this']]
        row = {'this': tv, 'this_median': float(np.median(tv))}
        if 'parent' in runs:
            pv = [r[leg]['at_1_us_per_sample'] for r in runs['parent']]
            spread = max(pv) - min(pv)
            row.update(parent=pv, parent_median=float(np.median(pv)), accept_lo=min(pv) - spread, accept_hi=max(pv) + spread)
            row['within'] = bool(row['accept_lo'] <= row['this_median'] <= row['accept_hi'])
        out['unchanged'][leg] = row
        xv = [r[leg]['at_tau_us_per_sample'] for r in runs['this']]
        out['tempered'][leg] = {'us_per_sample': xv, 'median_us_per_sample': float(np.median(xv)),
                                'median_whole_run_ms': float(np.median([r[leg]['at_tau_whole_run_ms'] for r in runs['this']])),
                                'median_whole_run_ms_at_1': float(np.median([r[leg]['at_1_whole_run_ms'] for r in runs['this']]))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', default=None)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--fill-repeats', type=int, default=50)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.arm == 'legs':
        return arm_legs(a)
    res = {'legs': measure_legs(a)}            # (children first: this process has not opened the device yet)
    res['fills'] = measure_fills(a)
    per_sample = res['legs']['unchanged']['paper_20']['this_median']
    f = res['fills']['mol']
    span_us = f['shape'][0] * per_sample
    f['span_us_at_paper_20'] = span_us
    f['tempered_fill_share_of_span'] = f['tempered_fill']['median_us'] / span_us
    f['extra_over_plain_fill_us'] = f['tempered_fill']['median_us'] - f['plain_fill']['median_us']
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, 'w') as fh:
            json.dump(res, fh, indent=1, sort_keys=True)
            fh.write('\n')


if __name__ == '__main__':
    main()
