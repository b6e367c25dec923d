"""Wide-synthesis timing (GPU): what wn_synthesize_wide delivers, against the pipeline as WaveNet.incremental runs it, and what the tile index costs the
existing launch-per-layer run.  Device events on the caller's stream around the call after a warm-up run of the same call (so the captured graph exists),
profiler off, every arm in a child process of its own; --out writes the JSON (profiles/wide_timing.json).

1. wide: paper model (24 layers / 2 stacks, R = 256), hparams.py's model, 40 frames (11 000 steps at hop 275), B = 32 ... 1 024; C5 width (bench.py's
   c5_stress, 40 frames of hop 300) at B = 32 and 256.  us per step = event time / steps, samples per second = B / that; medians of --repeats with p05 / p95.
2. yardstick: the same utterances through WaveNet.incremental on an inference-only context, in calls of the largest group the pipeline takes (what
   incremental() makes of a larger batch today); with --parent-lib PATH (a libwavenet_mi355.so built from the parent commit) on that library.  One child
   per B, alternating with the wide child of the same B.  Beyond 128 streams a leg is measured once (its time is the group's time x the groups).
3. existing: wn_synthesize(steps_per_graph = 32) of the paper model at B = 1, 8, 32, --parent-lib against this build, alternating, three children each;
   accepted when the median of this build lies inside the parent's min ... max widened by its spread (profiles/slots_timing.json -> existing_paths)."""
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


def _ev():
    import torch
    e = torch.cuda.Event(enable_timing=True); e.record(); return e


def _hp(model):
    import hparams as H
    if model == 'c5':
        import bench
        return bench.build_hparams('c5_stress')[0]
    hp = H._build()
    if model == 'paper':
        hp.parse(PAPER)
    return hp


def _params(hp, eng):
    from wavenet_vocoder.models.modules import initialize_parameters
    return initialize_parameters(hp, eng.layout, seed=5)


def _tolerate_missing_wide_symbol():
    """a parent build may lack wn_synthesize_wide / wn_synth_wide_slots_begin: the binding resolves every name at load time, so give it a stub (these arms never call it)"""
    import ctypes
    base = ctypes.CDLL

    class Lib(base):
        def __getattr__(self, name):
            try:
                return base.__getattr__(self, name)
            except AttributeError:
                if name not in ('wn_synthesize_wide', 'wn_synth_wide_slots_begin'):
                    raise
                return ctypes.CFUNCTYPE(ctypes.c_int)(lambda *x: -4)
    ctypes.CDLL = Lib


def _summary(us, B):
    us = [float(v) for v in us]
    med = float(np.median(us))
    return {'us_per_step': us, 'median_us_per_step': med, 'p05_us_per_step': float(np.percentile(us, 5)), 'p95_us_per_step': float(np.percentile(us, 95)),
            'samples_per_s': B / med * 1e6}


def arm_wide(a):
    if os.environ.get('WN_MI355_TEST_LIB'):
        _tolerate_missing_wide_symbol()
    import torch
    from wavenet_vocoder import _ext
    hp = _hp(a.model)
    hop = int(np.prod(hp.upsample_scales))
    B, Tc = int(a.streams), a.frames
    T = Tc * hop
    eng = _ext.Engine(hp, B, T, inference_only=True)
    eng.pack_weights(_params(hp, eng).cuda())
    c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.empty(B, T, device='cuda', dtype=torch.float32 if hp.input_type != 'mulaw-quantize' else torch.int32)
    us = []
    for r in range(a.repeats + 1):                     # (run 0: the warm-up, it captures the graph)
        e0 = _ev(); eng.synthesize_wide(c, None, out, steps_per_graph=32, seed=1); e1 = _ev()
        torch.cuda.synchronize(); eng.synth_check()
        if r:
            us.append(e0.elapsed_time(e1) * 1e3 / T)
    assert eng.synth_path == 'graph' and bool(torch.isfinite(out.float()).all())
    eng.close()
    print('ARM ' + json.dumps(dict(_summary(us, B), steps=T, streams=B)))


def arm_yard(a):
    if os.environ.get('WN_MI355_TEST_LIB'):
        _tolerate_missing_wide_symbol()
    import torch
    from wavenet_vocoder.models.wavenet import WaveNet
    hp = _hp(a.model)
    hop = int(np.prod(hp.upsample_scales))
    B, Tc = int(a.streams), a.frames
    T = Tc * hop
    model = WaveNet(hp)
    model.build(min(B, 32), T, inference_only=True)
    model.params.copy_(_params(hp, model.engine).cuda()); model._dirty = True
    group = min(B, 32)
    while group > 0 and not model.engine.pipeline_eligible(group):
        group -= 1
    if group == 0:
        print('ARM ' + json.dumps({'pipeline': False}))
        return
    c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()

    def once():
        for b0 in range(0, B, group):
            model.incremental(None, c=c[b0:b0 + group], check=False)

    model.incremental(None, c=c[:group, :, :8].contiguous(), check=True)      # warm-up: the pipeline's weight images, the noise buffer
    us = []
    for r in range(a.repeats):
        e0 = _ev(); once(); e1 = _ev()
        torch.cuda.synchronize(); model.engine.synth_check()
        us.append(e0.elapsed_time(e1) * 1e3 / T)
    assert model.engine.synth_path == 'pipeline'
    model.engine.close()
    print('ARM ' + json.dumps(dict(_summary(us, B), pipeline=True, group=group, runs=-(-B // group), steps=T, streams=B)))


def arm_existing(a):
    if os.environ.get('WN_MI355_TEST_LIB'):
        _tolerate_missing_wide_symbol()
    import torch
    from wavenet_vocoder import _ext
    hp = _hp('paper')
    hop = int(np.prod(hp.upsample_scales))
    Tc = a.frames; T = Tc * hop
    res = {}
    for B in [int(x) for x in a.streams.split(',')]:
        eng = _ext.Engine(hp, B, T, inference_only=True)
        eng.pack_weights(_params(hp, eng).cuda())
        c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty(B, T, device='cuda')
        for r in range(2):
            e0 = _ev(); eng.synthesize(c, None, out, steps_per_graph=32, seed=1); e1 = _ev()
            torch.cuda.synchronize(); eng.synth_check()
        assert eng.synth_path == 'graph'
        res[str(B)] = e0.elapsed_time(e1) * 1e3 / T
        eng.close()
    print('ARM ' + json.dumps(res))


def _child(arm, a, model, streams, repeats, lib=None, limit=600):
    env = dict(os.environ)
    env.pop('WN_MI355_TEST_LIB', None)
    if lib:
        env['WN_MI355_TEST_LIB'] = os.path.abspath(lib)
    p = subprocess.run(['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__), '--arm', arm, '--model', model, '--streams', str(streams),
                        '--frames', str(a.frames), '--repeats', str(repeats)], env=env, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith('ARM ')]
    if p.returncode != 0 or not line:
        raise RuntimeError('arm %s %s B=%s failed (%d): %s' % (arm, model, streams, p.returncode, p.stderr[-1500:]))
    return json.loads(line[-1][4:])


def measure_wide(a, model, streams, yard=True):
    res = {'frames': a.frames, 'wide': {}, 'incremental': {}}
    for B in streams:
        res['wide'][str(B)] = _child('wide', a, model, B, a.repeats)
        print('%s wide B=%d: %.1f us per step, %.3f M samples/s' % (model, B, res['wide'][str(B)]['median_us_per_step'], res['wide'][str(B)]['samples_per_s'] / 1e6), flush=True)
        if yard:
            res['incremental'][str(B)] = y = _child('yard', a, model, B, 3 if B <= 128 else 1, lib=a.parent_lib)
            if y.get('pipeline'):
                print('%s incremental B=%d (%d runs of <= %d): %.1f us per step, %.3f M samples/s' % (model, B, y['runs'], y['group'], y['median_us_per_step'], y['samples_per_s'] / 1e6), flush=True)
    if yard and all(v.get('pipeline') for v in res['incremental'].values()):
        ahead = [B for B in streams if res['wide'][str(B)]['samples_per_s'] > res['incremental'][str(B)]['samples_per_s']]
        res['incremental_library'] = 'parent' if a.parent_lib else 'this'
        res['wide_ahead_from_B'] = min(ahead) if ahead else None
        res['wide_ahead_at'] = ahead
    return res


def measure_wide_vs_parent(a, model, streams):
    """wn_synthesize_wide itself, --parent-lib against this build: children alternate (parent, this, parent, this), --repeats runs each; accepted when the
    median of this build lies inside the parent's own p05 ... p95 of the session"""
    out = {'frames': a.frames, 'model': model, 'summary': {}}
    for B in streams:
        us = {'parent': [], 'this': []}
        for r in range(2):
            for k, lib in (('parent', a.parent_lib), ('this', None)):
                us[k] += _child('wide', a, model, B, a.repeats, lib=lib)['us_per_step']
        pv = us['parent']
        row = {'this': us['this'], 'this_median': float(np.median(us['this'])), 'parent': pv, 'parent_median': float(np.median(pv)),
               'parent_p05': float(np.percentile(pv, 5)), 'parent_p95': float(np.percentile(pv, 95))}
        row['within'] = bool(row['parent_p05'] <= row['this_median'] <= row['parent_p95'])
        out['summary']['%s_%d.us_per_step' % (model, B)] = row
        print('wide %s B=%d: parent %.2f [%.2f, %.2f], this %.2f us per step' % (model, B, row['parent_median'], row['parent_p05'], row['parent_p95'], row['this_median']), flush=True)
    return out


def measure_existing(a):
    libs = [('this', None)] + ([('parent', a.parent_lib)] if a.parent_lib else [])
    runs = {k: [] for k, _ in libs}
    for r in range(3):
        for k, lib in libs[::-1]:
            runs[k].append(_child('existing', a, 'paper', '1,8,32', 1, lib=lib))
            print('existing %s: %s' % (k, runs[k][-1]), flush=True)
    out = {'frames': a.frames, 'steps_per_graph': 32, 'runs': runs, 'summary': {}}
    for B in runs['this'][0]:
        row = {'this': [r[B] for r in runs['this']], 'this_median': float(np.median([r[B] for r in runs['this']]))}
        if 'parent' in runs:
            pv = [r[B] for r in runs['parent']]
            spread = max(pv) - min(pv)
            row.update(parent=pv, parent_median=float(np.median(pv)), accept_lo=min(pv) - spread, accept_hi=max(pv) + spread)
            row['within'] = bool(row['accept_lo'] <= row['this_median'] <= row['accept_hi'])
        out['summary']['paper_%s.us_per_step' % B] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', default=None)
    ap.add_argument('--model', default='paper')
    ap.add_argument('--streams', default='32,64,128,256,512,1024')
    ap.add_argument('--frames', type=int, default=40)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--only', default='existing,paper,hparams,c5')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.arm:
        return {'wide': arm_wide, 'yard': arm_yard, 'existing': arm_existing}[a.arm](a)
    res = {}
    if a.out and os.path.exists(a.out):
        res = json.load(open(a.out))               # (a session may be split over several invocations: --only)
    res['method'] = 'hipEvent time of the call / steps after a warm-up run of the same call; profiler off; every arm a child process'

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, 'w'), indent=1)

    streams = [int(x) for x in a.streams.split(',')]
    for part in a.only.split(','):
        if part == 'existing':
            res['existing_path'] = measure_existing(a)
        elif part == 'wide_vs_parent':
            res['wide_vs_parent'] = measure_wide_vs_parent(a, 'paper', streams)
        elif part == 'c5':
            res['c5_width'] = measure_wide(a, 'c5', [b for b in (32, 256)], yard=False)
        else:
            res[part] = measure_wide(a, part, streams)
        flush()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
