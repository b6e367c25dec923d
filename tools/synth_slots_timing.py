"""Synthesis-slot timing (GPU), paper model on the pipeline unless stated; device events on the caller's stream after a warm-up, one JSON line
(--out writes it to a file: profiles/slots_timing.json).  Three measurements:

1. existing paths: per-sample time of one wn_synthesize and of a lockstep stream (8-frame pushes) at 1, 8, 12, 16, 20 streams (paper model) and 20
   streams (hparams.py's model), of THIS build and -- with --parent-lib PATH, a libwavenet_mi355.so built from the parent commit -- of the parent,
   alternating, --repeats times each, every arm in a child process of its own (WN_MI355_TEST_LIB selects the library);
2. what a session costs: all B slots live (equal utterances) vs the lockstep stream at the same B and push size, per sample, and the fixed cost per
   push fitted over pushes of 4, 8 and 16 frames (push time = a + b x samples);
3. what it buys: useful audio samples per second of padded batches (groups of B in input order, one wn_synthesize each, padded to the longest) vs one
   slot session driven by slot_plan (8-frame tick) at B = 12 and 20 on the first --utterances lengths of tests/golden/slot_lengths.json (a SYNTHETIC
   list), and the time from slot_open to the first samples of a late joiner next to 11 live slots."""
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


def _engine(hp, B, T):
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.modules import initialize_parameters
    eng = _ext.Engine(hp, B, T, inference_only=True)
    eng.pack_weights(initialize_parameters(hp, eng.layout, seed=5).cuda())
    return eng


def _hp(paper=True):
    import hparams as H
    hp = H._build()
    if paper:
        hp.parse(PAPER)
    return hp


def _stream_time(eng, c, k, hop, slots=False):
    """seconds for the whole utterance through 8-frame pushes: lockstep stream, or a session with every slot live; + the per-push times"""
    import torch
    B, Tc = int(c.shape[0]), int(c.shape[-1])
    bufs = [torch.empty(B, k * hop, device='cuda') for _ in range(2)]
    if slots:
        eng.slots_begin(B)
        for b in range(B):
            eng.slot_open(b, seed=1 + b)
    else:
        eng.stream_begin(B, seed=1)
    evs = [_ev()]
    ns = []
    for i, f0 in enumerate(range(0, Tc, k)):
        f1 = min(Tc, f0 + k)
        blk = c[:, :, f0:f1].contiguous()
        if slots:
            buf = bufs[i & 1] if f1 - f0 == k else torch.empty(B, (f1 - f0) * hop, device='cuda')
            n = max(eng.slots_push(blk, [f1 - f0] * B, [f1 == Tc] * B, buf))
        else:
            n = eng.stream_push(blk, bufs[i & 1], final=f1 == Tc)
        ns.append(n); evs.append(_ev())
    torch.cuda.synchronize(); eng.synth_check()
    per = [(ns[i], evs[i].elapsed_time(evs[i + 1]) / 1e3) for i in range(len(ns))]
    return evs[0].elapsed_time(evs[-1]) / 1e3, per


def _tolerate_missing_slot_symbols():
    """the parent build has no wn_synth_slot* entry points: the binding resolves every name at load time, so give it stubs for those (this arm never calls them)"""
    import ctypes
    base = ctypes.CDLL

    class Lib(base):
        def __getattr__(self, name):
            try:
                return base.__getattr__(self, name)
            except AttributeError:
                if not name.startswith('wn_synth_slot'):
                    raise
                return ctypes.CFUNCTYPE(ctypes.c_int)(lambda *x: -4)
    ctypes.CDLL = Lib


def arm_existing(a):
    """one child: one-shot and lockstep-stream time per sample of the library this process loaded"""
    if os.environ.get('WN_MI355_TEST_LIB'):
        _tolerate_missing_slot_symbols()
    import torch
    res = {}
    for name, paper, streams in (('paper', True, [int(x) for x in a.streams.split(',')]), ('hparams', False, [20])):
        hp = _hp(paper)
        hop = int(np.prod(hp.upsample_scales))
        Tc = a.frames; T = Tc * hop
        for B in streams:
            eng = _engine(hp, B, T)
            c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
            out = torch.empty(B, T, device='cuda')
            eng.synthesize(c[:, :, :8].contiguous(), None, out[:, :8 * hop].contiguous(), seed=1)
            torch.cuda.synchronize(); eng.synth_check()
            e0 = _ev(); eng.synthesize(c, None, out, seed=1); e1 = _ev(); torch.cuda.synchronize(); eng.synth_check()
            st, _ = _stream_time(eng, c, 8, hop)
            res['%s_%d' % (name, B)] = {'one_shot_us': e0.elapsed_time(e1) * 1e3 / T, 'stream_us': st * 1e6 / T}
            eng.close()
    print('ARM ' + json.dumps(res))


def measure_existing(a):
    libs = [('this', None)] + ([('parent', a.parent_lib)] if a.parent_lib else [])
    runs = {k: [] for k, _ in libs}
    for r in range(a.repeats):
        for k, lib in libs:
            env = dict(os.environ)
            if lib:
                env['WN_MI355_TEST_LIB'] = os.path.abspath(lib)
            p = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--arm', 'existing', '--streams', a.streams, '--frames', str(a.frames)],
                               env=env, capture_output=True, text=True)
            line = [l for l in p.stdout.splitlines() if l.startswith('ARM ')]
            if p.returncode != 0 or not line:
                raise RuntimeError('arm %s failed (%d): %s' % (k, p.returncode, p.stderr[-800:]))
            runs[k].append(json.loads(line[-1][4:]))
    out = {'frames': a.frames, 'repeats': a.repeats, 'runs': runs, 'summary': {}}
    for cfgk in runs['this'][0]:
        for m in ('one_shot_us', 'stream_us'):
            row = {'this_median': float(np.median([r[cfgk][m] for r in runs['this']])), 'this': [r[cfgk][m] for r in runs['this']]}
            if 'parent' in runs:
                pv = [r[cfgk][m] for r in runs['parent']]
                spread = max(pv) - min(pv)
                row.update(parent=pv, parent_median=float(np.median(pv)), accept_lo=min(pv) - spread, accept_hi=max(pv) + spread)
                row['within'] = bool(row['accept_lo'] <= row['this_median'] <= row['accept_hi'])
            out['summary']['%s.%s' % (cfgk, m)] = row
    return out


def measure_session_cost(a):
    import torch
    hp = _hp(True)
    hop = int(np.prod(hp.upsample_scales))
    Tc = a.frames; T = Tc * hop
    res = {}
    for B in (1, 8, 12, 20):
        eng = _engine(hp, B, T)
        c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
        _stream_time(eng, c[:, :, :16].contiguous(), 8, hop); _stream_time(eng, c[:, :, :16].contiguous(), 8, hop, slots=True)      # warm-up
        row = {}
        for slots in (False, True):
            pts = []
            tot8 = None
            for k in (4, 8, 16):
                tot, per = _stream_time(eng, c, k, hop, slots=slots)
                pts += [(n, t) for n, t in per[1:] if n == k * hop]
                if k == 8:
                    tot8 = tot
            x = np.array([p[0] for p in pts], float); y = np.array([p[1] for p in pts], float)
            bb, aa = np.polyfit(x, y, 1)
            row['session' if slots else 'stream'] = {'us_per_sample_8_frame_pushes': tot8 * 1e6 / T, 'fixed_ms_per_push': aa * 1e3, 'us_per_sample_slope': bb * 1e6}
        res[str(B)] = row
        eng.close()
    return res


def measure_throughput(a):
    import torch
    from wavenet_vocoder.models.wavenet import slot_plan
    d = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'slot_lengths.json')))
    lengths = d['frames'][:a.utterances]
    hp = _hp(True)
    hop = int(np.prod(hp.upsample_scales))
    tick = 8
    res = {'lengths': 'first %d of tests/golden/slot_lengths.json (synthetic)' % len(lengths), 'useful_samples': int(sum(lengths)) * hop, 'tick_frames': tick}
    for B in (12, 20):
        eng = _engine(hp, B, max(lengths) * hop)
        g = torch.Generator().manual_seed(2)
        mels = [torch.randn(hp.cin_channels, n, generator=g) for n in lengths]
        # padded batches
        out = torch.empty(B, max(lengths) * hop, device='cuda')
        eng.synthesize(torch.zeros(B, hp.cin_channels, 8, device='cuda'), None, out[:, :8 * hop].contiguous(), seed=1)
        torch.cuda.synchronize()
        e0 = _ev()
        for i in range(0, len(lengths), B):
            grp = mels[i:i + B]
            Tc = max(m.shape[-1] for m in grp)
            c = torch.zeros(len(grp), hp.cin_channels, Tc)
            for j, m in enumerate(grp):
                c[j, :, :m.shape[-1]] = m
            eng.synthesize(c.cuda(), None, torch.empty(len(grp), Tc * hop, device='cuda'), seed=3 + i)
        e1 = _ev(); torch.cuda.synchronize(); eng.synth_check()
        padded = e0.elapsed_time(e1) / 1e3
        # one slot session
        eng.slots_begin(B)
        owner, sent, pushes = [None] * B, [0] * len(lengths), 0
        bufs = [torch.empty(B, (tick + 1) * hop, device='cuda') for _ in range(2)]
        e0 = _ev()
        for opens, frames, final in slot_plan(lengths, B, tick):
            for b, u in opens:
                eng.slot_open(b, seed=100 + u); owner[b] = u
            c = torch.zeros(B, hp.cin_channels, tick)
            for b in range(B):
                if owner[b] is not None:
                    u = owner[b]
                    c[b, :, :frames[b]] = mels[u][:, sent[u]:sent[u] + frames[b]]
                    sent[u] += frames[b]
                    if final[b]:
                        owner[b] = None
            eng.slots_push(c.cuda(), frames, final, bufs[pushes & 1])
            pushes += 1
        e1 = _ev(); torch.cuda.synchronize(); eng.synth_check()
        sess = e0.elapsed_time(e1) / 1e3
        res[str(B)] = {'padded_s': padded, 'session_s': sess, 'pushes': pushes, 'padded_useful_samples_per_s': res['useful_samples'] / padded,
                       'session_useful_samples_per_s': res['useful_samples'] / sess, 'speedup': padded / sess}
        if B == 12:      # a late joiner next to 11 live slots: slot_open .. its first samples, 8-frame pushes
            eng.slots_begin(B)
            for b in range(11):
                eng.slot_open(b, seed=b)
            c = torch.randn(B, hp.cin_channels, tick, generator=g).cuda()
            for _ in range(3):
                eng.slots_push(c, [tick] * 11 + [0], [False] * B, bufs[0])
            torch.cuda.synchronize()
            e0 = _ev(); eng.slot_open(11, seed=99); n = eng.slots_push(c, [tick] * B, [False] * B, bufs[1]); e1 = _ev()
            torch.cuda.synchronize(); eng.synth_check()
            res['late_joiner_first_audio_ms'] = e0.elapsed_time(e1)
            res['late_joiner_samples'] = n[11]
        eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', default=None)
    ap.add_argument('--streams', default='1,8,12,16,20')
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--utterances', type=int, default=100)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--only', default='1,2,3')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.arm == 'existing':
        return arm_existing(a)
    res = {'model': 'paper (24 layers / 2 stacks, R = S = 256, 10-MoL, 2D [5, 5, 11])'}

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            json.dump(res, open(a.out, 'w'), indent=1)

    if '2' in a.only:
        res['session_vs_stream'] = measure_session_cost(a); flush()
    if '3' in a.only:
        res['throughput'] = measure_throughput(a); flush()
    if '1' in a.only:
        res['existing_paths'] = measure_existing(a); flush()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
