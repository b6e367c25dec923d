#!/usr/bin/env python3
"""Device time of a streaming mel-analysis push (csrc/wn_mel_stream.hip) -> profiles/mel_stream_timing.json.

    python tools/mel_stream_timing.py [--parent-lib PATH] [--out profiles/mel_stream_timing.json]

hipEvent medians of 30 pushes after 3 warm-ups (p05 / p95 beside them) of MelStream.push with 2 200 samples per row at 20 rows and at 1 row, default geometry
(2048 / 1100 / 275), pre-emphasis 0.97, every row in steady state (each push analyses 8 new frames in ONE mostly empty 32-frame tile per row).  Beside each: the
slot push it precedes, from the recorded figures of profiles/slots_timing.json, and the host path it replaces: numpy datasets.audio.melspectrogram (float64) of the
chunk with the win_size samples of context in front of it, per row, scaled to the rows.  The shader and memory clocks are read right after every timed loop.
--parent-lib: wn_mel_run after the refactor -- the three cases of tools/mel_timing.py (1 x 5 s, 20 x 9 s, 64 x 9 s; the library's own tile pick, its event
loop) on the parent commit's library and on this one, each in a child process of its own through WN_MI355_TEST_LIB, alternating, three runs each."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tacotron-2_amd'), os.path.join(ROOT, 'tools')):
    sys.path.insert(0, p)

PUSH, PRE = 2200, 0.97


def run_child():
    """wn_mel_run on the cases of tools/mel_timing.py with this process' library: one JSON line"""
    if os.environ.get('WN_MI355_TEST_LIB'):
        from mel_identity import _tolerate_missing_stream_symbols
        _tolerate_missing_stream_symbols()
    import torch
    from mel_timing import _events
    from mel_util import mel_hparams
    from wavenet_vocoder import _ext
    hp = mel_hparams()
    hop = hp.hop_size
    rng = np.random.RandomState(0)
    res = {}
    for name, B, n in (('1x5s', 1, 5 * hp.sample_rate), ('20x9s', 20, 899 * hop + 100), ('64x9s', 64, 899 * hop + 100)):
        wav = torch.from_numpy((0.1 * rng.randn(B, n)).astype(np.float32)).cuda()
        an = _ext.MelAnalyzer(hp, B, n)
        out = torch.empty(B, 1 + n // hop, hp.num_mels, device='cuda')
        res[name] = _events(lambda: an.run(wav, [n] * B, out=out), 3, 20)
        an.close()
    print('MELRUN ' + json.dumps(res))


def _child(lib):
    env = dict(os.environ)
    env.pop('WN_MI355_TEST_LIB', None)
    if lib:
        env['WN_MI355_TEST_LIB'] = os.path.abspath(lib)
    p = subprocess.run(['timeout', '-k', '10', '200', sys.executable, os.path.abspath(__file__), '--child'], env=env, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith('MELRUN ')]
    if p.returncode != 0 or not line:
        raise RuntimeError('child (%s) failed (%d): %s' % (lib or 'this', p.returncode, p.stderr[-1500:]))
    return json.loads(line[-1][7:])


def run_ab(parent_lib):
    runs = {'parent': [], 'this': []}
    for _ in range(3):
        runs['parent'].append(_child(parent_lib))
        runs['this'].append(_child(None))
    res = {'what': 'wn_mel_run, default geometry, the library\'s own tile pick; tools/mel_timing.py\'s event loop (3 warm-ups, 20 calls); parent and this build alternating, three '
                   'child processes each', 'cases': {}}
    for case in runs['this'][0]:
        pm = [r[case]['median_ms'] for r in runs['parent']]
        tm = [r[case]['median_ms'] for r in runs['this']]
        lo, hi = min(r[case]['min_ms'] for r in runs['parent']), max(r[case]['max_ms'] for r in runs['parent'])
        res['cases'][case] = {'parent_median_ms': pm, 'this_median_ms': tm, 'parent_calls_min_ms': lo, 'parent_calls_max_ms': hi,
                              'this_medians_inside_parent_median_range': bool(min(pm) <= float(np.median(tm)) <= max(pm)),
                              'this_medians_inside_parent_call_range': bool(all(lo <= v <= hi for v in tm))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--child', action='store_true')
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mel_stream_timing.json'))
    args = ap.parse_args()
    if args.child:
        return run_child()
    import torch
    from datasets import audio
    from denoise_stream_timing import events_of, synthesis_push_ms
    from mel_util import mel_hparams
    from wavenet_vocoder import _ext
    hp = mel_hparams()
    res = {'what': 'tools/mel_stream_timing.py: hipEvent medians of 30 pushes after 3 warm-ups, geometry (2048, 1100, 275), pre-emphasis 0.97, pushes of 2200 samples (8 frames) '
                   'per row, rows in steady state; clocks_after: rocm-smi --showclocks right after the timed loop of the case',
           'device': torch.cuda.get_device_name(0), 'cases': {},
           'not_measured': ['the slot push itself (the figure of profiles/slots_timing.json is taken as recorded, paper model)', 'pushes that end or restart rows',
                            'geometries other than the default', 'frame tiles above 32 (not built for the stream)', 'LiveVocoder end to end on a trained model']}
    synth = synthesis_push_ms()
    rs = np.random.RandomState(0)
    for B in (20, 1):
        host = (0.1 * rs.randn(B, PUSH)).astype(np.float32)
        x = torch.from_numpy(host).cuda()
        ms = _ext.MelStream(hp, B, PUSH, preemphasis=PRE)
        out = torch.empty(B, hp.num_mels, PUSH // ms.hop + 6, device='cuda')
        ms.push(x, restart=True, gain=[0.9] * B, out=out)
        case = {'rows': B, 'samples_per_row': PUSH, 'stream_push': events_of(lambda: ms.push(x, out=out))}
        ctx = np.concatenate([(0.1 * rs.randn(hp.win_size)).astype(np.float32), host[0]]).astype(np.float64)
        t0 = time.perf_counter()
        for _ in range(5):
            audio.melspectrogram(audio.preemphasis(ctx, PRE, True), hp)
        per = (time.perf_counter() - t0) / 5 * 1e3
        case['numpy_float64_host'] = {'ms_per_row': per, 'ms_for_rows_scaled': per * B, 'samples_analysed_per_row': int(ctx.size), 'host_threads_available': len(os.sched_getaffinity(0))}
        if B in synth:
            case['slot_push_ms'], case['slot_push_source'] = synth[B]
            case['stream_share_of_slot_push'] = case['stream_push']['median_ms'] / case['slot_push_ms']
        res['cases']['%d rows' % B] = case
        ms.close()
    if args.parent_lib:
        res['wn_mel_run_after_the_refactor'] = run_ab(args.parent_lib)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, indent=1, sort_keys=True))


if __name__ == '__main__':
    main()
