"""Streaming synthesis timing (GPU): a 5 s utterance (22.05 kHz) on the paper model at 1, 8 and 20 streams, one wn_synthesize vs a stream fed
4, 8 and 16 mel frames per push, all frames available up front (the generation's own latency).  Device events on the caller's stream after a
warm-up, as bench.py times synthesis.  Reports per configuration: time to first audio (begin of the first push .. end of the first push that
returned samples), wall time per sample, RTF, and the fixed cost per push fitted over the chunk sizes (push time = a + b x samples).  Prints one
JSON line; --out writes it to a file (profiles/stream_timing.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tacotron-2_amd')):
    sys.path.insert(0, p)

PAPER = ('layers=24,stacks=2,residual_channels=256,gate_channels=512,skip_out_channels=256,cin_channels=80,num_mels=80,out_channels=30,'
         'upsample_type=2D,upsample_scales=[5,5,11],hop_size=275,legacy=False,residual_legacy=False')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', default='1,8,20')
    ap.add_argument('--chunks', default='4,8,16')
    ap.add_argument('--seconds', type=float, default=5.0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import hparams as H
    from wavenet_vocoder import _ext
    from wavenet_vocoder.models.modules import initialize_parameters
    hp = H._build(); hp.parse(PAPER)
    sr, hop = hp.sample_rate, int(np.prod(hp.upsample_scales))
    Tc = int(round(a.seconds * sr / hop)); T = Tc * hop
    chunks = [int(x) for x in a.chunks.split(',')]
    res = {'model': 'paper (24 layers / 2 stacks, R = S = 256, 10-MoL, 2D [5, 5, 11])', 'utterance_samples': T, 'frames': Tc, 'sample_rate': sr,
           'streams': {}}

    def ev():
        e = torch.cuda.Event(enable_timing=True); e.record(); return e

    for B in [int(x) for x in a.streams.split(',')]:
        eng = _ext.Engine(hp, B, T, inference_only=True)
        eng.pack_weights(initialize_parameters(hp, eng.layout, seed=5).cuda())
        c = torch.randn(B, hp.cin_channels, Tc, generator=torch.Generator().manual_seed(1)).cuda()
        out = torch.empty(B, T, device='cuda')
        eng.synthesize(c[:, :, :8].contiguous(), None, out[:, :8 * hop].contiguous(), seed=1)          # warm-up
        torch.cuda.synchronize(); eng.synth_check()
        e0 = ev(); eng.synthesize(c, None, out, seed=1); e1 = ev(); torch.cuda.synchronize(); eng.synth_check()
        one = e0.elapsed_time(e1) / 1e3
        row = {'path': eng.synth_config()['path'], 'one_shot': {'time_to_first_audio_ms': one * 1e3, 'us_per_sample': one / T * 1e6, 'rtf': one / (T / sr)}}
        per_push = {}
        for k in chunks:
            bufs = [torch.empty(B, k * hop, device='cuda') for _ in range(2)]
            eng.stream_begin(B, seed=1)
            evs = [ev()]
            first = None
            for i, f0 in enumerate(range(0, Tc, k)):
                f1 = min(Tc, f0 + k)
                n = eng.stream_push(c[:, :, f0:f1].contiguous(), bufs[i & 1], final=f1 == Tc)
                evs.append(ev())
                if first is None and n > 0:
                    first = len(evs) - 1
            torch.cuda.synchronize(); eng.synth_check()
            tot = evs[0].elapsed_time(evs[-1]) / 1e3
            pushes = [evs[i].elapsed_time(evs[i + 1]) / 1e3 for i in range(len(evs) - 1)]
            full = pushes[:-1] if Tc % k else pushes                                  # pushes of exactly k frames
            per_push[k] = float(np.median(full))
            row['chunk_%d' % k] = {'pushes': len(pushes), 'time_to_first_audio_ms': evs[0].elapsed_time(evs[first]), 'us_per_sample': tot / T * 1e6,
                                   'rtf': tot / (T / sr), 'median_push_ms': per_push[k] * 1e3}
        ks = np.array(sorted(per_push), dtype=np.float64)
        b, a0 = np.polyfit(ks * hop, np.array([per_push[int(x)] for x in ks]), 1)
        row['fixed_cost_per_push_us'] = a0 * 1e6
        row['us_per_sample_fit'] = b * 1e6
        res['streams'][str(B)] = row
        eng.close()
        print('[stream timing] %d streams done' % B, file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
